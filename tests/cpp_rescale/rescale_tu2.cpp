// Second translation unit of tests/cpp_rescale: every rescale function of the header surface, instantiated again, must link
// without duplicate symbols.  Returns 0 when every path agrees with nfl::rescale on nfl::poly, chained over two moduli.
#include <nfl.hpp>

#include <cstring>
#include <vector>

int other_tu_rescale() {
  typedef nfl::poly<uint64_t, 64, 3> P3;
  typedef nfl::poly<uint64_t, 64, 2> P2;
  typedef nfl::poly<uint64_t, 64, 1> P1;
  int bad = 0;
  P3 a(nfl::uniform(7));
  P2 m;
  P1 want;
  nfl::rescale(m, a);
  nfl::rescale(want, m);   // 3 -> 2 -> 1 moduli
  P3 an(a);
  an.ntt_pow_phi();
  P2 mn;
  P1 gn;
  nfl::rescale_ntt(mn, an);
  nfl::rescale_ntt(gn, mn);
  gn.invntt_pow_invphi();
  bad += std::memcmp(gn.cdata(), want.cdata(), sizeof(uint64_t) * 64) != 0;
  nfl::poly_p<uint64_t, 64, 3> pa(a);
  nfl::poly_p<uint64_t, 64, 2> pm;
  nfl::poly_p<uint64_t, 64, 1> pg;
  nfl::rescale(pm, pa);
  nfl::rescale(pg, pm);
  bad += !(pg.poly_obj() == want);
  pa.ntt_pow_phi();
  nfl::rescale_ntt(pm, pa);
  nfl::rescale_ntt(pg, pm);
  pg.invntt_pow_invphi();
  bad += !(pg.poly_obj() == want);
  std::vector<P3> h(2, a);
  std::vector<P1> w(2);
  nfl::device_batch<P3> b3(2);
  nfl::device_batch<P2> b2(2);
  nfl::device_batch<P1> b1(2);
  b3.upload(h.data());
  b2.assign_rescale(b3);
  b1.assign_rescale(b2);
  b1.download(w.data());
  bad += std::memcmp(w[1].cdata(), want.cdata(), sizeof(uint64_t) * 64) != 0;
  nfl::sharded_batch<P3> s3(2, std::vector<int>{0});
  nfl::sharded_batch<P2> s2(2, std::vector<int>{0});
  s3.upload(h.data());
  s2.assign_rescale(s3);
  std::vector<P2> w2(2);
  s2.download(w2.data());
  bad += std::memcmp(w2[0].cdata(), m.cdata(), sizeof(uint64_t) * 64 * 2) != 0;
  return bad;
}
