// Second translation unit of tests/cpp_automorphism: every automorphism function of the header surface, instantiated again,
// must link without duplicate symbols.  Returns 0 when sigma_3 then sigma_3^-1 (mod 2n) is the identity on every path.
#include <nfl.hpp>

#include <cstring>
#include <vector>

int other_tu_automorphism() {
  typedef nfl::poly<uint64_t, 64, 3> P;
  const uint64_t k = 3, kinv = 171;  // 3 * 171 = 513 = 1 mod 128
  const size_t bytes = sizeof(uint64_t) * 64 * 3;
  int bad = 0;
  P a(nfl::uniform(7)), t, u;
  nfl::automorphism(t, a, k);
  nfl::automorphism(u, t, kinv);
  bad += std::memcmp(u.cdata(), a.cdata(), bytes) != 0;
  P an(a);
  an.ntt_pow_phi();
  nfl::automorphism_ntt(t, an, k);
  nfl::automorphism_ntt(u, t, kinv);
  bad += std::memcmp(u.cdata(), an.cdata(), bytes) != 0;
  nfl::poly_p<uint64_t, 64, 3> pa(a), pt, pu;
  nfl::automorphism(pt, pa, k);
  nfl::automorphism(pu, pt, kinv);
  bad += !(pu.poly_obj() == a);
  nfl::automorphism_ntt(pt, pa, k);
  nfl::automorphism_ntt(pu, pt, kinv);
  bad += !(pu.poly_obj() == a);
  std::vector<P> h(2, a), w(2);
  nfl::device_batch<P> b0(2), b1(2), b2(2);
  b0.upload(h.data());
  b1.assign_automorphism(b0, k, true);
  nfl::device_batch<P> *o[1] = {&b2};
  const uint64_t ks[1] = {kinv};
  nfl::device_batch<P>::assign_automorphisms(o, ks, 1, b1, true);
  b2.download(w.data());
  bad += std::memcmp(w[1].cdata(), a.cdata(), bytes) != 0;
  nfl::sharded_batch<P> s0(2, std::vector<int>{0}), s1(2, std::vector<int>{0}), s2(2, std::vector<int>{0});
  s0.upload(h.data());
  s1.assign_automorphism(s0, k);
  nfl::sharded_batch<P> *so[1] = {&s2};
  nfl::sharded_batch<P>::assign_automorphisms(so, ks, 1, s1);
  s2.download(w.data());
  bad += std::memcmp(w[0].cdata(), a.cdata(), bytes) != 0;
  return bad;
}
