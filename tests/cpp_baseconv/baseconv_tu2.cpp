// Second translation unit of tests/cpp_baseconv: every base conversion function of the header surface, instantiated again, must
// link without duplicate symbols.  Returns 0 when every path agrees with nfl::base_convert / nfl::mod_down on nfl::poly.
#include <nfl.hpp>

#include <cstring>
#include <vector>

int other_tu_baseconv() {
  typedef nfl::poly<uint64_t, 64, 3> P3;
  typedef nfl::poly<uint64_t, 64, 1> P1;
  int bad = 0;
  P3 a(nfl::uniform(7));
  P3 up(a);
  nfl::base_convert(up, 2, 1, 0, 3, true);   // the last row spread over every row
  P1 want;
  nfl::mod_down(want, a);                    // 3 -> 1 moduli
  nfl::poly_p<uint64_t, 64, 3> pa(a);
  nfl::poly_p<uint64_t, 64, 1> pg;
  nfl::mod_down(pg, pa);
  bad += !(pg.poly_obj() == want);
  nfl::base_convert(pa, 2, 1, 0, 3, true);
  bad += !(pa.poly_obj() == up);
  std::vector<P3> h(2, a), hu(2);
  std::vector<P1> w(2);
  nfl::device_batch<P3> b3(2);
  nfl::device_batch<P1> b1(2);
  b3.upload(h.data());
  b1.assign_mod_down(b3);
  b1.download(w.data());
  bad += std::memcmp(w[1].cdata(), want.cdata(), sizeof(uint64_t) * 64) != 0;
  b3.assign_base_convert(b3, 2, 1, 0, 3, true);
  b3.download(hu.data());
  bad += std::memcmp(hu[0].cdata(), up.cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  nfl::sharded_batch<P3> s3(2, std::vector<int>{0});
  nfl::sharded_batch<P1> s1(2, std::vector<int>{0});
  s3.upload(h.data());
  s1.assign_mod_down(s3);
  s1.download(w.data());
  bad += std::memcmp(w[0].cdata(), want.cdata(), sizeof(uint64_t) * 64) != 0;
  s3.assign_base_convert(s3, 2, 1, 0, 3, true);
  s3.download(hu.data());
  bad += std::memcmp(hu[1].cdata(), up.cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  return bad;
}
