// Second translation unit of tests/cpp_dot: every dot function of the header surface, instantiated again, must link without
// duplicate symbols.  Returns 0 when poly_p and device_batch agree with nfl::dot on nfl::poly.
#include <nfl.hpp>

#include <cstring>
#include <vector>

int other_tu_dot() {
  typedef nfl::poly<uint64_t, 64, 3> P;
  typedef nfl::poly_p<uint64_t, 64, 3> PP;
  const size_t terms = 3;
  int bad = 0;
  std::vector<P> a(terms), b(terms);
  for (size_t j = 0; j < terms; ++j) {
    a[j] = P(nfl::uniform(7 + j));
    b[j] = P(nfl::uniform(70 + j));
  }
  P want, twice;
  nfl::dot(want, a.data(), b.data(), terms);
  twice = want;
  nfl::dot_add(twice, a.data(), b.data(), terms);
  P sum = want + want;
  bad += !(twice == sum);
  std::vector<PP> pa, pb;
  for (size_t j = 0; j < terms; ++j) {
    pa.push_back(PP(a[j]));
    pb.push_back(PP(b[j]));
  }
  PP out;
  nfl::dot(out, pa.data(), pb.data(), terms);
  bad += !(out.poly_obj() == want);
  nfl::dot_add(out, pa.data(), pb.data(), terms);
  bad += !(out.poly_obj() == sum);
  nfl::device_batch<P> da(terms), db(terms), d1(1);
  da.upload(a.data());
  db.upload(b.data());
  d1.assign_dot(da, db, terms);
  P w;
  d1.download(&w);
  bad += std::memcmp(w.cdata(), want.cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  d1.assign_matvec(da, db);
  d1.download(&w);
  bad += std::memcmp(w.cdata(), want.cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  return bad;
}
