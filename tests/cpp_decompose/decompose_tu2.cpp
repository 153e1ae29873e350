// Second translation unit of tests/cpp_decompose: every decomposition function of the header surface, instantiated again, must
// link without duplicate symbols.  Returns 0 when poly_p and device_batch agree with nfl::decompose / nfl::gadget_mul on nfl::poly.
#include <nfl.hpp>

#include <cstring>
#include <vector>

int other_tu_decompose() {
  typedef nfl::poly<uint64_t, 64, 3> P;
  typedef nfl::poly_p<uint64_t, 64, 3> PP;
  const int w = 16;
  const size_t terms = nfl::gadget_terms<P>(w);
  int bad = terms != 3 * 4;
  P x(nfl::uniform(7));
  std::vector<P> want(terms), want_n(terms), want_g(terms);
  nfl::decompose(want.data(), x, w, true);
  nfl::decompose_ntt(want_n.data(), x, w, true);
  nfl::gadget_mul(want_g.data(), x, w);
  for (size_t j = 0; j < terms; ++j) {
    P t = want[j];
    t.ntt_pow_phi();
    bad += !(t == want_n[j]);
  }
  PP px(x);
  std::vector<PP> out(terms);
  nfl::decompose(out.data(), px, w, true);
  for (size_t j = 0; j < terms; ++j) bad += !(out[j].poly_obj() == want[j]);
  nfl::decompose_ntt(out.data(), px, w, true);
  for (size_t j = 0; j < terms; ++j) bad += !(out[j].poly_obj() == want_n[j]);
  nfl::gadget_mul(out.data(), px, w);
  for (size_t j = 0; j < terms; ++j) bad += !(out[j].poly_obj() == want_g[j]);
  nfl::device_batch<P> src(1), dst(terms);
  src.upload(&x);
  std::vector<P> got(terms);
  dst.assign_decompose(src, w, NFLHIP_FORM_NTT | NFLHIP_DECOMP_SIGNED);
  dst.download(got.data());
  for (size_t j = 0; j < terms; ++j) bad += std::memcmp(got[j].cdata(), want_n[j].cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  dst.assign_gadget_mul(src, w);
  dst.download(got.data());
  for (size_t j = 0; j < terms; ++j) bad += std::memcmp(got[j].cdata(), want_g[j].cdata(), sizeof(uint64_t) * 64 * 3) != 0;
  return bad;
}
