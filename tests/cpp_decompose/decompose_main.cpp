// tests/cpp_decompose/decompose_main.cpp -- gadget decomposition on the header surface (include/nfl_hip/nfl.hpp):
//   * nfl::gadget_terms, nfl::decompose / nfl::decompose_ntt / nfl::gadget_mul on nfl::poly (the staged host entry) and on
//     nfl::poly_p (resident: deferred operations pending before the call and recorded after it, `out` elements shared
//     copy-on-write, `in` an element of `out`),
//   * device_batch::assign_decompose and device_batch::assign_gadget_mul,
//   * the end-to-end identity through nfl::dot:  invntt(sum_j decompose_ntt(x)[j] * ntt(gadget_mul(y))[j]) == x * y,
// every digit against a host restatement of the definition, step by step.  Second translation unit: decompose_tu2.cpp.
// Usage: decompose_test [eager].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception (no GPU: the library's "no CPU
// fallback" error).
#include <nfl.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int other_tu_decompose();

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

typedef __int128 i128;
// digit t of the canonical word x of a row with modulus p, by the definition
static i128 host_digit(uint64_t x, uint64_t p, int w, size_t l, size_t t, bool sgn) {
  const i128 B = i128(1) << w;
  if (!sgn) return (i128(x) >> (w * int(t))) & (B - 1);
  i128 r = x <= (p - 1) / 2 ? i128(x) : i128(x) - i128(p);
  for (size_t k = 0; k + 1 < l; ++k) {
    const i128 d = ((((r + B / 2) % B) + B) % B) - B / 2;
    if (k == t) return d;
    r = (r - d) / B;
  }
  return r;
}
template <class P> static void host_decompose(std::vector<P> &out, P const &in, int w, bool sgn) {
  typedef typename P::value_type T;
  const size_t l = nfl::gadget_terms<P>(w) / P::nmoduli;
  for (size_t m = 0; m < P::nmoduli; ++m)
    for (size_t t = 0; t < l; ++t)
      for (size_t i = 0; i < P::degree; ++i) {
        const i128 d = host_digit(uint64_t(in(m, i)), P::get_modulus(m), w, l, t, sgn);
        for (size_t r = 0; r < P::nmoduli; ++r) out[m * l + t](r, i) = T(uint64_t(d < 0 ? i128(P::get_modulus(r)) + d : d));
      }
}
template <class P> static void host_gadget_mul(std::vector<P> &out, P const &in, int w) {
  typedef typename P::value_type T;
  const size_t l = nfl::gadget_terms<P>(w) / P::nmoduli;
  for (size_t m = 0; m < P::nmoduli; ++m)
    for (size_t t = 0; t < l; ++t)
      for (size_t i = 0; i < P::degree; ++i)
        for (size_t r = 0; r < P::nmoduli; ++r)
          out[m * l + t](r, i) = r == m ? T(uint64_t(((unsigned __int128)(uint64_t(in(m, i))) << (w * int(t))) % P::get_modulus(m))) : T(0);
}
template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }
template <class P> static bool same_all(std::vector<P> const &a, std::vector<P> const &b) {
  bool ok = a.size() == b.size();
  for (size_t j = 0; ok && j < a.size(); ++j) ok = same(a[j], b[j]);
  return ok;
}

template <class T, size_t D, size_t M> static void run(const char *name, int w) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly_p<T, D, M> PP;
  const size_t terms = nfl::gadget_terms<P>(w);
  std::printf("%s, w = %d, %u terms\n", name, w, unsigned(terms));
  CHECK(terms == M * ((8 * sizeof(T) - 2 + w - 1) / w), "gadget_terms");
  CHECK(nfl::gadget_terms<P>(0) == 0 && nfl::gadget_terms<P>(int(8 * sizeof(T)) - 2) == 0, "gadget_terms refuses an invalid width");
  P x(nfl::uniform(0x51)), y(nfl::uniform(0x52)), c(nfl::uniform(0x53));
  for (size_t m = 0; m < M; ++m) {  // edge words in front
    const T p = T(P::get_modulus(m));
    const T e[5] = {T(0), T(1), T((p - 1) / 2), T((p + 1) / 2), T(p - 1)};
    for (size_t i = 0; i < 5 && i < D; ++i) x(m, i) = e[i];
  }
  std::vector<P> want_u(terms), want_s(terms), want_g(terms), got(terms);
  host_decompose(want_u, x, w, false);
  host_decompose(want_s, x, w, true);
  host_gadget_mul(want_g, y, w);
  P xy = x;  // x * y in coefficient form
  {
    P a = x, b = y;
    a.ntt_pow_phi();
    b.ntt_pow_phi();
    xy = a * b;
    xy.invntt_pow_invphi();
  }
  {  // poly
    nfl::decompose(got.data(), x, w);
    CHECK(same_all(got, want_u), "poly: decompose");
    nfl::decompose(got.data(), x, w, true);
    CHECK(same_all(got, want_s), "poly: decompose, signed");
    nfl::gadget_mul(got.data(), y, w);
    CHECK(same_all(got, want_g), "poly: gadget_mul");
    std::vector<P> dn(terms), gn(got);
    nfl::decompose_ntt(dn.data(), x, w, true);
    std::vector<P> want_n(want_s);
    for (size_t j = 0; j < terms; ++j) want_n[j].ntt_pow_phi();
    CHECK(same_all(dn, want_n), "poly: decompose_ntt equals ntt_pow_phi of decompose");
    for (size_t j = 0; j < terms; ++j) gn[j].ntt_pow_phi();
    P z;
    nfl::dot(z, dn.data(), gn.data(), terms);
    z.invntt_pow_invphi();
    CHECK(same(z, xy), "poly: invntt(dot(decompose_ntt(x), ntt(gadget_mul(y)))) == x * y");
    got[1] = x;
    nfl::decompose(got.data(), got[1], w);
    CHECK(same_all(got, want_u), "poly: the input is an element of the output");
    bool threw = false;
    try {
      nfl::decompose(got.data(), x, 0);
    } catch (std::runtime_error const &) {
      threw = true;
    }
    CHECK(threw, "an invalid width throws std::runtime_error");
  }
  for (int round = 0; round < 2; ++round) {  // poly_p: deferred work pending before, more recorded after
    PP px(x), py(y), pc(c);
    P xc = x + c;
    std::vector<P> want_xc(terms);
    host_decompose(want_xc, xc, w, round == 1);
    PP in = px + pc;                         // pending: the input is a deferred sum
    std::vector<PP> out(terms);
    out[0] = pc * py;                        // the old value of an output handle, pending too, shared with `keep`
    PP keep = out[0];
    nfl::decompose(out.data(), in, w, round == 1);   // the queue runs, then the launch
    PP after = out[terms - 1] + pc;          // recorded after: reads a result
    bool ok = true;
    for (size_t j = 0; j < terms; ++j) ok &= same(out[j].poly_obj(), want_xc[j]);
    CHECK(ok, "poly_p: decompose of a pending sum");
    P want_after = want_xc[terms - 1] + c;
    CHECK(same(after.poly_obj(), want_after), "poly_p: a sum recorded after the call sees the result");
    P cy = c * y;
    CHECK(same(keep.poly_obj(), cy), "poly_p: the sharer of an output's old value keeps it");
    std::vector<PP> share(out);              // copy-on-write sharers of the outputs
    out[0] = px;
    nfl::decompose(out.data(), out[0], w);   // the input is an element of the output
    ok = true;
    for (size_t j = 0; j < terms; ++j) ok &= same(out[j].poly_obj(), want_u[j]) && same(share[j].poly_obj(), want_xc[j]);
    CHECK(ok, "poly_p: the input is an element of the output; sharers keep the earlier digits");
    std::vector<PP> dn(terms), gn(terms);
    nfl::decompose_ntt(dn.data(), px, w, round == 1);
    nfl::gadget_mul(gn.data(), py, w);
    ok = true;
    for (size_t j = 0; j < terms; ++j) ok &= same(gn[j].poly_obj(), want_g[j]);
    CHECK(ok, "poly_p: gadget_mul");
    for (size_t j = 0; j < terms; ++j) gn[j].ntt_pow_phi();
    PP z;
    nfl::dot(z, dn.data(), gn.data(), terms);
    z.invntt_pow_invphi();
    CHECK(same(z.poly_obj(), xy), "poly_p: invntt(dot(decompose_ntt(x), ntt(gadget_mul(y)))) == x * y");
  }
  {  // device_batch
    const size_t G = 3;
    std::vector<P> hx(G), w_all(G * terms), got_all(G * terms), one(terms);
    for (size_t b = 0; b < G; ++b) {
      hx[b] = b == 0 ? x : P(nfl::uniform(0x300 + b));
      host_decompose(one, hx[b], w, true);
      for (size_t j = 0; j < terms; ++j) w_all[b * terms + j] = one[j];
    }
    nfl::device_batch<P> src(G), dst(G * terms);
    src.upload(hx.data());
    dst.assign_decompose(src, w, NFLHIP_FORM_COEFF | NFLHIP_DECOMP_SIGNED);
    dst.download(got_all.data());
    CHECK(same_all(got_all, w_all), "device_batch: assign_decompose, signed");
    nfl::device_batch<P> dn(G * terms);
    dn.assign_decompose(src, w, NFLHIP_FORM_NTT | NFLHIP_DECOMP_SIGNED);
    dst.ntt_pow_phi();
    std::vector<P> a(G * terms);
    dn.download(a.data());
    dst.download(got_all.data());
    CHECK(same_all(a, got_all), "device_batch: the NTT form equals ntt_pow_phi of the coefficient form");
    for (size_t b = 0; b < G; ++b) {
      host_gadget_mul(one, hx[b], w);
      for (size_t j = 0; j < terms; ++j) w_all[b * terms + j] = one[j];
    }
    dst.assign_gadget_mul(src, w);
    dst.download(got_all.data());
    CHECK(same_all(got_all, w_all), "device_batch: assign_gadget_mul");
    bool threw = false;
    try {
      nfl::device_batch<P> small(G * terms - 1);
      small.assign_decompose(src, w);
    } catch (std::runtime_error const &) {
      threw = true;
    }
    CHECK(threw, "an output of the wrong size throws std::runtime_error");
  }
}

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "eager") == 0) nfl::set_deferred(false);
    run<uint64_t, 1024, 2>("u64/1024/2", 20);
    run<uint64_t, 4096, 4>("u64/4096/4", 31);
    run<uint32_t, 1024, 3>("u32/1024/3", 15);
    run<uint16_t, 128, 2>("u16/128/2", 7);
    run<uint64_t, 64, 94>("u64/64/94", 61);
    CHECK(other_tu_decompose() == 0, "second translation unit");
    std::printf(g_fail ? "decompose: FAILED (%d)\n" : "decompose: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("decompose: exception: %s\n", e.what());
    return 2;
  }
}
