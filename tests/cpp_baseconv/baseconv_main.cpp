// tests/cpp_baseconv/baseconv_main.cpp -- the RNS base conversion and the mod-down of the header surface (include/nfl_hip/nfl.hpp):
//   * nfl::base_convert / nfl::mod_down on nfl::poly (host-pointer path) and nfl::poly_p (resident; mod_down's input and output
//     are different ring types with deferred queues of their own: operations are pending on BOTH sides when the call is made,
//     and more are recorded on both after it; a copy-on-write sharer keeps its value across the in-place base_convert),
//   * device_batch::assign_base_convert / assign_mod_down and the same on a one-device sharded_batch,
// every result against a host restatement of the row formulas (include/nflhip.h "RNS base conversion") in 128-bit arithmetic,
// with the fixed-point correction exactly as defined there.  Second translation unit: baseconv_tu2.cpp.
// Usage: baseconv_test [eager].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception (no GPU: the library's
// "no CPU fallback" error).
#include <nfl.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int other_tu_baseconv();

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

typedef unsigned __int128 u128;
static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t p) { return uint64_t(u128(a) * b % p); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t p) {
  uint64_t r = 1 % p;
  for (a %= p; e; e >>= 1, a = mulmod(a, a, p))
    if (e & 1) r = mulmod(r, a, p);
  return r;
}
// (Q/p_i) mod p, Q the product of rows [s0, s0 + ks) (i == ks: Q itself)
template <class P> static uint64_t q_over(size_t s0, size_t ks, size_t i, uint64_t p) {
  uint64_t r = 1 % p;
  for (size_t t = 0; t < ks; ++t)
    if (t != i) r = mulmod(r, P::get_modulus(s0 + t) % p, p);
  return r;
}
// rows [d0, d0 + kd) of out = the conversion of rows [s0, s0 + ks) of in; the other rows of out are not touched
template <class P> static void host_convert(P &out, P const &in, size_t s0, size_t ks, size_t d0, size_t kd, bool centered) {
  typedef typename P::value_type T;
  const int W = 8 * int(sizeof(T));
  for (size_t c = 0; c < P::degree; ++c) {
    std::vector<uint64_t> y(ks);
    u128 F = 0;
    for (size_t i = 0; i < ks; ++i) {
      const uint64_t p = P::get_modulus(s0 + i);
      y[i] = mulmod(uint64_t(in(s0 + i, c)), powmod(q_over<P>(s0, ks, i, p), p - 2, p), p);
      F += W == 64 ? u128((u128(y[i]) * uint64_t((u128(1) << 124) / p)) >> 64) : u128(y[i]) * uint64_t((u128(1) << 60) / p);
    }
    const uint64_t v = uint64_t((F + (u128(1) << 59)) >> 60);
    for (size_t j = d0; j < d0 + kd; ++j) {
      const uint64_t p = P::get_modulus(j);
      uint64_t acc = 0;
      for (size_t i = 0; i < ks; ++i) acc = (acc + mulmod(y[i], q_over<P>(s0, ks, i, p), p)) % p;
      if (centered) acc = (acc + p - mulmod(v % p, q_over<P>(s0, ks, ks, p), p)) % p;
      out(j, c) = T(acc);
    }
  }
}
template <class PO, class PI> static void host_mod_down(PO &out, PI const &in, bool floor) {
  typedef typename PI::value_type T;
  const size_t K = PI::nmoduli - PO::nmoduli, kept = PO::nmoduli;
  PI conv(in);
  host_convert(conv, in, kept, K, 0, kept, !floor);
  for (size_t j = 0; j < kept; ++j) {
    const uint64_t p = PI::get_modulus(j), pinv = powmod(q_over<PI>(kept, K, K, p), p - 2, p);
    for (size_t c = 0; c < PI::degree; ++c) out(j, c) = T(mulmod((uint64_t(in(j, c)) + p - uint64_t(conv(j, c))) % p, pinv, p));
  }
}
template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }

template <class T, size_t D, size_t M, size_t K> static void run(const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  std::printf("%s\n", name);
  P a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
  S c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  const size_t s0 = M - K, ks = K;   // the mod-up from the last K rows to every row, and the conversion of the first rows to the rest
  {  // poly: both modes, both functions
    for (int centered = 0; centered < 2; ++centered) {
      P want(a), got(a);
      host_convert(want, a, s0, ks, 0, M, centered != 0);
      nfl::base_convert(got, s0, ks, 0, M, centered != 0);
      CHECK(same(got, want), "poly: base_convert to every row");
      P want2(a), got2(a);
      host_convert(want2, a, 0, M - K, M - K, K, centered != 0);
      nfl::base_convert(got2, 0, M - K, M - K, K, centered != 0);
      CHECK(same(got2, want2), "poly: base_convert prefix to suffix");
      S wd, gd;
      host_mod_down(wd, a, centered != 0);
      nfl::mod_down(gd, a, centered != 0);
      CHECK(same(gd, wd), "poly: mod_down");
    }
  }
  for (int round = 0; round < 3; ++round) {  // poly_p: deferred work pending on both sides, before and after
    P s = a + b, prod = s * b;
    S want_s, u = c + d, want_after, want_prod;
    host_mod_down(want_s, s, false);
    want_after = want_s * u;
    PP pa(a), pb(b);
    SP pc(c), pd(d);
    PP x = pa + pb;                  // pending on the input side
    SP y = pc + pd;                  // pending on the output side
    SP out = pc * pd;                // the old value of the output handle, pending too, shared with `keep`
    SP keep = out;
    nfl::mod_down(out, x);           // both queues run, then the mod-down
    SP z = out * y;                  // recorded after, on the output side: reads the result and the earlier pending sum
    PP w = x * pb;                   // recorded after, on the input side: the input is unchanged
    CHECK(same(out.poly_obj(), want_s), "poly_p: mod_down of a pending sum");
    CHECK(same(z.poly_obj(), want_after), "poly_p: a product recorded after the call sees the result");
    CHECK(same(w.poly_obj(), prod), "poly_p: the input side goes on with the unchanged input");
    S cd = c * d;
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of the output's old value keeps it");
    CHECK(same(y.poly_obj(), u), "poly_p: the output side's pending sum");
    host_mod_down(want_prod, prod, true);
    SP o2;
    nfl::mod_down(o2, w, true);
    CHECK(same(o2.poly_obj(), want_prod), "poly_p: floor mod_down of the product recorded after the first call");
    // in place: a pending sum converted, a sharer of the old value keeps it, work recorded after sees the new value
    PP v = pa + pb;
    PP sharer = v;
    nfl::base_convert(v, s0, ks, 0, M, round != 0);
    P want_v(s);
    host_convert(want_v, s, s0, ks, 0, M, round != 0);
    PP after = v + pb;
    P want_a = want_v + b;
    CHECK(same(v.poly_obj(), want_v), "poly_p: base_convert of a pending sum, in place");
    CHECK(same(sharer.poly_obj(), s), "poly_p: the copy-on-write sharer keeps its value across base_convert");
    CHECK(same(after.poly_obj(), want_a), "poly_p: a sum recorded after base_convert sees the converted value");
  }
  {  // device_batch and a one-device sharded_batch
    const size_t B = 5;
    std::vector<P> h(B), wu(B), want_u(B);
    std::vector<S> w(B), want(B);
    for (size_t i = 0; i < B; ++i) {
      h[i] = P(nfl::uniform(100 + i));
      host_mod_down(want[i], h[i], false);
      want_u[i] = h[i];
      host_convert(want_u[i], h[i], s0, ks, 0, M, true);
    }
    nfl::device_batch<P> src(B), up(B);
    nfl::device_batch<S> dst(B);
    src.upload(h.data());
    dst.assign_mod_down(src);
    dst.download(w.data());
    bool ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "device_batch: assign_mod_down");
    up.upload(h.data());
    up.assign_base_convert(up, s0, ks, 0, M, true);   // in place
    up.download(wu.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(wu[i], want_u[i]);
    CHECK(ok, "device_batch: assign_base_convert in place");
    up.upload(h.data());
    up.assign_base_convert(src, s0, ks, 0, M, true);  // from another batch
    up.download(wu.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(wu[i], want_u[i]);
    CHECK(ok, "device_batch: assign_base_convert from another batch");
    nfl::sharded_batch<P> ss(B, std::vector<int>{0});
    nfl::sharded_batch<S> sd(B, std::vector<int>{0});
    ss.upload(h.data());
    sd.assign_mod_down(ss);
    sd.download(w.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "sharded_batch: assign_mod_down");
    ss.assign_base_convert(ss, s0, ks, 0, M, true);
    ss.download(wu.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(wu[i], want_u[i]);
    CHECK(ok, "sharded_batch: assign_base_convert in place");
    bool threw = false;
    try {
      nfl::device_batch<S> small(B - 1);
      small.assign_mod_down(src);
    } catch (std::runtime_error const &) {
      threw = true;
    }
    CHECK(threw, "batches of different sizes throw std::runtime_error");
    threw = false;
    try {
      up.assign_base_convert(up, 0, M + 1, 0, 1);
    } catch (std::exception const &) {
      threw = true;
    }
    CHECK(threw, "a range outside the ring throws");
  }
}

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "eager") == 0) nfl::set_deferred(false);
    run<uint64_t, 1024, 2, 1>("u64/1024/2 k=1");
    run<uint64_t, 4096, 4, 2>("u64/4096/4 k=2");
    run<uint64_t, 64, 4, 3>("u64/64/4 k=3");
    run<uint32_t, 1024, 3, 1>("u32/1024/3 k=1");
    run<uint16_t, 128, 2, 1>("u16/128/2 k=1");
    run<uint64_t, 64, 40, 17>("u64/64/40 k=17");
    CHECK(other_tu_baseconv() == 0, "second translation unit");
    std::printf(g_fail ? "baseconv: FAILED (%d)\n" : "baseconv: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("baseconv: exception: %s\n", e.what());
    return 2;
  }
}
