// tests/cpp_rescale/rescale_main.cpp -- the RNS rescale of the header surface (include/nfl_hip/nfl.hpp):
//   * nfl::rescale / nfl::rescale_ntt on nfl::poly (host-pointer path) and nfl::poly_p (resident; the input and the output
//     are different ring types with deferred queues of their own: operations are pending on BOTH sides when the call is made,
//     and more are recorded on both after it),
//   * device_batch::assign_rescale and the same on a one-device sharded_batch,
// every result against a host restatement of the row formula (include/nflhip.h "RNS rescale").  The NTT form is checked
// through the transforms of the smaller ring: invntt(rescale_ntt(ntt(a))) == rescale(a).  Second translation unit:
// rescale_tu2.cpp.  Usage: rescale_test [eager].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception (no GPU: the
// library's "no CPU fallback" error).
#include <nfl.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int other_tu_rescale();

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

typedef unsigned __int128 u128;
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t p) {
  uint64_t r = 1 % p;
  for (a %= p; e; e >>= 1, a = uint64_t(u128(a) * a % p))
    if (e & 1) r = uint64_t(u128(r) * a % p);
  return r;
}
// r = (x_L + h) mod q, y_i = (x_i + h - r) q^-1 mod p_i
template <class PO, class PI> static void host_rescale(PO &out, PI const &in) {
  typedef typename PI::value_type T;
  const size_t L = PI::nmoduli - 1;
  const uint64_t q = PI::get_modulus(L), h = (q - 1) / 2;
  for (size_t cm = 0; cm < L; ++cm) {
    const uint64_t p = PI::get_modulus(cm), qinv = powmod(q, p - 2, p);
    for (size_t i = 0; i < PI::degree; ++i) {
      const uint64_t r = (uint64_t(in(L, i)) + h) % q;
      const uint64_t t = (uint64_t(in(cm, i)) + h + 2 * p - r) % p;
      out(cm, i) = T(u128(t) * qinv % p);
    }
  }
}
template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }

template <class T, size_t D, size_t M> static void run(const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - 1> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - 1> SP;
  std::printf("%s\n", name);
  P a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
  S c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  {  // poly: both forms
    S want, got;
    host_rescale(want, a);
    nfl::rescale(got, a);
    CHECK(same(got, want), "poly: rescale");
    P an(a);
    an.ntt_pow_phi();
    S gn;
    nfl::rescale_ntt(gn, an);
    gn.invntt_pow_invphi();
    CHECK(same(gn, want), "poly: invntt(rescale_ntt(ntt(a))) == rescale(a)");
  }
  for (int round = 0; round < 3; ++round) {  // poly_p: deferred work pending on both sides, before and after
    P s = a + b, prod = s * b;
    S want_s, u = c + d, want_after, want_prod;
    host_rescale(want_s, s);
    want_after = want_s * u;
    PP pa(a), pb(b);
    SP pc(c), pd(d);
    PP x = pa + pb;                  // pending on the input side
    SP y = pc + pd;                  // pending on the output side
    SP out = pc * pd;                // the old value of the output handle, pending too, shared with `keep`
    SP keep = out;
    nfl::rescale(out, x);            // both queues run, then the rescale
    SP z = out * y;                  // recorded after, on the output side: reads the result and the earlier pending sum
    PP w = x * pb;                   // recorded after, on the input side: the input is unchanged
    CHECK(same(out.poly_obj(), want_s), "poly_p: rescale of a pending sum");
    CHECK(same(z.poly_obj(), want_after), "poly_p: a product recorded after the call sees the result");
    CHECK(same(w.poly_obj(), prod), "poly_p: the input side goes on with the unchanged input");
    S cd = c * d;
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of the output's old value keeps it");
    CHECK(same(y.poly_obj(), u), "poly_p: the output side's pending sum");
    PP xn = pa + pb;
    xn.ntt_pow_phi();                // pending transform on the input side
    SP yn;
    nfl::rescale_ntt(yn, xn);
    yn.invntt_pow_invphi();          // recorded after, on the output side
    CHECK(same(yn.poly_obj(), want_s), "poly_p: rescale_ntt between pending transforms");
    host_rescale(want_prod, prod);
    SP o2;
    nfl::rescale(o2, w);
    CHECK(same(o2.poly_obj(), want_prod), "poly_p: rescale of the product recorded after the first call");
  }
  {  // device_batch and a one-device sharded_batch
    const size_t B = 5;
    std::vector<P> h(B);
    std::vector<S> w(B), want(B);
    for (size_t i = 0; i < B; ++i) {
      h[i] = P(nfl::uniform(100 + i));
      host_rescale(want[i], h[i]);
    }
    nfl::device_batch<P> src(B);
    nfl::device_batch<S> dst(B);
    src.upload(h.data());
    dst.assign_rescale(src);
    dst.download(w.data());
    bool ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "device_batch: assign_rescale");
    src.ntt_pow_phi();               // enqueued on the source's stream before the call
    dst.assign_rescale(src, true);
    dst.invntt_pow_invphi();         // enqueued on the destination's stream after it
    dst.download(w.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "device_batch: assign_rescale in NTT form between transforms on both streams");
    nfl::sharded_batch<P> ss(B, std::vector<int>{0});
    nfl::sharded_batch<S> sd(B, std::vector<int>{0});
    ss.upload(h.data());
    sd.assign_rescale(ss);
    sd.download(w.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "sharded_batch: assign_rescale");
    ss.ntt_pow_phi();
    sd.assign_rescale(ss, true);
    sd.invntt_pow_invphi();
    sd.download(w.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
    CHECK(ok, "sharded_batch: assign_rescale in NTT form");
    bool threw = false;
    try {
      nfl::device_batch<S> small(B - 1);
      small.assign_rescale(src);
    } catch (std::runtime_error const &) {
      threw = true;
    }
    CHECK(threw, "batches of different sizes throw std::runtime_error");
  }
}

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "eager") == 0) nfl::set_deferred(false);
    run<uint64_t, 1024, 2>("u64/1024/2");
    run<uint64_t, 4096, 4>("u64/4096/4");
    run<uint64_t, 16384, 3>("u64/16384/3");
    run<uint32_t, 1024, 3>("u32/1024/3");
    run<uint16_t, 128, 2>("u16/128/2");
    run<uint64_t, 64, 94>("u64/64/94");
    CHECK(other_tu_rescale() == 0, "second translation unit");
    std::printf(g_fail ? "rescale: FAILED (%d)\n" : "rescale: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("rescale: exception: %s\n", e.what());
    return 2;
  }
}
