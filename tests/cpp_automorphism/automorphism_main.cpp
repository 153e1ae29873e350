// tests/cpp_automorphism/automorphism_main.cpp -- the Galois automorphisms of the header surface (include/nfl_hip/nfl.hpp):
//   * nfl::automorphism / nfl::automorphism_ntt on nfl::poly (host-pointer path) and nfl::poly_p (resident, with deferred
//     operations recorded before and after, out == in, and a copy-on-write sharer that must keep the old value),
//   * device_batch::assign_automorphism / assign_automorphisms and the same on a sharded_batch,
// every result against a host restatement of the coefficient-form map (include/nflhip.h).  The NTT form is checked
// through the transforms: invntt(sigma_ntt(ntt(a))) == sigma_coeff(a).  Second translation unit: automorphism_tu2.cpp.
// Usage: automorphism_test [eager].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception (no GPU: the library's
// "no CPU fallback" error).
#include <nfl.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int other_tu_automorphism();

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

// sigma_k in coefficient form: coefficient i goes to i k mod 2n, negated mod p when that is n or above
template <class P> static void host_sigma(P &out, P const &in, uint64_t k) {
  typedef typename P::value_type T;
  const size_t n = P::degree;
  for (size_t cm = 0; cm < P::nmoduli; ++cm) {
    const T p = P::get_modulus(cm);
    for (size_t i = 0; i < n; ++i) {
      const size_t e = size_t((uint64_t(i) * (k % (2 * n))) % (2 * n));
      const T x = in(cm, i);
      if (e < n) out(cm, e) = x;
      else out(cm, e - n) = x ? T(p - x) : T(0);
    }
  }
}
template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }

template <class T, size_t D, size_t M> static void run(const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly_p<T, D, M> PP;
  const uint64_t ks[] = {1, 3, 5, 2 * D - 1, 2 * D + 7, 0x12345 | 1};
  std::printf("%s\n", name);
  P a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
  for (uint64_t k : ks) {
    // poly, coefficient form, separate output and in place
    P want, got;
    host_sigma(want, a, k);
    nfl::automorphism(got, a, k);
    CHECK(same(got, want), "poly: automorphism");
    P inplace(a);
    nfl::automorphism(inplace, inplace, k);
    CHECK(same(inplace, want), "poly: automorphism in place");
    // poly, NTT form
    P an(a), gn;
    an.ntt_pow_phi();
    nfl::automorphism_ntt(gn, an, k);
    gn.invntt_pow_invphi();
    CHECK(same(gn, want), "poly: invntt(automorphism_ntt(ntt(a))) == automorphism(a)");
    nfl::automorphism_ntt(an, an, k);
    an.invntt_pow_invphi();
    CHECK(same(an, want), "poly: automorphism_ntt in place");
  }
  // poly_p: deferred operations before and after, out == in, a copy-on-write sharer
  for (uint64_t k : ks) {
    P s = a + b, want_s, want_t, t_host;
    host_sigma(want_s, s, k);
    t_host = want_s * b;
    host_sigma(want_t, t_host, k);
    PP pa(a), pb(b);
    PP x = pa + pb;                   // deferred
    PP y;
    nfl::automorphism(y, x, k);       // runs the queue, then sigma
    PP z = y * pb;                    // deferred again, reads the automorphism's result
    CHECK(same(y.poly_obj(), want_s), "poly_p: automorphism after a deferred sum");
    CHECK(same(z.poly_obj(), t_host), "poly_p: a deferred product of the result");
    PP keep = z;                      // shares z's payload
    nfl::automorphism(z, z, k);       // out == in: z gets a fresh payload, keep is unchanged
    CHECK(same(z.poly_obj(), want_t), "poly_p: automorphism in place");
    CHECK(same(keep.poly_obj(), t_host), "poly_p: the copy-on-write sharer keeps the old value");
    PP xn = pa + pb;
    xn.ntt_pow_phi();                 // deferred transform
    PP yn;
    nfl::automorphism_ntt(yn, xn, k);
    yn.invntt_pow_invphi();
    CHECK(same(yn.poly_obj(), want_s), "poly_p: automorphism_ntt between deferred transforms");
  }
  // device_batch: single and multi, both forms
  {
    const size_t B = 5;
    std::vector<P> h(B), w(B);
    for (size_t i = 0; i < B; ++i) h[i] = P(nfl::uniform(100 + i));
    nfl::device_batch<P> src(B), dst(B), o0(B), o1(B), o2(B);
    src.upload(h.data());
    for (uint64_t k : ks) {
      std::vector<P> want(B);
      for (size_t i = 0; i < B; ++i) host_sigma(want[i], h[i], k);
      dst.assign_automorphism(src, k);
      dst.download(w.data());
      bool ok = true;
      for (size_t i = 0; i < B; ++i) ok &= same(w[i], want[i]);
      CHECK(ok, "device_batch: assign_automorphism");
    }
    nfl::device_batch<P> *outs[3] = {&o0, &o1, &o2};
    const uint64_t mk[3] = {3, 5, 2 * D - 1};
    nfl::device_batch<P>::assign_automorphisms(outs, mk, 3, src);
    for (int m = 0; m < 3; ++m) {
      outs[m]->download(w.data());
      bool ok = true;
      for (size_t i = 0; i < B; ++i) {
        P want;
        host_sigma(want, h[i], mk[m]);
        ok &= same(w[i], want);
      }
      CHECK(ok, "device_batch: assign_automorphisms");
    }
    // NTT form through the batch transforms
    nfl::device_batch<P> sn(B);
    sn.upload(h.data());
    sn.ntt_pow_phi();
    nfl::device_batch<P>::assign_automorphisms(outs, mk, 3, sn, true);
    for (int m = 0; m < 3; ++m) {
      outs[m]->invntt_pow_invphi();
      outs[m]->download(w.data());
      bool ok = true;
      for (size_t i = 0; i < B; ++i) {
        P want;
        host_sigma(want, h[i], mk[m]);
        ok &= same(w[i], want);
      }
      CHECK(ok, "device_batch: assign_automorphisms in NTT form");
    }
    dst.assign_automorphism(sn, 7, true);
    dst.invntt_pow_invphi();
    dst.download(w.data());
    bool ok = true;
    for (size_t i = 0; i < B; ++i) {
      P want;
      host_sigma(want, h[i], 7);
      ok &= same(w[i], want);
    }
    CHECK(ok, "device_batch: assign_automorphism in NTT form");
    // a one-device sharded_batch, shard by shard
    nfl::sharded_batch<P> ss(B, std::vector<int>{0}), sd(B, std::vector<int>{0}), s1(B, std::vector<int>{0});
    ss.upload(h.data());
    sd.assign_automorphism(ss, 5);
    sd.download(w.data());
    ok = true;
    for (size_t i = 0; i < B; ++i) {
      P want;
      host_sigma(want, h[i], 5);
      ok &= same(w[i], want);
    }
    CHECK(ok, "sharded_batch: assign_automorphism");
    nfl::sharded_batch<P> *souts[2] = {&sd, &s1};
    const uint64_t sk[2] = {3, 2 * D - 1};
    nfl::sharded_batch<P>::assign_automorphisms(souts, sk, 2, ss);
    for (int m = 0; m < 2; ++m) {
      souts[m]->download(w.data());
      ok = true;
      for (size_t i = 0; i < B; ++i) {
        P want;
        host_sigma(want, h[i], sk[m]);
        ok &= same(w[i], want);
      }
      CHECK(ok, "sharded_batch: assign_automorphisms");
    }
  }
  // an even k is refused with the reference's exception type
  bool threw = false;
  try {
    P o;
    nfl::automorphism(o, a, 2);
  } catch (std::runtime_error const &) {
    threw = true;
  }
  CHECK(threw, "an even k throws std::runtime_error");
}

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "eager") == 0) nfl::set_deferred(false);
    run<uint64_t, 1024, 2>("u64/1024/2");
    run<uint64_t, 4096, 4>("u64/4096/4");
    run<uint32_t, 1024, 2>("u32/1024/2");
    run<uint16_t, 128, 1>("u16/128/1");
    run<uint64_t, 64, 94>("u64/64/94");
    CHECK(other_tu_automorphism() == 0, "second translation unit");
    std::printf(g_fail ? "automorphism: FAILED (%d)\n" : "automorphism: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("automorphism: exception: %s\n", e.what());
    return 2;
  }
}
