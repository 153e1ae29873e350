// tests/cpp_level/level_main.cpp -- key switching and multiplication below the top level on the header surface
// (include/nfl_hip/poly_p.hpp, batch.hpp; include/nflhip.h "leveled key switching"):
//   * nfl::key_switch_level_ntt<K>, mul_relin_level_ntt<K>, square_relin_level_ntt<K> and mul_relin_rescale_level_ntt<K> on nfl::poly (the
//     staged host entries) equal the C entries called on raw pointers (buffers of nflhip_malloc) with K, the level and the WHOLE
//     top-level key written out by hand;
//   * at the top level, Lv = M - K, they equal the existing nfl::key_switch_ntt / mul_relin_ntt / mul_relin_rescale_ntt;
//   * the same on nfl::poly_p (resident: deferred work pending on an input, on a key polynomial and on the output's old value; a
//     copy-on-write sharer keeps the old value; an output may be an input; work recorded after sees the result) -- only the live key
//     polynomials are gathered: the dead ones of the array are moved from, and touching one would throw;
//   * device_batch::assign_key_switch_level<K> / assign_mul_relin_level<K>: every polynomial equal to the poly path's.
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_level.c and of the tests it builds on (tests/test_level_cpp.py).
// Usage: level_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }
template <class P> static bool same(std::vector<P> const &a, std::vector<P> const &b) {
  bool ok = a.size() == b.size();
  for (size_t i = 0; ok && i < a.size(); ++i) ok = same(a[i], b[i]);
  return ok;
}
template <class P, class B> static std::vector<P> polys(const B &b) {
  std::vector<P> h(b.size());
  if (b.size()) b.download(h.data());
  return h;
}

// the C entries on raw pointers: B polynomials per operand, the whole key; rows_out = Lv, or Lv - 1 with the rescale
template <class S, class O, class P, class KB>
static bool raw(const KB &kbatch, std::vector<O> &g0, std::vector<O> &g1, const std::vector<S> *const h[4], int nin, const std::vector<P> &key, size_t K,
                size_t alpha, int flags, bool mul) {
  nflhip_ctx *ctx = kbatch.ctx();
  const size_t B = h[0]->size(), ib = B * sizeof(S), ob = B * sizeof(O), kbytes = key.size() * sizeof(P);
  void *q0 = nullptr, *q1 = nullptr, *ri[4] = {nullptr, nullptr, nullptr, nullptr}, *rk = nullptr;
  bool ok = nflhip_malloc(ctx, &q0, ob) == 0 && nflhip_malloc(ctx, &q1, ob) == 0 && nflhip_malloc(ctx, &rk, kbytes) == 0;
  for (int k = 0; k < nin; ++k) ok = ok && nflhip_malloc(ctx, &ri[k], ib) == 0 && nflhip_memcpy_h2d(ctx, ri[k], (*h[k])[0].cdata(), ib, kbatch.queue()) == 0;
  ok = ok && nflhip_memcpy_h2d(ctx, rk, key[0].cdata(), kbytes, kbatch.queue()) == 0;
  if (mul) ok = ok && nflhip_mulrelin_level_ntt_dev(ctx, q0, q1, ri[0], ri[1], ri[2], ri[3], rk, B, K, alpha, S::nmoduli, flags, kbatch.queue()) == 0;
  else ok = ok && nflhip_keyswitch_level_ntt_dev(ctx, q0, q1, ri[0], rk, B, K, alpha, S::nmoduli, flags, kbatch.queue()) == 0;
  g0.resize(B), g1.resize(B);
  ok = ok && nflhip_memcpy_d2h(ctx, g0[0].data(), q0, ob, kbatch.queue()) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), q1, ob, kbatch.queue()) == 0;
  ok = ok && nflhip_stream_sync(ctx, kbatch.queue()) == 0;
  nflhip_free(ctx, q0), nflhip_free(ctx, q1), nflhip_free(ctx, rk);
  for (int k = 0; k < nin; ++k) nflhip_free(ctx, ri[k]);
  return ok;
}

template <bool TOP> struct top_level {  // below the top level: nothing to compare with
  template <class S, class P> static void check(std::vector<S> const *const *, std::vector<P> const &, size_t, std::vector<S> const &, std::vector<S> const &,
                                                std::vector<S> const &, std::vector<S> const &) {}
};
template <> struct top_level<true> {
  template <class S, class P> static void check(std::vector<S> const *const *h, std::vector<P> const &key, size_t alpha, std::vector<S> const &k0,
                                                std::vector<S> const &k1, std::vector<S> const &m0, std::vector<S> const &m1) {
    for (size_t i = 0; i < k0.size(); ++i) {
      S x0, x1;
      nfl::key_switch_ntt(x0, x1, (*h[1])[i], key.data(), alpha, true, false);
      CHECK(same(x0, k0[i]) && same(x1, k1[i]), "at the top level key_switch_level_ntt<K> is key_switch_ntt");
      nfl::mul_relin_ntt(x0, x1, (*h[0])[i], (*h[1])[i], (*h[2])[i], (*h[3])[i], key.data(), alpha, true, false);
      CHECK(same(x0, m0[i]) && same(x1, m1[i]), "at the top level mul_relin_level_ntt<K> is mul_relin_ntt");
    }
  }
};

template <class T, size_t D, size_t M, size_t K, size_t Lv> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, Lv> S;
  typedef nfl::poly<T, D, Lv - 1> R;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, Lv> SP;
  typedef nfl::poly_p<T, D, Lv - 1> RP;
  const size_t dnum = (M - K + alpha - 1) / alpha, live = (Lv + alpha - 1) / alpha;
  std::printf("%s level %zu alpha=%zu, %zu digits of %zu live, %zu polynomials\n", name, Lv, alpha, live, dnum, B);
  std::vector<P> key, ka, kb;
  for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial a sum, so that poly_p can hold it pending
    ka.push_back(P(nfl::uniform(0x100 + t)));
    kb.push_back(P(nfl::uniform(0x200 + t)));
    key.push_back(ka[t] + kb[t]);
  }
  std::vector<S> h[4];
  for (int k = 0; k < 4; ++k) {
    h[k].resize(B);
    for (size_t i = 0; i < B; ++i) h[k][i] = S(nfl::uniform(100 + 10 * i + k));
  }
  const std::vector<S> *const hp[4] = {&h[0], &h[1], &h[2], &h[3]}, *const h1[4] = {&h[1], nullptr, nullptr, nullptr};
  nfl::device_batch<P> kbatch(2 * dnum, 0);
  kbatch.upload(key.data());
  // the poly path against the C entries on raw pointers, K, the level and the whole key written out by hand
  std::vector<S> k0(B), k1(B), m0(B), m1(B), q0(B), q1(B), g0, g1;
  std::vector<R> r0(B), r1(B), gr0, gr1;
  for (size_t i = 0; i < B; ++i) {
    nfl::key_switch_level_ntt<K>(k0[i], k1[i], h[1][i], key.data(), alpha, true, false);
    nfl::mul_relin_level_ntt<K>(m0[i], m1[i], h[0][i], h[1][i], h[2][i], h[3][i], key.data(), alpha, true, false);
    nfl::square_relin_level_ntt<K>(q0[i], q1[i], h[0][i], h[1][i], key.data(), alpha, true, false);
    nfl::mul_relin_rescale_level_ntt<K>(r0[i], r1[i], h[0][i], h[1][i], h[2][i], h[3][i], key.data(), alpha, true, false);
  }
  { const bool ok = raw<S, S>(kbatch, g0, g1, h1, 1, key, K, alpha, NFLHIP_KEYSWITCH_CENTERED, false); CHECK(ok, "raw pointers: the key switch succeeds"); }
  CHECK(same(g0, k0) && same(g1, k1), "poly: key_switch_level_ntt<K> equals the C entry with K and the level written out");
  CHECK(!same(k0[0], k1[0]), "poly: the two components differ");
  { const bool ok = raw<S, S>(kbatch, g0, g1, hp, 4, key, K, alpha, NFLHIP_MULRELIN_CENTERED, true); CHECK(ok, "raw pointers: the multiplication succeeds"); }
  CHECK(same(g0, m0) && same(g1, m1), "poly: mul_relin_level_ntt<K> equals the C entry");
  { const bool ok = raw<S, S>(kbatch, g0, g1, hp, 2, key, K, alpha, NFLHIP_MULRELIN_CENTERED, true); CHECK(ok, "raw pointers: the square succeeds"); }
  CHECK(same(g0, q0) && same(g1, q1) && !same(q0, m0), "poly: square_relin_level_ntt<K> equals the C entry");
  { const bool ok = raw<S, R>(kbatch, gr0, gr1, hp, 4, key, K, alpha, NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_RESCALE, true); CHECK(ok, "raw pointers: the rescale succeeds"); }
  CHECK(same(gr0, r0) && same(gr1, r1) && !same(r0, r1), "poly: mul_relin_rescale_level_ntt<K> equals the C entry");
  top_level<Lv == M - K>::check(hp, key, alpha, k0, k1, m0, m1);
  {  // the modes reach the entry
    S x0, x1;
    nfl::key_switch_level_ntt<K>(x0, x1, h[1][0], key.data(), alpha, false, true);
    const bool ok = raw<S, S>(kbatch, g0, g1, h1, 1, key, K, alpha, NFLHIP_KEYSWITCH_FLOOR, false);
    CHECK(ok && same(x0, g0[0]) && same(x1, g1[0]), "poly: fast mode, floor");
    S y(h[1][0]);
    nfl::key_switch_level_ntt<K>(y, x1, y, key.data(), alpha, true, false);
    CHECK(same(y, k0[0]) && same(x1, k1[0]), "poly: an output may be the input");
  }
  {  // poly_p: an input, a key polynomial and the output's old value pending; sharers keep their values
    S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de));
    S a0 = a + b;
    const S ab = a * b;
    S w0, w1, v0, v1;
    nfl::key_switch_level_ntt<K>(w0, w1, a0, key.data(), alpha, true, false);
    nfl::mul_relin_level_ntt<K>(v0, v1, a0, c, h[2][0], h[3][0], key.data(), alpha, true, false);
    R u0, u1;
    nfl::mul_relin_rescale_level_ntt<K>(u0, u1, a0, c, h[2][0], h[3][0], key.data(), alpha, true, false);
    PP pka(ka[1]), pkb(kb[1]);
    std::vector<PP> pkey;
    for (size_t t = 0; t < 2 * dnum; ++t) pkey.push_back(PP(key[t]));
    pkey[1] = pka + pkb;
    // the DEAD key polynomials, those of the digits >= dnum_l, are moved from: a call that touched one would be refused (an empty
    // polynomial) -- only the 2 dnum_l live ones are gathered
    std::vector<PP> graveyard;
    for (size_t t = 2 * live; t < 2 * dnum; ++t) graveyard.push_back(std::move(pkey[t]));
    SP pa(a), pb(b), pc(c), pd(h[2][0]), pe(h[3][0]);
    SP pa0 = pa + pb;
    SP out0 = pa * pb, out1 = pa + pb;
    SP keep = out0;
    nfl::key_switch_level_ntt<K>(out0, out1, pa0, pkey.data(), alpha, true, false);
    SP z = out0 + pc;
    const S want_z = w0 + c;
    CHECK(same(out0.poly_obj(), w0) && same(out1.poly_obj(), w1), "poly_p: key_switch_level_ntt<K> of a pending input with a pending key polynomial");
    CHECK(same(keep.poly_obj(), ab) && same(pa0.poly_obj(), a0) && same(pkey[1].poly_obj(), key[1]), "poly_p: the sharer keeps the old value; input and key stay");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after the call sees the result");
    SP sharer = pa0;
    nfl::key_switch_level_ntt<K>(pa0, out1, pa0, pkey.data(), alpha, true, false);
    CHECK(same(pa0.poly_obj(), w0) && same(out1.poly_obj(), w1) && same(sharer.poly_obj(), a0), "poly_p: out0 may be the input; its sharer keeps the input");
    SP pa1 = pa + pb, o0, o1;
    nfl::mul_relin_level_ntt<K>(o0, o1, pa1, pc, pd, pe, pkey.data(), alpha, true, false);
    CHECK(same(o0.poly_obj(), v0) && same(o1.poly_obj(), v1), "poly_p: mul_relin_level_ntt<K> equals the poly path");
    RP pr0, pr1;
    nfl::mul_relin_rescale_level_ntt<K>(pr0, pr1, pa1, pc, pd, pe, pkey.data(), alpha, true, false);
    CHECK(same(pr0.poly_obj(), u0) && same(pr1.poly_obj(), u1), "poly_p: mul_relin_rescale_level_ntt<K> equals the poly path");
    SP s0, s1, p0(h[0][0]), p1(h[1][0]);
    nfl::square_relin_level_ntt<K>(s0, s1, p0, p1, pkey.data(), alpha, true, false);
    CHECK(same(s0.poly_obj(), q0[0]) && same(s1.poly_obj(), q1[0]), "poly_p: square_relin_level_ntt<K> equals the poly path");
  }
  // device_batch against the poly path
  nfl::device_batch<S> s0(B, 0), s1(B, 0), t0(B, 0), t1(B, 0), o0(B, 0), o1(B, 0);
  nfl::device_batch<R> b0(B, 0), b1(B, 0);
  s0.upload(h[0].data()), s1.upload(h[1].data()), t0.upload(h[2].data()), t1.upload(h[3].data());
  nfl::device_batch<S>::template assign_key_switch_level<K>(o0, o1, s1, kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), k0) && same(polys<S>(o1), k1), "device_batch: assign_key_switch_level<K> equals the poly path, polynomial by polynomial");
  nfl::device_batch<S>::template assign_mul_relin_level<K>(o0, o1, s0, s1, &t0, &t1, kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), m0) && same(polys<S>(o1), m1), "device_batch: assign_mul_relin_level<K> equals the poly path");
  nfl::device_batch<S>::template assign_mul_relin_level<K>(b0, b1, s0, s1, &t0, &t1, kbatch, alpha, true, false);
  CHECK(same(polys<R>(b0), r0) && same(polys<R>(b1), r1), "device_batch: the rescaled outputs equal the poly path");
  nfl::device_batch<S>::template assign_mul_relin_level<K>(o0, o1, s0, s1, static_cast<const nfl::device_batch<S> *>(nullptr),
                                                           static_cast<const nfl::device_batch<S> *>(nullptr), kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), q0) && same(polys<S>(o1), q1), "device_batch: the square equals the poly path");
  CHECK(same(polys<S>(s0), h[0]) && same(polys<S>(t1), h[3]) && same(polys<P>(kbatch), key), "device_batch: the inputs and the key stay as they were");
}

int main(int argc, char **argv) {
  try {
    const size_t B = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5;
    if (B == 0) return 2;
    run<uint64_t, 64, 6, 2, 2>(B, 2, "u64/64/6 K=2");    // one digit fewer than the top
    run<uint64_t, 64, 6, 2, 3>(B, 2, "u64/64/6 K=2");    // a short last digit that is full at the top
    run<uint64_t, 64, 6, 2, 4>(B, 2, "u64/64/6 K=2");    // the top level: the existing entries
    run<uint64_t, 64, 6, 2, 2>(B, 3, "u64/64/6 K=2");    // alpha above the level: one short digit
    run<uint32_t, 128, 4, 1, 2>(B, 1, "u32/128/4 K=1");
    std::printf(g_fail ? "level: FAILED (%d)\n" : "level: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("level: exception: %s\n", e.what());
    return 2;
  }
}
