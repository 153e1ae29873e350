// tests/cpp_mulrelin_dot/mulrelin_dot_main.cpp -- sums of ciphertext products on the header surface (include/nfl_hip/poly_p.hpp,
// batch.hpp; include/nflhip.h "sums of ciphertext products"):
//   * nfl::tensor_dot_ntt on nfl::poly equals the sum over terms of nfl::tensor_ntt, added up by the polynomials' own operator;
//   * nfl::mul_relin_dot_level_ntt<K> / square_relin_dot_level_ntt<K> on nfl::poly (the staged host entry) equal the C entry called on
//     raw pointers (buffers of nflhip_malloc) with the strides, the terms, K and the level written out by hand -- with the rescale
//     when the outputs live in the ring with one modulus less --, equal (d0, d1) + key_switch_level_ntt<K>(d2) of tensor_dot_ntt, and
//     at one term nfl::mul_relin_level_ntt<K>;
//   * the same on nfl::poly_p (resident: a pending operand and a pending key polynomial; the dead key polynomials moved from);
//   * device_batch::assign_mul_relin_dot_level<K>: every group equal to the poly path's, dense and shared b, the rescale, the squares.
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_mulrelin_dot.c and of the tests it builds on
// (tests/test_mulrelin_dot_cpp.py).  Usage: mulrelin_dot_test [groups].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
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

// the C entry on raw pointers: G groups of `terms` polynomials per operand (b: `terms` polynomials with shared), the whole key
template <class S, class O, class P, class KB>
static bool raw(const KB &kbatch, std::vector<O> &g0, std::vector<O> &g1, const std::vector<S> *const h[4], int nin, size_t G, size_t terms, bool shared,
                const std::vector<P> &key, size_t K, size_t alpha, int flags) {
  nflhip_ctx *ctx = kbatch.ctx();
  const size_t ob = G * sizeof(O), kbytes = key.size() * sizeof(P);
  void *q0 = nullptr, *q1 = nullptr, *ri[4] = {nullptr, nullptr, nullptr, nullptr}, *rk = nullptr;
  bool ok = nflhip_malloc(ctx, &q0, ob) == 0 && nflhip_malloc(ctx, &q1, ob) == 0 && nflhip_malloc(ctx, &rk, kbytes) == 0;
  nflhip_dot_operand op[4];
  for (int k = 0; k < nin; ++k) {
    const size_t count = (k >= 2 && shared ? 1 : G) * terms;
    ok = ok && nflhip_malloc(ctx, &ri[k], count * sizeof(S)) == 0 && nflhip_memcpy_h2d(ctx, ri[k], (*h[k])[0].cdata(), count * sizeof(S), kbatch.queue()) == 0;
    op[k].ptr = ri[k], op[k].group_stride = k >= 2 && shared ? 0 : terms, op[k].term_stride = 1;
  }
  ok = ok && nflhip_memcpy_h2d(ctx, rk, key[0].cdata(), kbytes, kbatch.queue()) == 0;
  ok = ok && nflhip_mulrelin_dot_ntt_dev(ctx, q0, q1, &op[0], &op[1], nin == 4 ? &op[2] : nullptr, nin == 4 ? &op[3] : nullptr, rk, G, terms, K, alpha,
                                         S::nmoduli, flags, kbatch.queue()) == 0;
  g0.resize(G), g1.resize(G);
  ok = ok && nflhip_memcpy_d2h(ctx, g0[0].data(), q0, ob, kbatch.queue()) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), q1, ob, kbatch.queue()) == 0;
  ok = ok && nflhip_stream_sync(ctx, kbatch.queue()) == 0;
  nflhip_free(ctx, q0), nflhip_free(ctx, q1), nflhip_free(ctx, rk);
  for (int k = 0; k < nin; ++k) nflhip_free(ctx, ri[k]);
  return ok;
}

template <class T, size_t D, size_t M, size_t K, size_t Lv> static void run(size_t G, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, Lv> S;
  typedef nfl::poly<T, D, Lv - 1> R;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, Lv> SP;
  typedef nfl::poly_p<T, D, Lv - 1> RP;
  const size_t terms = 3, dnum = (M - K + alpha - 1) / alpha, live = (Lv + alpha - 1) / alpha;
  std::printf("%s level %zu alpha=%zu, %zu groups of %zu terms\n", name, Lv, alpha, G, terms);
  std::vector<P> key, ka, kb;
  for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial a sum, so that poly_p can hold it pending
    ka.push_back(P(nfl::uniform(0x100 + t)));
    kb.push_back(P(nfl::uniform(0x200 + t)));
    key.push_back(ka[t] + kb[t]);
  }
  std::vector<S> h[4];  // [group][term]
  for (int k = 0; k < 4; ++k) {
    h[k].resize(G * terms);
    for (size_t i = 0; i < G * terms; ++i) h[k][i] = S(nfl::uniform(100 + 10 * i + k));
  }
  const std::vector<S> *const hp[4] = {&h[0], &h[1], &h[2], &h[3]};
  nfl::device_batch<P> kbatch(2 * dnum, 0);
  kbatch.upload(key.data());
  // the poly path, group by group
  std::vector<S> m0(G), m1(G), q0(G), q1(G), sh0(G), sh1(G), g0, g1;
  std::vector<R> r0(G), r1(G), gr0, gr1;
  for (size_t g = 0; g < G; ++g) {
    const S *a0 = &h[0][g * terms], *a1 = &h[1][g * terms], *b0 = &h[2][g * terms], *b1 = &h[3][g * terms];
    nfl::mul_relin_dot_level_ntt<K>(m0[g], m1[g], a0, a1, b0, b1, terms, key.data(), alpha, true, false);
    nfl::square_relin_dot_level_ntt<K>(q0[g], q1[g], a0, a1, terms, key.data(), alpha, true, false);
    nfl::mul_relin_dot_level_ntt<K>(r0[g], r1[g], a0, a1, b0, b1, terms, key.data(), alpha, true, false);
    nfl::mul_relin_dot_level_ntt<K>(sh0[g], sh1[g], a0, a1, &h[2][0], &h[3][0], terms, key.data(), alpha, true, false);   // b of group 0 for every group
  }
  { const bool ok = raw<S, S>(kbatch, g0, g1, hp, 4, G, terms, false, key, K, alpha, NFLHIP_MULRELIN_CENTERED); CHECK(ok, "raw pointers: the sum of products succeeds"); }
  CHECK(same(g0, m0) && same(g1, m1) && !same(m0[0], m1[0]), "poly: mul_relin_dot_level_ntt<K> equals the C entry with the strides, terms, K and level written out");
  { const bool ok = raw<S, S>(kbatch, g0, g1, hp, 2, G, terms, false, key, K, alpha, NFLHIP_MULRELIN_CENTERED); CHECK(ok, "raw pointers: the sum of squares succeeds"); }
  CHECK(same(g0, q0) && same(g1, q1) && !same(q0, m0), "poly: square_relin_dot_level_ntt<K> equals the C entry");
  { const bool ok = raw<S, R>(kbatch, gr0, gr1, hp, 4, G, terms, false, key, K, alpha, NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_RESCALE); CHECK(ok, "raw pointers: the rescale succeeds"); }
  CHECK(same(gr0, r0) && same(gr1, r1) && !same(r0, r1), "poly: the outputs' ring decides the rescale");
  { const bool ok = raw<S, S>(kbatch, g0, g1, hp, 4, G, terms, true, key, K, alpha, NFLHIP_MULRELIN_CENTERED); CHECK(ok, "raw pointers: a shared b succeeds"); }
  CHECK(same(g0, sh0) && same(g1, sh1) && same(sh0[0], m0[0]), "poly: a b shared by every group is group stride 0");
  {  // against the per-term header calls: the tensor products summed, one key switch, two additions
    const S *a0 = &h[0][0], *a1 = &h[1][0], *b0 = &h[2][0], *b1 = &h[3][0];
    S d0, d1, d2, s0, s1, s2;
    nfl::tensor_dot_ntt(d0, d1, d2, a0, a1, b0, b1, terms);
    for (size_t j = 0; j < terms; ++j) {
      S t0, t1, t2;
      nfl::tensor_ntt(t0, t1, t2, a0[j], a1[j], &b0[j], &b1[j]);
      if (j == 0) s0 = t0, s1 = t1, s2 = t2;
      else s0 = s0 + t0, s1 = s1 + t1, s2 = s2 + t2;
    }
    CHECK(same(d0, s0) && same(d1, s1) && same(d2, s2), "poly: tensor_dot_ntt equals the sum of tensor_ntt over the terms");
    S k0, k1;
    nfl::key_switch_level_ntt<K>(k0, k1, d2, key.data(), alpha, true, false);
    const S w0 = d0 + k0, w1 = d1 + k1;
    CHECK(same(w0, m0[0]) && same(w1, m1[0]), "poly: the sum of products equals (d0, d1) + key_switch_level_ntt<K>(d2)");
    S e0, e1, e2;
    nfl::tensor_dot_ntt(e0, e1, e2, a0, a1, static_cast<const S *>(nullptr), static_cast<const S *>(nullptr), terms);
    nfl::tensor_dot_ntt(s0, s1, s2, a0, a1, a0, a1, terms);
    CHECK(same(e0, s0) && same(e1, s1) && same(e2, s2) && !same(e0, d0), "poly: the squares are b = a");
    S o0, o1, x0, x1;
    nfl::mul_relin_dot_level_ntt<K>(o0, o1, a0, a1, b0, b1, 1, key.data(), alpha, true, false);
    nfl::mul_relin_level_ntt<K>(x0, x1, a0[0], a1[0], b0[0], b1[0], key.data(), alpha, true, false);
    CHECK(same(o0, x0) && same(o1, x1), "poly: one term is mul_relin_level_ntt<K>");
    nfl::mul_relin_dot_level_ntt<K>(o0, o1, a0, a1, b0, b1, terms, key.data(), alpha, false, true);
    const bool ok = raw<S, S>(kbatch, g0, g1, hp, 4, 1, terms, false, key, K, alpha, NFLHIP_MULRELIN_FLOOR);
    CHECK(ok && same(o0, g0[0]) && same(o1, g1[0]), "poly: fast mode, floor");
  }
  {  // poly_p: a pending operand and a pending key polynomial; only the live key polynomials are gathered
    std::vector<PP> pkey;
    for (size_t t = 0; t < 2 * dnum; ++t) pkey.push_back(PP(key[t]));
    PP pka(ka[1]), pkb(kb[1]);
    pkey[1] = pka + pkb;
    std::vector<PP> graveyard;
    for (size_t t = 2 * live; t < 2 * dnum; ++t) graveyard.push_back(std::move(pkey[t]));
    std::vector<SP> p[4];
    for (int k = 0; k < 4; ++k)
      for (size_t j = 0; j < terms; ++j) p[k].push_back(SP(h[k][j]));
    S u(nfl::uniform(0x5eed)), v(nfl::uniform(0xbeef));
    const S uv = u + v;
    std::vector<S> hq(h[0].begin(), h[0].begin() + terms);
    hq[1] = uv;
    SP pu(u), pv(v);
    p[0][1] = pu + pv;                                       // pending
    S w0, w1;
    nfl::mul_relin_dot_level_ntt<K>(w0, w1, hq.data(), &h[1][0], &h[2][0], &h[3][0], terms, key.data(), alpha, true, false);
    SP o0, o1;
    nfl::mul_relin_dot_level_ntt<K>(o0, o1, p[0].data(), p[1].data(), p[2].data(), p[3].data(), terms, pkey.data(), alpha, true, false);
    CHECK(same(o0.poly_obj(), w0) && same(o1.poly_obj(), w1), "poly_p: mul_relin_dot_level_ntt<K> with a pending operand and a pending key polynomial");
    CHECK(same(p[0][1].poly_obj(), uv) && same(pkey[1].poly_obj(), key[1]), "poly_p: operand and key stay");
    R x0, x1;
    nfl::mul_relin_dot_level_ntt<K>(x0, x1, hq.data(), &h[1][0], &h[2][0], &h[3][0], terms, key.data(), alpha, true, false);
    RP pr0, pr1;
    nfl::mul_relin_dot_level_ntt<K>(pr0, pr1, p[0].data(), p[1].data(), p[2].data(), p[3].data(), terms, pkey.data(), alpha, true, false);
    CHECK(same(pr0.poly_obj(), x0) && same(pr1.poly_obj(), x1), "poly_p: the rescaled outputs equal the poly path");
    nfl::square_relin_dot_level_ntt<K>(w0, w1, hq.data(), &h[1][0], terms, key.data(), alpha, true, false);
    nfl::square_relin_dot_level_ntt<K>(o0, o1, p[0].data(), p[1].data(), terms, pkey.data(), alpha, true, false);
    CHECK(same(o0.poly_obj(), w0) && same(o1.poly_obj(), w1), "poly_p: square_relin_dot_level_ntt<K> equals the poly path");
    S d0, d1, d2;
    nfl::tensor_dot_ntt(d0, d1, d2, hq.data(), &h[1][0], &h[2][0], &h[3][0], terms);
    SP e0, e1, e2;
    nfl::tensor_dot_ntt(e0, e1, e2, p[0].data(), p[1].data(), p[2].data(), p[3].data(), terms);
    CHECK(same(e0.poly_obj(), d0) && same(e1.poly_obj(), d1) && same(e2.poly_obj(), d2), "poly_p: tensor_dot_ntt equals the poly path");
  }
  // device_batch against the poly path
  nfl::device_batch<S> s0(G * terms, 0), s1(G * terms, 0), t0(G * terms, 0), t1(G * terms, 0), u0(terms, 0), u1(terms, 0), o0(G, 0), o1(G, 0);
  nfl::device_batch<R> b0(G, 0), b1(G, 0);
  s0.upload(h[0].data()), s1.upload(h[1].data()), t0.upload(h[2].data()), t1.upload(h[3].data()), u0.upload(h[2].data()), u1.upload(h[3].data());
  nfl::device_batch<S>::template assign_mul_relin_dot_level<K>(o0, o1, s0, s1, &t0, &t1, terms, kbatch, alpha, false, true, false);
  CHECK(same(polys<S>(o0), m0) && same(polys<S>(o1), m1), "device_batch: assign_mul_relin_dot_level<K> equals the poly path, group by group");
  nfl::device_batch<S>::template assign_mul_relin_dot_level<K>(b0, b1, s0, s1, &t0, &t1, terms, kbatch, alpha, false, true, false);
  CHECK(same(polys<R>(b0), r0) && same(polys<R>(b1), r1), "device_batch: the rescaled outputs equal the poly path");
  nfl::device_batch<S>::template assign_mul_relin_dot_level<K>(o0, o1, s0, s1, &u0, &u1, terms, kbatch, alpha, true, true, false);
  CHECK(same(polys<S>(o0), sh0) && same(polys<S>(o1), sh1), "device_batch: a shared b equals the poly path");
  nfl::device_batch<S>::template assign_mul_relin_dot_level<K>(o0, o1, s0, s1, static_cast<const nfl::device_batch<S> *>(nullptr),
                                                               static_cast<const nfl::device_batch<S> *>(nullptr), terms, kbatch, alpha, false, true, false);
  CHECK(same(polys<S>(o0), q0) && same(polys<S>(o1), q1), "device_batch: the squares equal the poly path");
  CHECK(same(polys<S>(s0), h[0]) && same(polys<S>(t1), h[3]) && same(polys<P>(kbatch), key), "device_batch: the inputs and the key stay as they were");
}

int main(int argc, char **argv) {
  try {
    const size_t G = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 3;
    if (G == 0) return 2;
    run<uint64_t, 64, 6, 2, 2>(G, 2, "u64/64/6 K=2");    // one digit fewer than the top
    run<uint64_t, 64, 6, 2, 3>(G, 2, "u64/64/6 K=2");    // a short last digit that is full at the top
    run<uint64_t, 64, 6, 2, 4>(G, 2, "u64/64/6 K=2");    // the top level
    run<uint32_t, 128, 4, 1, 2>(G, 1, "u32/128/4 K=1");
    std::printf(g_fail ? "mulrelin_dot: FAILED (%d)\n" : "mulrelin_dot: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("mulrelin_dot: exception: %s\n", e.what());
    return 2;
  }
}
