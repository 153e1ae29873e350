// tests/cpp_level_rotate/level_rotate_main.cpp -- hoisted rotations and slot linear transforms below the top level on the header surface
// (include/nfl_hip/poly_p.hpp, batch.hpp; include/nflhip.h "rotations and linear transforms at a level"):
//   * nfl::rotate_hoisted_level_ntt<K> and nfl::linear_transform_level_ntt<K> on nfl::poly (the staged host entries) equal the C entries
//     called on raw pointers (buffers of nflhip_malloc) with K, the level, the WHOLE top-level keys and the whole diagonals written out
//     by hand;
//   * at the top level, Lv = M - K, they equal the existing nfl::rotate_hoisted_ntt / nfl::linear_transform_ntt;
//   * the same on nfl::poly_p (resident: deferred work pending on an input, on a key polynomial and on a diagonal; a copy-on-write
//     sharer keeps the old value; an output may be an input) -- only the live key polynomials are gathered: the dead ones of every
//     key array are moved from, and touching one would throw;
//   * device_batch::assign_rotations_level<K> / assign_linear_transform_level<K>: every polynomial equal to the poly path's.
// Two rotations (k = 5 and 2 D - 1) with a key each; the linear transform has a third, unkeyed term (k = 1, no key).
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_level_rotate.c and of the tests it builds on
// (tests/test_level_rotate_cpp.py).  Usage: level_rotate_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
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

static const size_t ROT = 2, TERMS = 3;  // rotations; terms of the linear transform, the last one unkeyed

// the C entries on raw pointers: B polynomials per operand, the whole keys and diagonals.  rot: outs = [ROT][2][B], else [2][B]
template <class S, class P, class KB>
static bool raw(const KB &kbatch, std::vector<std::vector<S> > &g, const std::vector<S> &c0, const std::vector<S> &c1, const std::vector<P> *keys,
                const std::vector<P> &ws, const uint64_t *ks, size_t K, size_t alpha, int flags, bool rot) {
  nflhip_ctx *ctx = kbatch.ctx();
  void *q = kbatch.queue();
  const size_t B = c1.size(), ob = B * sizeof(S), kbytes = keys[0].size() * sizeof(P), nout = rot ? 2 * ROT : 2;
  void *r0 = nullptr, *r1 = nullptr, *rk[ROT] = {nullptr, nullptr}, *rw[TERMS] = {nullptr, nullptr, nullptr};
  std::vector<void *> out(nout, nullptr);
  bool ok = nflhip_malloc(ctx, &r0, ob) == 0 && nflhip_malloc(ctx, &r1, ob) == 0;
  ok = ok && nflhip_memcpy_h2d(ctx, r0, c0[0].cdata(), ob, q) == 0 && nflhip_memcpy_h2d(ctx, r1, c1[0].cdata(), ob, q) == 0;
  for (size_t m = 0; m < ROT; ++m) ok = ok && nflhip_malloc(ctx, &rk[m], kbytes) == 0 && nflhip_memcpy_h2d(ctx, rk[m], keys[m][0].cdata(), kbytes, q) == 0;
  for (size_t m = 0; m < TERMS; ++m) ok = ok && nflhip_malloc(ctx, &rw[m], sizeof(P)) == 0 && nflhip_memcpy_h2d(ctx, rw[m], ws[m].cdata(), sizeof(P), q) == 0;
  for (size_t o = 0; o < nout; ++o) ok = ok && nflhip_malloc(ctx, &out[o], ob) == 0;
  const void *kp[TERMS] = {rk[0], rk[1], nullptr}, *wp[TERMS] = {rw[0], rw[1], rw[2]};
  if (rot) {
    void *o0[ROT] = {out[0], out[2]}, *o1[ROT] = {out[1], out[3]};
    ok = ok && nflhip_rotate_hoisted_level_ntt_dev(ctx, o0, o1, r0, r1, kp, ks, ROT, B, K, alpha, S::nmoduli, flags, q) == 0;
  } else {
    ok = ok && nflhip_lintrans_level_ntt_dev(ctx, out[0], out[1], r0, r1, kp, wp, ks, TERMS, B, K, alpha, S::nmoduli, flags, q) == 0;
  }
  g.assign(nout, std::vector<S>(B));
  for (size_t o = 0; o < nout; ++o) ok = ok && nflhip_memcpy_d2h(ctx, g[o][0].data(), out[o], ob, q) == 0;
  ok = ok && nflhip_stream_sync(ctx, q) == 0;
  nflhip_free(ctx, r0), nflhip_free(ctx, r1);
  for (size_t m = 0; m < ROT; ++m) nflhip_free(ctx, rk[m]);
  for (size_t m = 0; m < TERMS; ++m) nflhip_free(ctx, rw[m]);
  for (size_t o = 0; o < nout; ++o) nflhip_free(ctx, out[o]);
  return ok;
}

template <bool TOP> struct top_level {  // below the top level: nothing to compare with
  template <class S, class P> static void check(std::vector<S> const &, std::vector<S> const &, P const *const *, P const *const *, const uint64_t *, size_t,
                                                std::vector<std::vector<S> > const &, std::vector<std::vector<S> > const &) {}
};
template <> struct top_level<true> {
  template <class S, class P> static void check(std::vector<S> const &c0, std::vector<S> const &c1, P const *const *kp, P const *const *wp, const uint64_t *ks,
                                                size_t alpha, std::vector<std::vector<S> > const &rot, std::vector<std::vector<S> > const &lt) {
    for (size_t i = 0; i < c1.size(); ++i) {
      S x0[ROT], x1[ROT], y0, y1;
      nfl::rotate_hoisted_ntt(x0, x1, &c0[i], c1[i], kp, ks, ROT, alpha, true, false);
      CHECK(same(x0[0], rot[0][i]) && same(x1[0], rot[1][i]) && same(x0[1], rot[2][i]) && same(x1[1], rot[3][i]),
            "at the top level rotate_hoisted_level_ntt<K> is rotate_hoisted_ntt");
      nfl::linear_transform_ntt(y0, y1, &c0[i], c1[i], kp, wp, ks, TERMS, alpha, true, false);
      CHECK(same(y0, lt[0][i]) && same(y1, lt[1][i]), "at the top level linear_transform_level_ntt<K> is linear_transform_ntt");
    }
  }
};

template <class T, size_t D, size_t M, size_t K, size_t Lv> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, Lv> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, Lv> SP;
  const size_t dnum = (M - K + alpha - 1) / alpha, live = (Lv + alpha - 1) / alpha;
  std::printf("%s level %zu alpha=%zu, %zu digits of %zu live, %zu polynomials\n", name, Lv, alpha, live, dnum, B);
  const uint64_t ks[TERMS] = {5, 2 * D - 1, 1};
  std::vector<P> key[ROT], ka, kb, ws;
  for (size_t m = 0; m < ROT; ++m)
    for (size_t t = 0; t < 2 * dnum; ++t) key[m].push_back(P(nfl::uniform(0x100 + 0x40 * m + t)));
  ka.push_back(P(nfl::uniform(0x300))), kb.push_back(P(nfl::uniform(0x301)));
  key[1][1] = ka[0] + kb[0];  // a key polynomial that poly_p can hold pending
  for (size_t m = 0; m < TERMS; ++m) ws.push_back(P(nfl::uniform(0x400 + m)));
  std::vector<S> c0(B), c1(B);
  for (size_t i = 0; i < B; ++i) c0[i] = S(nfl::uniform(100 + 10 * i)), c1[i] = S(nfl::uniform(101 + 10 * i));
  const P *kp[TERMS] = {key[0].data(), key[1].data(), nullptr}, *wp[TERMS] = {&ws[0], &ws[1], &ws[2]};
  nfl::device_batch<P> kb0(2 * dnum, 0), kb1(2 * dnum, 0), wb0(1, 0), wb1(1, 0), wb2(1, 0);
  kb0.upload(key[0].data()), kb1.upload(key[1].data()), wb0.upload(&ws[0]), wb1.upload(&ws[1]), wb2.upload(&ws[2]);
  // the poly path against the C entries on raw pointers
  std::vector<std::vector<S> > rot(2 * ROT, std::vector<S>(B)), lt(2, std::vector<S>(B)), g;
  for (size_t i = 0; i < B; ++i) {
    S x0[ROT], x1[ROT];
    nfl::rotate_hoisted_level_ntt<K>(x0, x1, &c0[i], c1[i], kp, ks, ROT, alpha, true, false);
    rot[0][i] = x0[0], rot[1][i] = x1[0], rot[2][i] = x0[1], rot[3][i] = x1[1];
    nfl::linear_transform_level_ntt<K>(lt[0][i], lt[1][i], &c0[i], c1[i], kp, wp, ks, TERMS, alpha, true, false);
  }
  { const bool ok = raw<S, P>(kb0, g, c0, c1, key, ws, ks, K, alpha, NFLHIP_ROTATE_CENTERED, true); CHECK(ok, "raw pointers: the rotations succeed"); }
  CHECK(g.size() == 2 * ROT && same(g[0], rot[0]) && same(g[1], rot[1]) && same(g[2], rot[2]) && same(g[3], rot[3]),
        "poly: rotate_hoisted_level_ntt<K> equals the C entry with K and the level written out");
  CHECK(!same(rot[0][0], rot[2][0]) && !same(rot[0][0], rot[1][0]), "poly: the rotations and the components differ");
  { const bool ok = raw<S, P>(kb0, g, c0, c1, key, ws, ks, K, alpha, NFLHIP_LINTRANS_CENTERED, false); CHECK(ok, "raw pointers: the linear transform succeeds"); }
  CHECK(g.size() == 2 && same(g[0], lt[0]) && same(g[1], lt[1]) && !same(lt[0][0], lt[1][0]), "poly: linear_transform_level_ntt<K> equals the C entry");
  top_level<Lv == M - K>::check(c0, c1, kp, wp, ks, alpha, rot, lt);
  {  // the modes reach the entry; c0 may be NULL; an output may be an input
    S x0[ROT], x1[ROT], y0, y1;
    nfl::rotate_hoisted_level_ntt<K>(x0, x1, &c0[0], c1[0], kp, ks, ROT, alpha, false, true);
    const bool ok = raw<S, P>(kb0, g, c0, c1, key, ws, ks, K, alpha, NFLHIP_ROTATE_FLOOR, true);
    CHECK(ok && same(x0[1], g[2][0]) && same(x1[1], g[3][0]), "poly: fast mode, floor");
    nfl::linear_transform_level_ntt<K>(y0, y1, static_cast<const S *>(nullptr), c1[0], kp, wp, ks, TERMS, alpha, true, false);
    CHECK(!same(y0, lt[0][0]) && same(y1, lt[1][0]), "poly: without c0 only out0 changes");
    S a(c0[0]), b(c1[0]);
    nfl::linear_transform_level_ntt<K>(a, b, &a, b, kp, wp, ks, TERMS, alpha, true, false);
    CHECK(same(a, lt[0][0]) && same(b, lt[1][0]), "poly: the outputs may be the inputs");
  }
  {  // poly_p: an input, a key polynomial and a diagonal pending; sharers keep their values; the dead key polynomials are moved from
    S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
    const S a1 = a + b;
    S w0[ROT], w1[ROT], v0, v1;
    nfl::rotate_hoisted_level_ntt<K>(w0, w1, &c0[0], a1, kp, ks, ROT, alpha, true, false);
    nfl::linear_transform_level_ntt<K>(v0, v1, &c0[0], a1, kp, wp, ks, TERMS, alpha, true, false);
    std::vector<PP> pkey[ROT], pws, graveyard;
    for (size_t m = 0; m < ROT; ++m)
      for (size_t t = 0; t < 2 * dnum; ++t) pkey[m].push_back(PP(key[m][t]));
    PP pka(ka[0]), pkb(kb[0]);
    pkey[1][1] = pka + pkb;
    for (size_t m = 0; m < ROT; ++m)
      for (size_t t = 2 * live; t < 2 * dnum; ++t) graveyard.push_back(std::move(pkey[m][t]));
    for (size_t m = 0; m < TERMS; ++m) pws.push_back(PP(ws[m]));
    PP half(ws[2]);
    pws[2] = half + half - half;  // a diagonal with deferred work pending
    const PP *pkp[TERMS] = {pkey[0].data(), pkey[1].data(), nullptr}, *pwp[TERMS] = {&pws[0], &pws[1], &pws[2]};
    SP pa(a), pb(b), pc0(c0[0]);
    SP pa1 = pa + pb;
    SP o0[ROT], o1[ROT];
    o0[0] = pa * pb;
    SP keep = o0[0];
    const S ab = a * b;
    nfl::rotate_hoisted_level_ntt<K>(o0, o1, &pc0, pa1, pkp, ks, ROT, alpha, true, false);
    CHECK(same(o0[0].poly_obj(), w0[0]) && same(o1[0].poly_obj(), w1[0]) && same(o0[1].poly_obj(), w0[1]) && same(o1[1].poly_obj(), w1[1]),
          "poly_p: rotate_hoisted_level_ntt<K> of a pending input with a pending key polynomial");
    CHECK(same(keep.poly_obj(), ab) && same(pa1.poly_obj(), a1) && same(pkey[1][1].poly_obj(), key[1][1]), "poly_p: the sharer keeps the old value; input and key stay");
    SP l0, l1;
    nfl::linear_transform_level_ntt<K>(l0, l1, &pc0, pa1, pkp, pwp, ks, TERMS, alpha, true, false);
    CHECK(same(l0.poly_obj(), v0) && same(l1.poly_obj(), v1), "poly_p: linear_transform_level_ntt<K> equals the poly path");
    SP sharer = pa1;
    nfl::linear_transform_level_ntt<K>(pc0, pa1, &pc0, pa1, pkp, pwp, ks, TERMS, alpha, true, false);
    CHECK(same(pc0.poly_obj(), v0) && same(pa1.poly_obj(), v1) && same(sharer.poly_obj(), a1), "poly_p: the outputs may be the inputs; a sharer keeps the input");
  }
  // device_batch against the poly path
  nfl::device_batch<S> s0(B, 0), s1(B, 0), a0(B, 0), a1(B, 0), b0(B, 0), b1(B, 0);
  s0.upload(c0.data()), s1.upload(c1.data());
  nfl::device_batch<S> *r0[ROT] = {&a0, &b0}, *r1[ROT] = {&a1, &b1};
  const nfl::device_batch<P> *kbs[TERMS] = {&kb0, &kb1, nullptr}, *wbs[TERMS] = {&wb0, &wb1, &wb2};
  nfl::device_batch<S>::template assign_rotations_level<K>(r0, r1, &s0, s1, kbs, ks, ROT, alpha, true, false);
  CHECK(same(polys<S>(a0), rot[0]) && same(polys<S>(a1), rot[1]) && same(polys<S>(b0), rot[2]) && same(polys<S>(b1), rot[3]),
        "device_batch: assign_rotations_level<K> equals the poly path, polynomial by polynomial");
  nfl::device_batch<S>::template assign_linear_transform_level<K>(a0, a1, &s0, s1, kbs, wbs, ks, TERMS, alpha, true, false);
  CHECK(same(polys<S>(a0), lt[0]) && same(polys<S>(a1), lt[1]), "device_batch: assign_linear_transform_level<K> equals the poly path");
  CHECK(same(polys<S>(s0), c0) && same(polys<S>(s1), c1) && same(polys<P>(kb1), key[1]) && same(polys<P>(wb2), std::vector<P>(1, ws[2])),
        "device_batch: the inputs, the keys and the diagonals stay as they were");
}

int main(int argc, char **argv) {
  try {
    const size_t B = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5;
    if (B == 0) return 2;
    run<uint64_t, 64, 6, 2, 1>(B, 2, "u64/64/6 K=2");    // a digit shorter than alpha
    run<uint64_t, 64, 6, 2, 3>(B, 2, "u64/64/6 K=2");    // a short last digit that is full at the top
    run<uint64_t, 64, 6, 2, 4>(B, 2, "u64/64/6 K=2");    // the top level: the existing entries
    run<uint64_t, 64, 6, 2, 3>(B, 1, "u64/64/6 K=2");    // three digits of four
    run<uint32_t, 128, 4, 1, 2>(B, 1, "u32/128/4 K=1");
    std::printf(g_fail ? "level_rotate: FAILED (%d)\n" : "level_rotate: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("level_rotate: exception: %s\n", e.what());
    return 2;
  }
}
