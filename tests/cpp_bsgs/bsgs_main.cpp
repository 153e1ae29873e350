// tests/cpp_bsgs/bsgs_main.cpp -- BSGS slot linear transforms on the header surface (include/nfl_hip/poly_p.hpp, batch.hpp;
// include/nflhip.h "BSGS slot linear transforms"):
//   * nfl::bsgs_linear_transform_ntt<K> on nfl::poly (the staged host entry) equals the C entry called on raw pointers (buffers of
//     nflhip_malloc) with the baby keys, the giant keys, the diagonals at j * n1 + i, K and the level written out by hand;
//   * the same on nfl::poly_p (resident: deferred work pending on an input, on a key polynomial and on a diagonal; a copy-on-write
//     sharer keeps the old value; an output may be an input) -- only the live key polynomials are gathered: the dead ones of every key
//     array are moved from, and touching one would throw;
//   * device_batch::assign_bsgs_linear_transform<K>: every polynomial equal to the poly path's.
// N1 = 3 baby steps (k = 5 and 25 keyed, k = 1 without a key) and N2 = 2 giant steps (k = 2 D - 1 keyed, k = 1 without a key); the
// diagonal of (1, 2) is NULL.  N1 != N2 and every diagonal differs, so a transposed weight index shows.
// Every check is an equality between two surfaces over the same entry, so the program runs against the real library (GPU) and, on the
// CPU, against tests/cpp/mock plus the toy entry of toy_bsgs.c and the toys it builds on (tests/test_bsgs_cpp.py).
// Usage: bsgs_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
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

static const size_t N1 = 3, N2 = 2, KEYS = 3, NW = N1 * N2, NULL_W = 1 * N1 + 2;  // keys: babies 0 and 1, giant 0

// the C entry on raw pointers: B polynomials per operand, the whole keys and diagonals; g = [2][B]
template <class S, class P, class KB>
static bool raw(const KB &kbatch, std::vector<std::vector<S> > &g, const std::vector<S> &c0, const std::vector<S> &c1, const std::vector<P> *keys,
                const std::vector<P> &ws, const uint64_t *bks, const uint64_t *gks, size_t K, size_t alpha, int flags) {
  nflhip_ctx *ctx = kbatch.ctx();
  void *q = kbatch.queue();
  const size_t B = c1.size(), ob = B * sizeof(S), kbytes = keys[0].size() * sizeof(P);
  void *r0 = nullptr, *r1 = nullptr, *rk[KEYS] = {nullptr, nullptr, nullptr}, *rw[NW] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
       *out[2] = {nullptr, nullptr};
  bool ok = nflhip_malloc(ctx, &r0, ob) == 0 && nflhip_malloc(ctx, &r1, ob) == 0;
  ok = ok && nflhip_memcpy_h2d(ctx, r0, c0[0].cdata(), ob, q) == 0 && nflhip_memcpy_h2d(ctx, r1, c1[0].cdata(), ob, q) == 0;
  for (size_t m = 0; m < KEYS; ++m) ok = ok && nflhip_malloc(ctx, &rk[m], kbytes) == 0 && nflhip_memcpy_h2d(ctx, rk[m], keys[m][0].cdata(), kbytes, q) == 0;
  for (size_t m = 0; m < NW; ++m) ok = ok && nflhip_malloc(ctx, &rw[m], sizeof(P)) == 0 && nflhip_memcpy_h2d(ctx, rw[m], ws[m].cdata(), sizeof(P), q) == 0;
  for (size_t o = 0; o < 2; ++o) ok = ok && nflhip_malloc(ctx, &out[o], ob) == 0;
  const void *bp[N1] = {rk[0], rk[1], nullptr}, *gp[N2] = {rk[2], nullptr}, *wp[NW];
  for (size_t m = 0; m < NW; ++m) wp[m] = m == NULL_W ? nullptr : rw[m];
  ok = ok && nflhip_bsgs_ntt_dev(ctx, out[0], out[1], r0, r1, bp, bks, N1, gp, gks, N2, wp, B, K, alpha, S::nmoduli, flags, q) == 0;
  g.assign(2, std::vector<S>(B));
  for (size_t o = 0; o < 2; ++o) ok = ok && nflhip_memcpy_d2h(ctx, g[o][0].data(), out[o], ob, q) == 0;
  ok = ok && nflhip_stream_sync(ctx, q) == 0;
  nflhip_free(ctx, r0), nflhip_free(ctx, r1);
  for (size_t m = 0; m < KEYS; ++m) nflhip_free(ctx, rk[m]);
  for (size_t m = 0; m < NW; ++m) nflhip_free(ctx, rw[m]);
  for (size_t o = 0; o < 2; ++o) nflhip_free(ctx, out[o]);
  return ok;
}

template <class T, size_t D, size_t M, size_t K, size_t Lv> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, Lv> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, Lv> SP;
  const size_t dnum = (M - K + alpha - 1) / alpha, live = (Lv + alpha - 1) / alpha;
  std::printf("%s level %zu alpha=%zu, %zu digits of %zu live, %zu polynomials\n", name, Lv, alpha, live, dnum, B);
  const uint64_t bks[N1] = {5, 25, 1}, gks[N2] = {2 * D - 1, 1};
  std::vector<P> key[KEYS], ka, kb, ws;
  for (size_t m = 0; m < KEYS; ++m)
    for (size_t t = 0; t < 2 * dnum; ++t) key[m].push_back(P(nfl::uniform(0x100 + 0x40 * m + t)));
  ka.push_back(P(nfl::uniform(0x300))), kb.push_back(P(nfl::uniform(0x301)));
  key[1][1] = ka[0] + kb[0];  // a key polynomial that poly_p can hold pending
  for (size_t m = 0; m < NW; ++m) ws.push_back(P(nfl::uniform(0x400 + m)));
  std::vector<S> c0(B), c1(B);
  for (size_t i = 0; i < B; ++i) c0[i] = S(nfl::uniform(100 + 10 * i)), c1[i] = S(nfl::uniform(101 + 10 * i));
  const P *bp[N1] = {key[0].data(), key[1].data(), nullptr}, *gp[N2] = {key[2].data(), nullptr}, *wp[NW];
  for (size_t m = 0; m < NW; ++m) wp[m] = m == NULL_W ? nullptr : &ws[m];
  nfl::device_batch<P> kb0(2 * dnum, 0), kb1(2 * dnum, 0), kb2(2 * dnum, 0);
  kb0.upload(key[0].data()), kb1.upload(key[1].data()), kb2.upload(key[2].data());
  std::vector<nfl::device_batch<P> *> wb;
  for (size_t m = 0; m < NW; ++m) {
    wb.push_back(new nfl::device_batch<P>(1, 0));
    wb[m]->upload(&ws[m]);
  }
  // the poly path against the C entry on raw pointers
  std::vector<std::vector<S> > lt(2, std::vector<S>(B)), g;
  for (size_t i = 0; i < B; ++i) nfl::bsgs_linear_transform_ntt<K>(lt[0][i], lt[1][i], &c0[i], c1[i], bp, bks, N1, gp, gks, N2, wp, alpha, true, false);
  { const bool ok = raw<S, P>(kb0, g, c0, c1, key, ws, bks, gks, K, alpha, NFLHIP_BSGS_CENTERED); CHECK(ok, "raw pointers: the call succeeds"); }
  CHECK(g.size() == 2 && same(g[0], lt[0]) && same(g[1], lt[1]) && !same(lt[0][0], lt[1][0]), "poly: bsgs_linear_transform_ntt<K> equals the C entry");
  {  // the modes reach the entry; c0 may be NULL; an output may be an input
    S y0, y1;
    nfl::bsgs_linear_transform_ntt<K>(y0, y1, &c0[0], c1[0], bp, bks, N1, gp, gks, N2, wp, alpha, false, true);
    const bool ok = raw<S, P>(kb0, g, c0, c1, key, ws, bks, gks, K, alpha, NFLHIP_BSGS_FLOOR);
    CHECK(ok && same(y0, g[0][0]) && same(y1, g[1][0]), "poly: fast mode, floor");
    nfl::bsgs_linear_transform_ntt<K>(y0, y1, static_cast<const S *>(nullptr), c1[0], bp, bks, N1, gp, gks, N2, wp, alpha, true, false);
    CHECK(!same(y0, lt[0][0]), "poly: without c0 out0 changes");
    S a(c0[0]), b(c1[0]);
    nfl::bsgs_linear_transform_ntt<K>(a, b, &a, b, bp, bks, N1, gp, gks, N2, wp, alpha, true, false);
    CHECK(same(a, lt[0][0]) && same(b, lt[1][0]), "poly: the outputs may be the inputs");
  }
  {  // poly_p: an input, a key polynomial and a diagonal pending; sharers keep their values; the dead key polynomials are moved from
    S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
    const S a1 = a + b;
    S v0, v1;
    nfl::bsgs_linear_transform_ntt<K>(v0, v1, &c0[0], a1, bp, bks, N1, gp, gks, N2, wp, alpha, true, false);
    std::vector<PP> pkey[KEYS], pws, graveyard;
    for (size_t m = 0; m < KEYS; ++m)
      for (size_t t = 0; t < 2 * dnum; ++t) pkey[m].push_back(PP(key[m][t]));
    PP pka(ka[0]), pkb(kb[0]);
    pkey[1][1] = pka + pkb;
    for (size_t m = 0; m < KEYS; ++m)
      for (size_t t = 2 * live; t < 2 * dnum; ++t) graveyard.push_back(std::move(pkey[m][t]));
    for (size_t m = 0; m < NW; ++m) pws.push_back(PP(ws[m]));
    PP half(ws[2]);
    pws[2] = half + half - half;  // a diagonal with deferred work pending
    const PP *pbp[N1] = {pkey[0].data(), pkey[1].data(), nullptr}, *pgp[N2] = {pkey[2].data(), nullptr}, *pwp[NW];
    for (size_t m = 0; m < NW; ++m) pwp[m] = m == NULL_W ? nullptr : &pws[m];
    SP pa(a), pb(b), pc0(c0[0]);
    SP pa1 = pa + pb;
    SP l0 = pa * pb, l1;
    SP keep = l0;
    const S ab = a * b;
    nfl::bsgs_linear_transform_ntt<K>(l0, l1, &pc0, pa1, pbp, bks, N1, pgp, gks, N2, pwp, alpha, true, false);
    CHECK(same(l0.poly_obj(), v0) && same(l1.poly_obj(), v1), "poly_p: bsgs_linear_transform_ntt<K> of a pending input equals the poly path");
    CHECK(same(keep.poly_obj(), ab) && same(pa1.poly_obj(), a1) && same(pkey[1][1].poly_obj(), key[1][1]), "poly_p: the sharer keeps the old value; input and key stay");
    SP sharer = pa1;
    nfl::bsgs_linear_transform_ntt<K>(pc0, pa1, &pc0, pa1, pbp, bks, N1, pgp, gks, N2, pwp, alpha, true, false);
    CHECK(same(pc0.poly_obj(), v0) && same(pa1.poly_obj(), v1) && same(sharer.poly_obj(), a1), "poly_p: the outputs may be the inputs; a sharer keeps the input");
  }
  // device_batch against the poly path
  nfl::device_batch<S> s0(B, 0), s1(B, 0), a0(B, 0), a1(B, 0);
  s0.upload(c0.data()), s1.upload(c1.data());
  const nfl::device_batch<P> *bbs[N1] = {&kb0, &kb1, nullptr}, *gbs[N2] = {&kb2, nullptr}, *wbs[NW];
  for (size_t m = 0; m < NW; ++m) wbs[m] = m == NULL_W ? nullptr : wb[m];
  nfl::device_batch<S>::template assign_bsgs_linear_transform<K>(a0, a1, &s0, s1, bbs, bks, N1, gbs, gks, N2, wbs, alpha, true, false);
  CHECK(same(polys<S>(a0), lt[0]) && same(polys<S>(a1), lt[1]), "device_batch: assign_bsgs_linear_transform<K> equals the poly path");
  CHECK(same(polys<S>(s0), c0) && same(polys<S>(s1), c1) && same(polys<P>(kb1), key[1]) && same(polys<P>(*wb[2]), std::vector<P>(1, ws[2])),
        "device_batch: the inputs, the keys and the diagonals stay as they were");
  for (size_t m = 0; m < NW; ++m) delete wb[m];
}

int main(int argc, char **argv) {
  try {
    const size_t B = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5;
    if (B == 0) return 2;
    run<uint64_t, 64, 6, 2, 1>(B, 2, "u64/64/6 K=2");    // a digit shorter than alpha
    run<uint64_t, 64, 6, 2, 3>(B, 2, "u64/64/6 K=2");    // a short last digit that is full at the top
    run<uint64_t, 64, 6, 2, 4>(B, 2, "u64/64/6 K=2");    // the top level
    run<uint64_t, 64, 6, 2, 3>(B, 1, "u64/64/6 K=2");    // three digits of four
    run<uint32_t, 128, 4, 1, 2>(B, 1, "u32/128/4 K=1");
    std::printf(g_fail ? "bsgs: FAILED (%d)\n" : "bsgs: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("bsgs: exception: %s\n", e.what());
    return 2;
  }
}
