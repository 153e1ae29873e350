// tests/cpp_lintrans/lintrans_main.cpp -- slot linear transforms of the header surface (include/nfl_hip/poly_p.hpp, batch.hpp):
//   * nfl::linear_transform_ntt on nfl::poly (host-pointer path): with only unrotated diagonals (NULL keys, k = 1) it equals the sums
//     written by hand through the header's own products and sums; c0 enters out0 only; different keys and different diagonals give
//     different results; an output may be c0 or c1;
//   * nfl::linear_transform_ntt on nfl::poly_p (resident: deferred work pending on c0, c1, a key polynomial, a diagonal and an
//     output's old value; a copy-on-write sharer keeps the old value; work recorded after sees the result) equals the poly path;
//   * device_batch::assign_linear_transform: every polynomial equal to the poly path's, and the keys and diagonals used through
//     device_batches equal to those used through raw pointers (nflhip_lintrans_ntt_dev on buffers of nflhip_malloc).
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_lintrans.c, tests/cpp_rotate, tests/cpp_keyswitch,
// tests/cpp_baseconv_ntt and tests/cpp_baseconv (tests/test_lintrans_cpp.py).
// Usage: lintrans_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static const size_t COUNT = 4;

template <class T, size_t D, size_t M, size_t K> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  const size_t L = M - K, dnum = (L + alpha - 1) / alpha;
  std::printf("%s alpha=%zu, %zu digits, %zu terms, %zu polynomials\n", name, alpha, dnum, COUNT, B);
  const uint64_t ks[COUNT] = {5, 1, 2 * D - 1, 5};  // term 1 is the unrotated diagonal; a repeated k, with another key and diagonal
  const uint64_t ones[COUNT] = {1, 1, 1, 1};
  std::vector<std::vector<P>> key(COUNT), ka(COUNT), kb(COUNT);
  std::vector<P> w, wa, wb;
  const P *kptr[COUNT], *wptr[COUNT], *nokey[COUNT];
  for (size_t m = 0; m < COUNT; ++m) {
    for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial and diagonal a sum, so that poly_p can hold it pending
      ka[m].push_back(P(nfl::uniform(0x100 + 64 * m + t)));
      kb[m].push_back(P(nfl::uniform(0x200 + 64 * m + t)));
      key[m].push_back(ka[m][t] + kb[m][t]);
    }
    wa.push_back(P(nfl::uniform(0x300 + m)));
    wb.push_back(P(nfl::uniform(0x400 + m)));
    w.push_back(wa[m] + wb[m]);
  }
  for (size_t m = 0; m < COUNT; ++m) kptr[m] = ks[m] == 1 ? nullptr : key[m].data(), wptr[m] = &w[m], nokey[m] = nullptr;
  S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  const S c1 = a + b, c0 = c + d, cd = c * d;
  for (int mode = 0; mode < 4; ++mode) {
    const bool centered = (mode & 1) != 0, floor = (mode & 2) != 0;
    // only unrotated diagonals: the sums by hand, on the first L rows of every diagonal
    {
      std::vector<S> wl(COUNT);
      for (size_t m = 0; m < COUNT; ++m) std::memcpy(static_cast<void *>(wl[m].data()), w[m].cdata(), sizeof(S));
      S h0 = wl[0] * c0, h1 = wl[0] * c1;
      for (size_t m = 1; m < COUNT; ++m) {
        const S t0 = wl[m] * c0, t1 = wl[m] * c1;
        h0 = h0 + t0;
        h1 = h1 + t1;
      }
      S u0, u1;
      nfl::linear_transform_ntt(u0, u1, &c0, c1, nokey, wptr, ones, COUNT, alpha, centered, floor);
      CHECK(same(u0, h0) && same(u1, h1), "poly: with unrotated diagonals only, the sums of products written by hand");
    }
    S w0, w1, n0, n1;
    nfl::linear_transform_ntt(w0, w1, &c0, c1, kptr, wptr, ks, COUNT, alpha, centered, floor);
    nfl::linear_transform_ntt(n0, n1, static_cast<const S *>(nullptr), c1, kptr, wptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(n1, w1) && !same(n0, w0), "poly: c0 enters out0 only");
    {
      const P *k2[COUNT] = {kptr[3], kptr[1], kptr[2], kptr[0]}, *w2[COUNT] = {wptr[3], wptr[1], wptr[2], wptr[0]};
      S x0, x1, y0, y1;
      nfl::linear_transform_ntt(x0, x1, &c0, c1, k2, wptr, ks, COUNT, alpha, centered, floor);
      nfl::linear_transform_ntt(y0, y1, &c0, c1, kptr, w2, ks, COUNT, alpha, centered, floor);
      CHECK(!same(x0, w0) && !same(x1, w1) && !same(y0, w0) && !same(y1, w1) && !same(w0, w1), "poly: keys and diagonals are paired with their terms");
    }
    S x0 = c0, x1 = c1;
    nfl::linear_transform_ntt(x0, x1, &x0, x1, kptr, wptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(x0, w0) && same(x1, w1), "poly: an output may be c0 or c1");
    // poly_p: c0, c1, a key polynomial, a diagonal and an output's old value pending; sharers keep their values
    std::vector<std::vector<PP>> pkey(COUNT);
    std::vector<PP> pw;
    const PP *pkptr[COUNT], *pwptr[COUNT];
    PP pka(ka[2][1]), pkb(kb[2][1]), pwa(wa[1]), pwb(wb[1]);
    for (size_t m = 0; m < COUNT; ++m) {
      for (size_t t = 0; t < 2 * dnum; ++t) pkey[m].push_back(PP(key[m][t]));
      pw.push_back(PP(w[m]));
    }
    pkey[2][1] = pka + pkb;
    pw[1] = pwa + pwb;
    for (size_t m = 0; m < COUNT; ++m) pkptr[m] = ks[m] == 1 ? nullptr : pkey[m].data(), pwptr[m] = &pw[m];
    SP pa(a), pb(b), pc(c), pd(d);
    SP p1 = pa + pb, p0 = pc + pd;
    SP q0 = pc * pd, q1;
    SP keep = q0;
    nfl::linear_transform_ntt(q0, q1, &p0, p1, pkptr, pwptr, ks, COUNT, alpha, centered, floor);
    SP z = q0 + pc;
    const S want_z = w0 + c;
    CHECK(same(q0.poly_obj(), w0) && same(q1.poly_obj(), w1), "poly_p: linear_transform_ntt of pending inputs with a pending key polynomial and diagonal");
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of an output's old value keeps it");
    CHECK(same(p1.poly_obj(), c1) && same(p0.poly_obj(), c0) && same(pkey[2][1].poly_obj(), key[2][1]) && same(pw[1].poly_obj(), w[1]),
          "poly_p: the call leaves its inputs, keys and diagonals as they were");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after the call sees the result");
    SP sharer = p1;
    q1 = p1;
    nfl::linear_transform_ntt(q0, q1, static_cast<const SP *>(nullptr), q1, pkptr, pwptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(sharer.poly_obj(), c1) && same(q0.poly_obj(), n0) && same(q1.poly_obj(), n1), "poly_p: an output may be c1, c0 may be NULL; the sharer keeps the input");
  }
  // device_batch against the poly path; the key and weight batches against raw pointers
  std::vector<S> h1(B), h0(B), want0(B), want1(B);
  for (size_t i = 0; i < B; ++i) {
    h1[i] = S(nfl::uniform(100 + i));
    h0[i] = S(nfl::uniform(900 + i));
    nfl::linear_transform_ntt(want0[i], want1[i], &h0[i], h1[i], kptr, wptr, ks, COUNT, alpha, true, false);
  }
  typedef nfl::device_batch<S> BS;
  typedef nfl::device_batch<P> BP;
  BS s0(B, 0), s1(B, 0), bo0(B, 0), bo1(B, 0);
  s0.upload(h0.data());
  s1.upload(h1.data());
  std::vector<std::unique_ptr<BP>> bk(COUNT), bw;
  const BP *pk[COUNT], *pwt[COUNT];
  for (size_t m = 0; m < COUNT; ++m) {
    if (ks[m] != 1) {
      bk[m].reset(new BP(2 * dnum, 0));
      bk[m]->upload(key[m].data());
    }
    bw.emplace_back(new BP(1, 0));
    bw[m]->upload(&w[m]);
    pk[m] = bk[m].get(), pwt[m] = bw[m].get();
  }
  BS::assign_linear_transform(bo0, bo1, &s0, s1, pk, pwt, ks, COUNT, alpha, true, false);
  CHECK(same(polys<S>(bo0), want0) && same(polys<S>(bo1), want1), "device_batch: assign_linear_transform equals the poly path, polynomial by polynomial");
  CHECK(same(polys<S>(s0), h0) && same(polys<S>(s1), h1) && same(polys<P>(*bk[2]), key[2]) && same(polys<P>(*bw[1]), std::vector<P>(1, w[1])),
        "device_batch: the call leaves its sources, keys and diagonals as they were");
  {
    nflhip_ctx *ctx = bw[0]->ctx();
    void *q = bw[0]->queue();
    const size_t ob = B * sizeof(S), kbytes = 2 * dnum * sizeof(P);
    void *r0 = nullptr, *r1 = nullptr, *rk[COUNT] = {nullptr, nullptr, nullptr, nullptr}, *rw[COUNT], *ri0 = nullptr, *ri1 = nullptr;
    bool fine = nflhip_malloc(ctx, &ri0, ob) == 0 && nflhip_malloc(ctx, &ri1, ob) == 0 && nflhip_malloc(ctx, &r0, ob) == 0 && nflhip_malloc(ctx, &r1, ob) == 0;
    fine = fine && nflhip_memcpy_h2d(ctx, ri0, h0[0].cdata(), ob, q) == 0 && nflhip_memcpy_h2d(ctx, ri1, h1[0].cdata(), ob, q) == 0;
    for (size_t m = 0; m < COUNT; ++m) {
      if (ks[m] != 1) fine = fine && nflhip_malloc(ctx, &rk[m], kbytes) == 0 && nflhip_memcpy_h2d(ctx, rk[m], key[m][0].cdata(), kbytes, q) == 0;
      fine = fine && nflhip_malloc(ctx, &rw[m], sizeof(P)) == 0 && nflhip_memcpy_h2d(ctx, rw[m], w[m].cdata(), sizeof(P), q) == 0;
    }
    fine = fine && nflhip_lintrans_ntt_dev(ctx, r0, r1, ri0, ri1, rk, rw, ks, COUNT, B, K, alpha, NFLHIP_LINTRANS_CENTERED, q) == 0;
    std::vector<S> g0(B), g1(B);
    fine = fine && nflhip_memcpy_d2h(ctx, g0[0].data(), r0, ob, q) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), r1, ob, q) == 0 && nflhip_stream_sync(ctx, q) == 0;
    CHECK(fine, "raw pointers: the calls succeed");
    CHECK(same(g0, polys<S>(bo0)) && same(g1, polys<S>(bo1)), "the keys and diagonals used through device_batches equal those used through raw pointers");
    for (size_t m = 0; m < COUNT; ++m) {
      if (rk[m]) nflhip_free(ctx, rk[m]);
      nflhip_free(ctx, rw[m]);
    }
    nflhip_free(ctx, ri0), nflhip_free(ctx, ri1), nflhip_free(ctx, r0), nflhip_free(ctx, r1);
  }
}

int main(int argc, char **argv) {
  try {
    const size_t B = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5;
    if (B == 0) return 2;
    run<uint64_t, 64, 5, 2>(B, 1, "u64/64/5 K=2");
    run<uint64_t, 64, 5, 2>(B, 2, "u64/64/5 K=2");
    run<uint64_t, 1024, 3, 1>(B, 1, "u64/1024/3 K=1");
    run<uint32_t, 128, 4, 1>(B, 2, "u32/128/4 K=1");
    std::printf(g_fail ? "lintrans: FAILED (%d)\n" : "lintrans: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("lintrans: exception: %s\n", e.what());
    return 2;
  }
}
