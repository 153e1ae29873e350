// tests/cpp_rotate/rotate_main.cpp -- hoisted rotations of the header surface (include/nfl_hip/poly_p.hpp, batch.hpp):
//   * nfl::rotate_hoisted_ntt on nfl::poly (host-pointer path) equals the definition written by hand through the existing header
//     calls: per rotation nfl::key_switch_ntt of c1, + c0, nfl::automorphism_ntt of both results; with and without c0; an output may
//     be c0 or c1;
//   * nfl::rotate_hoisted_ntt on nfl::poly_p (resident: deferred work pending on c0, c1, a key polynomial and an output's old value; a
//     copy-on-write sharer keeps the old value; work recorded after sees the result);
//   * device_batch::assign_rotations: every polynomial equal to the poly path's, and the keys used through device_batches equal to
//     the keys used through raw pointers (nflhip_rotate_hoisted_ntt_dev on buffers of nflhip_malloc).
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_rotate.c, tests/cpp_keyswitch, tests/cpp_baseconv_ntt and
// tests/cpp_baseconv (tests/test_rotate_cpu.py).
// Usage: rotate_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
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

static const size_t COUNT = 3;

template <class T, size_t D, size_t M, size_t K> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  const size_t L = M - K, dnum = (L + alpha - 1) / alpha;
  std::printf("%s alpha=%zu, %zu digits, %zu rotations, %zu polynomials\n", name, alpha, dnum, COUNT, B);
  const uint64_t ks[COUNT] = {5, 2 * D - 1, 5};  // a repeated k, with another key
  std::vector<std::vector<P>> key(COUNT), ka(COUNT), kb(COUNT);
  const P *kptr[COUNT];
  for (size_t m = 0; m < COUNT; ++m) {
    for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial a sum, so that poly_p can hold it pending
      ka[m].push_back(P(nfl::uniform(0x100 + 64 * m + t)));
      kb[m].push_back(P(nfl::uniform(0x200 + 64 * m + t)));
      key[m].push_back(ka[m][t] + kb[m][t]);
    }
    kptr[m] = key[m].data();
  }
  S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  const S c1 = a + b, c0 = c + d, cd = c * d;
  for (int mode = 0; mode < 4; ++mode) {
    const bool centered = (mode & 1) != 0, floor = (mode & 2) != 0;
    // the definition, by hand through the existing header calls
    std::vector<S> w0(COUNT), w1(COUNT), n0(COUNT);
    for (size_t m = 0; m < COUNT; ++m) {
      S d0, d1;
      nfl::key_switch_ntt(d0, d1, c1, kptr[m], alpha, centered, floor);
      const S y0 = d0 + c0;
      nfl::automorphism_ntt(w0[m], y0, ks[m]);
      nfl::automorphism_ntt(w1[m], d1, ks[m]);
      nfl::automorphism_ntt(n0[m], d0, ks[m]);
    }
    std::vector<S> o0(COUNT), o1(COUNT);
    nfl::rotate_hoisted_ntt(o0.data(), o1.data(), &c0, c1, kptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(o0, w0) && same(o1, w1), "poly: rotate_hoisted_ntt equals the definition written by hand");
    CHECK(!same(o0[0], o0[2]) && !same(o0[0], o1[0]), "poly: two keys for one k give different results; the components differ");
    nfl::rotate_hoisted_ntt(o0.data(), o1.data(), static_cast<const S *>(nullptr), c1, kptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(o0, n0) && same(o1, w1), "poly: without c0 the first component is the key switch's, permuted");
    std::vector<S> x0(COUNT), x1(COUNT);
    x0[1] = c0, x1[2] = c1;
    nfl::rotate_hoisted_ntt(x0.data(), x1.data(), &x0[1], x1[2], kptr, ks, COUNT, alpha, centered, floor);
    CHECK(same(x0, w0) && same(x1, w1), "poly: an output may be c0 or c1");
    // poly_p: c0, c1, a key polynomial and an output's old value pending; sharers keep their values
    std::vector<std::vector<PP>> pkey(COUNT);
    const PP *pkptr[COUNT];
    PP pka(ka[1][1]), pkb(kb[1][1]);
    for (size_t m = 0; m < COUNT; ++m) {
      for (size_t t = 0; t < 2 * dnum; ++t) pkey[m].push_back(PP(key[m][t]));
      pkptr[m] = pkey[m].data();
    }
    pkey[1][1] = pka + pkb;
    SP pa(a), pb(b), pc(c), pd(d);
    SP p1 = pa + pb, p0 = pc + pd;
    std::vector<SP> q0(COUNT), q1(COUNT);
    q0[0] = pc * pd;
    SP keep = q0[0];
    nfl::rotate_hoisted_ntt(q0.data(), q1.data(), &p0, p1, pkptr, ks, COUNT, alpha, centered, floor);
    SP z = q0[2] + pc;
    const S want_z = w0[2] + c;
    bool ok = true;
    for (size_t m = 0; m < COUNT; ++m) ok = ok && same(q0[m].poly_obj(), w0[m]) && same(q1[m].poly_obj(), w1[m]);
    CHECK(ok, "poly_p: rotate_hoisted_ntt of pending inputs with a pending key polynomial");
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of an output's old value keeps it");
    CHECK(same(p1.poly_obj(), c1) && same(p0.poly_obj(), c0) && same(pkey[1][1].poly_obj(), key[1][1]), "poly_p: the call leaves its inputs and keys as they were");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after the call sees the result");
    SP sharer = p1;
    q1[1] = p1;
    nfl::rotate_hoisted_ntt(q0.data(), q1.data(), static_cast<const SP *>(nullptr), q1[1], pkptr, ks, COUNT, alpha, centered, floor);
    ok = same(sharer.poly_obj(), c1);
    for (size_t m = 0; m < COUNT; ++m) ok = ok && same(q0[m].poly_obj(), n0[m]) && same(q1[m].poly_obj(), w1[m]);
    CHECK(ok, "poly_p: an output may be c1, c0 may be NULL; the sharer keeps the input");
  }
  // device_batch against the poly path; the key batches against raw pointers
  std::vector<S> h1(B), h0(B);
  std::vector<std::vector<S>> want0(COUNT, std::vector<S>(B)), want1(COUNT, std::vector<S>(B));
  for (size_t i = 0; i < B; ++i) {
    h1[i] = S(nfl::uniform(100 + i));
    h0[i] = S(nfl::uniform(900 + i));
    S t0[COUNT], t1[COUNT];
    nfl::rotate_hoisted_ntt(t0, t1, &h0[i], h1[i], kptr, ks, COUNT, alpha, true, false);
    for (size_t m = 0; m < COUNT; ++m) want0[m][i] = t0[m], want1[m][i] = t1[m];
  }
  typedef nfl::device_batch<S> BS;
  typedef nfl::device_batch<P> BP;
  BS s0(B, 0), s1(B, 0);
  s0.upload(h0.data());
  s1.upload(h1.data());
  std::vector<std::unique_ptr<BS>> bo0, bo1;
  std::vector<std::unique_ptr<BP>> bk;
  BS *po0[COUNT], *po1[COUNT];
  const BP *pk[COUNT];
  for (size_t m = 0; m < COUNT; ++m) {
    bo0.emplace_back(new BS(B, 0));
    bo1.emplace_back(new BS(B, 0));
    bk.emplace_back(new BP(2 * dnum, 0));
    bk[m]->upload(key[m].data());
    po0[m] = bo0[m].get(), po1[m] = bo1[m].get(), pk[m] = bk[m].get();
  }
  BS::assign_rotations(po0, po1, &s0, s1, pk, ks, COUNT, alpha, true, false);
  bool ok = true;
  for (size_t m = 0; m < COUNT; ++m) ok = ok && same(polys<S>(*bo0[m]), want0[m]) && same(polys<S>(*bo1[m]), want1[m]);
  CHECK(ok, "device_batch: assign_rotations equals the poly path, polynomial by polynomial");
  CHECK(same(polys<S>(s0), h0) && same(polys<S>(s1), h1) && same(polys<P>(*bk[1]), key[1]), "device_batch: the call leaves its sources and keys as they were");
  {
    nflhip_ctx *ctx = bk[0]->ctx();
    void *q = bk[0]->queue();
    const size_t ob = B * sizeof(S), kbytes = 2 * dnum * sizeof(P);
    void *r0[COUNT], *r1[COUNT], *rk[COUNT], *ri0 = nullptr, *ri1 = nullptr;
    bool fine = nflhip_malloc(ctx, &ri0, ob) == 0 && nflhip_malloc(ctx, &ri1, ob) == 0;
    fine = fine && nflhip_memcpy_h2d(ctx, ri0, h0[0].cdata(), ob, q) == 0 && nflhip_memcpy_h2d(ctx, ri1, h1[0].cdata(), ob, q) == 0;
    for (size_t m = 0; m < COUNT; ++m) {
      fine = fine && nflhip_malloc(ctx, &r0[m], ob) == 0 && nflhip_malloc(ctx, &r1[m], ob) == 0 && nflhip_malloc(ctx, &rk[m], kbytes) == 0;
      fine = fine && nflhip_memcpy_h2d(ctx, rk[m], key[m][0].cdata(), kbytes, q) == 0;
    }
    fine = fine && nflhip_rotate_hoisted_ntt_dev(ctx, r0, r1, ri0, ri1, rk, ks, COUNT, B, K, alpha, NFLHIP_ROTATE_CENTERED, q) == 0;
    bool eq = true;
    for (size_t m = 0; m < COUNT && fine; ++m) {
      std::vector<S> g0(B), g1(B);
      fine = nflhip_memcpy_d2h(ctx, g0[0].data(), r0[m], ob, q) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), r1[m], ob, q) == 0 && nflhip_stream_sync(ctx, q) == 0;
      eq = eq && same(g0, polys<S>(*bo0[m])) && same(g1, polys<S>(*bo1[m]));
    }
    CHECK(fine, "raw pointers: the calls succeed");
    CHECK(eq, "the keys used through device_batches equal the keys used through raw pointers");
    for (size_t m = 0; m < COUNT; ++m) nflhip_free(ctx, r0[m]), nflhip_free(ctx, r1[m]), nflhip_free(ctx, rk[m]);
    nflhip_free(ctx, ri0), nflhip_free(ctx, ri1);
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
    std::printf(g_fail ? "rotate: FAILED (%d)\n" : "rotate: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("rotate: exception: %s\n", e.what());
    return 2;
  }
}
