// tests/cpp_mulrelin/mulrelin_main.cpp -- ciphertext multiplication of the header surface (include/nfl_hip/poly_p.hpp, batch.hpp):
//   * nfl::tensor_ntt and nfl::mul_relin_ntt / square_relin_ntt on nfl::poly (host-pointer path) equal the sequence written by hand
//     through the existing header calls: three products and a sum for the tensor, nfl::key_switch_ntt on its third component, two
//     additions;
//   * the same on nfl::poly_p (resident: deferred work pending on an input, on a key polynomial and on the output's old value; a
//     copy-on-write sharer keeps the old value; an output may be an input; work recorded after sees the result);
//   * nfl::mul_relin_rescale_ntt: poly, poly_p, device_batch and raw pointers agree (its words are not those of a two-step way);
//   * device_batch::assign_mul_relin: every polynomial equal to the poly path's, and raw pointers (nflhip_mulrelin_ntt_dev on buffers
//     of nflhip_malloc) equal to the batch.
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_mulrelin.c, tests/cpp_keyswitch, tests/cpp_baseconv_ntt and
// tests/cpp_baseconv (tests/test_mulrelin_cpp.py).
// Usage: mulrelin_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <class T, size_t D, size_t M, size_t K> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly<T, D, M - K - 1> R;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  typedef nfl::poly_p<T, D, M - K - 1> RP;
  const size_t L = M - K, dnum = (L + alpha - 1) / alpha;
  std::printf("%s alpha=%zu, %zu digits, %zu polynomials\n", name, alpha, dnum, B);
  std::vector<P> key, ka, kb;
  for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial a sum, so that poly_p can hold it pending
    ka.push_back(P(nfl::uniform(0x100 + t)));
    kb.push_back(P(nfl::uniform(0x200 + t)));
    key.push_back(ka[t] + kb[t]);
  }
  S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d)), e(nfl::uniform(0xe66)), f(nfl::uniform(0xf00));
  S a0 = a + b, a1 = c, b0 = d, b1 = e;  // (not const: a resident handle is made from a poly it may adopt)
  const S cd = c * d;
  // the tensor product against three products and a sum
  const S h0 = a0 * b0, hx = a0 * b1, hy = a1 * b0, h1 = hx + hy, h2 = a1 * b1;
  const S qx = a0 * a1, qy = a1 * a0, q0 = a0 * a0, q1 = qx + qy, q2 = a1 * a1;
  {
    S t0, t1, t2;
    nfl::tensor_ntt(t0, t1, t2, a0, a1, &b0, &b1);
    CHECK(same(t0, h0) && same(t1, h1) && same(t2, h2), "poly: tensor_ntt equals the products written by hand");
    nfl::tensor_ntt(t0, t1, t2, a0, a1);
    CHECK(same(t0, q0) && same(t1, q1) && same(t2, q2), "poly: the square");
    S x0(a0), x1(a1);
    nfl::tensor_ntt(x1, t1, x0, x0, x1, &b0, &b1);
    CHECK(same(x1, h0) && same(t1, h1) && same(x0, h2), "poly: the outputs may be the inputs");
    SP pa(a), pb(b), p1(a1), pb0(b0), pb1(b1);
    SP p0 = pa + pb, o0 = pa * pb, o1, o2;
    SP keep = o0;
    nfl::tensor_ntt(o0, o1, o2, p0, p1, &pb0, &pb1);
    CHECK(same(o0.poly_obj(), h0) && same(o1.poly_obj(), h1) && same(o2.poly_obj(), h2), "poly_p: tensor_ntt of a pending input");
    CHECK(same(keep.poly_obj(), S(a * b)) && same(p0.poly_obj(), a0), "poly_p: the sharer of out0's old value keeps it; the input stays");
    nfl::tensor_ntt(p1, o1, p0, p0, p1);
    CHECK(same(p1.poly_obj(), q0) && same(o1.poly_obj(), q1) && same(p0.poly_obj(), q2), "poly_p: the square over its own inputs");
  }
  for (int mode = 0; mode < 4; ++mode) {
    const bool centered = (mode & 1) != 0, floor = (mode & 2) != 0;
    S k0, k1, o0, o1;
    nfl::key_switch_ntt(k0, k1, h2, key.data(), alpha, centered, floor);
    const S w0 = h0 + k0, w1 = h1 + k1;
    nfl::mul_relin_ntt(o0, o1, a0, a1, b0, b1, key.data(), alpha, centered, floor);
    CHECK(same(o0, w0) && same(o1, w1), "poly: mul_relin_ntt equals tensor, key switch and additions written by hand");
    CHECK(!same(o0, o1), "poly: the two components differ");
    nfl::key_switch_ntt(k0, k1, q2, key.data(), alpha, centered, floor);
    const S s0 = q0 + k0, s1 = q1 + k1;
    nfl::square_relin_ntt(o0, o1, a0, a1, key.data(), alpha, centered, floor);
    CHECK(same(o0, s0) && same(o1, s1), "poly: square_relin_ntt equals the square written by hand");
    S x(b0), y(a1);
    nfl::mul_relin_ntt(x, y, a0, y, x, b1, key.data(), alpha, centered, floor);
    CHECK(same(x, w0) && same(y, w1), "poly: the outputs may be inputs");
    R r0, r1;
    nfl::mul_relin_rescale_ntt(r0, r1, a0, a1, b0, b1, key.data(), alpha, centered, floor);
    CHECK(!same(r0, r1), "poly: the rescaled components differ");
    // poly_p: an input, a key polynomial and the output's old value pending; sharers keep their values
    PP pka(ka[1]), pkb(kb[1]);
    std::vector<PP> pkey;
    for (size_t t = 0; t < 2 * dnum; ++t) pkey.push_back(PP(key[t]));
    pkey[1] = pka + pkb;
    SP pa(a), pb(b), pc(c), pd(d), pe(e);
    SP pa0 = pa + pb;
    SP out0 = pc * pd, out1 = pc + pd;
    SP keep = out0;
    nfl::mul_relin_ntt(out0, out1, pa0, pc, pd, pe, pkey.data(), alpha, centered, floor);
    SP z = out0 + pc;
    const S want_z = w0 + c;
    CHECK(same(out0.poly_obj(), w0) && same(out1.poly_obj(), w1), "poly_p: mul_relin_ntt of a pending input with a pending key polynomial");
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of out0's old value keeps it");
    CHECK(same(pa0.poly_obj(), a0) && same(pkey[1].poly_obj(), key[1]), "poly_p: mul_relin_ntt leaves its inputs and key as they were");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after mul_relin_ntt sees the result");
    SP sharer = pd;
    nfl::mul_relin_ntt(pd, out1, pa0, pc, pd, pe, pkey.data(), alpha, centered, floor);
    CHECK(same(pd.poly_obj(), w0) && same(out1.poly_obj(), w1) && same(sharer.poly_obj(), b0), "poly_p: out0 may be an input; its sharer keeps the input");
    SP sq0, sq1;
    nfl::square_relin_ntt(sq0, sq1, pa0, pc, pkey.data(), alpha, centered, floor);
    CHECK(same(sq0.poly_obj(), s0) && same(sq1.poly_obj(), s1), "poly_p: square_relin_ntt");
    RP pr0, pr1;
    SP pd2(d);
    nfl::mul_relin_rescale_ntt(pr0, pr1, pa0, pc, pd2, pe, pkey.data(), alpha, centered, floor);
    CHECK(same(pr0.poly_obj(), r0) && same(pr1.poly_obj(), r1), "poly_p: mul_relin_rescale_ntt equals the poly path");
  }
  // device_batch against the poly path; raw pointers against the batch
  std::vector<S> h[4], want0(B), want1(B), sq0(B), sq1(B);
  std::vector<R> wr0(B), wr1(B);
  for (int k = 0; k < 4; ++k) h[k].resize(B);
  for (size_t i = 0; i < B; ++i) {
    for (int k = 0; k < 4; ++k) h[k][i] = S(nfl::uniform(100 + 10 * i + k));
    nfl::mul_relin_ntt(want0[i], want1[i], h[0][i], h[1][i], h[2][i], h[3][i], key.data(), alpha, true, false);
    nfl::square_relin_ntt(sq0[i], sq1[i], h[0][i], h[1][i], key.data(), alpha, true, false);
    nfl::mul_relin_rescale_ntt(wr0[i], wr1[i], h[0][i], h[1][i], h[2][i], h[3][i], key.data(), alpha, true, false);
  }
  nfl::device_batch<S> s0(B, 0), s1(B, 0), t0(B, 0), t1(B, 0), o0(B, 0), o1(B, 0);
  nfl::device_batch<R> r0(B, 0), r1(B, 0);
  nfl::device_batch<P> kbatch(2 * dnum, 0);
  s0.upload(h[0].data()), s1.upload(h[1].data()), t0.upload(h[2].data()), t1.upload(h[3].data());
  kbatch.upload(key.data());
  nfl::device_batch<S>::assign_mul_relin(o0, o1, s0, s1, &t0, &t1, kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), want0) && same(polys<S>(o1), want1), "device_batch: assign_mul_relin equals the poly path, polynomial by polynomial");
  nfl::device_batch<S>::assign_mul_relin(r0, r1, s0, s1, &t0, &t1, kbatch, alpha, true, false);
  CHECK(same(polys<R>(r0), wr0) && same(polys<R>(r1), wr1), "device_batch: the rescaled outputs equal the poly path");
  nfl::device_batch<S>::assign_mul_relin(o0, o1, s0, s1, static_cast<const nfl::device_batch<S> *>(nullptr), static_cast<const nfl::device_batch<S> *>(nullptr),
                                         kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), sq0) && same(polys<S>(o1), sq1), "device_batch: the square equals the poly path");
  CHECK(same(polys<S>(s0), h[0]) && same(polys<S>(t1), h[3]) && same(polys<P>(kbatch), key), "device_batch: the inputs and the key stay as they were");
  {
    nflhip_ctx *ctx = kbatch.ctx();
    const size_t ib = B * sizeof(S), ob = B * sizeof(R), kbytes = 2 * dnum * sizeof(P);
    void *q0 = nullptr, *q1 = nullptr, *ri[4] = {nullptr, nullptr, nullptr, nullptr}, *rk = nullptr;
    bool ok = nflhip_malloc(ctx, &q0, ob) == 0 && nflhip_malloc(ctx, &q1, ob) == 0 && nflhip_malloc(ctx, &rk, kbytes) == 0;
    for (int k = 0; k < 4; ++k) ok = ok && nflhip_malloc(ctx, &ri[k], ib) == 0 && nflhip_memcpy_h2d(ctx, ri[k], h[k][0].cdata(), ib, kbatch.queue()) == 0;
    ok = ok && nflhip_memcpy_h2d(ctx, rk, key[0].cdata(), kbytes, kbatch.queue()) == 0;
    ok = ok && nflhip_mulrelin_ntt_dev(ctx, q0, q1, ri[0], ri[1], ri[2], ri[3], rk, B, K, alpha, NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_RESCALE,
                                       kbatch.queue()) == 0;
    std::vector<R> g0(B), g1(B);
    ok = ok && nflhip_memcpy_d2h(ctx, g0[0].data(), q0, ob, kbatch.queue()) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), q1, ob, kbatch.queue()) == 0;
    ok = ok && nflhip_stream_sync(ctx, kbatch.queue()) == 0;
    CHECK(ok, "raw pointers: the calls succeed");
    CHECK(same(g0, polys<R>(r0)) && same(g1, polys<R>(r1)), "the rescaled product through a device_batch equals the one through raw pointers");
    nflhip_free(ctx, q0), nflhip_free(ctx, q1), nflhip_free(ctx, rk);
    for (int k = 0; k < 4; ++k) nflhip_free(ctx, ri[k]);
  }
  (void)f;
}

int main(int argc, char **argv) {
  try {
    const size_t B = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5;
    if (B == 0) return 2;
    run<uint64_t, 64, 5, 2>(B, 1, "u64/64/5 K=2");
    run<uint64_t, 64, 5, 2>(B, 2, "u64/64/5 K=2");
    run<uint64_t, 1024, 4, 1>(B, 1, "u64/1024/4 K=1");
    run<uint32_t, 128, 4, 1>(B, 2, "u32/128/4 K=1");
    std::printf(g_fail ? "mulrelin: FAILED (%d)\n" : "mulrelin: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("mulrelin: exception: %s\n", e.what());
    return 2;
  }
}
