// tests/cpp_keyswitch/keyswitch_main.cpp -- the hybrid key switch of the header surface (include/nfl_hip/poly_p.hpp, batch.hpp):
//   * nfl::key_switch_ntt on nfl::poly (host-pointer path) equals the sequence written by hand through the existing header calls:
//     the input embedded into the key's ring, nfl::base_convert_ntt per digit, nfl::dot per component, nfl::mod_down_ntt;
//   * nfl::key_switch_ntt on nfl::poly_p (resident: deferred work pending on the input, on a key polynomial and on the output's old
//     value; a copy-on-write sharer keeps the old value; an output may be the input; work recorded after sees the result);
//   * device_batch::assign_key_switch: every polynomial equal to the poly path's, and the key used through a device_batch equal to
//     the key used through raw pointers (nflhip_keyswitch_ntt_dev on buffers of nflhip_malloc).
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_keyswitch.c, tests/cpp_baseconv_ntt and tests/cpp_baseconv
// (tests/test_keyswitch_cpu.py).
// Usage: keyswitch_test [batch].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
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

// the definition, by hand through the existing header calls
template <class T, size_t D, size_t M, size_t K>
static void by_hand(nfl::poly<T, D, M - K> &o0, nfl::poly<T, D, M - K> &o1, nfl::poly<T, D, M - K> const &in, std::vector<nfl::poly<T, D, M>> const &key,
                    size_t alpha, bool centered, bool floor) {
  typedef nfl::poly<T, D, M> P;
  const size_t L = M - K, dnum = (L + alpha - 1) / alpha;
  P X(nfl::uniform(1));
  for (size_t j = 0; j < M; ++j)
    for (size_t q = 0; q < D; ++q) X(j, q) = j < L ? in(j, q) : 0;
  std::vector<P> U(dnum, X), kc(dnum, X);
  for (size_t d = 0; d < dnum; ++d) nfl::base_convert_ntt(U[d], d * alpha, L - d * alpha < alpha ? L - d * alpha : alpha, 0, M, centered);
  for (int c = 0; c < 2; ++c) {
    for (size_t d = 0; d < dnum; ++d) kc[d] = key[2 * d + c];
    P acc(nfl::uniform(2));
    nfl::dot(acc, U.data(), kc.data(), dnum);
    nfl::mod_down_ntt(c ? o1 : o0, acc, floor);
  }
}

template <class T, size_t D, size_t M, size_t K> static void run(size_t B, size_t alpha, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  const size_t L = M - K, dnum = (L + alpha - 1) / alpha;
  std::printf("%s alpha=%zu, %zu digits, %zu polynomials\n", name, alpha, dnum, B);
  std::vector<P> key, ka, kb;
  for (size_t t = 0; t < 2 * dnum; ++t) {  // every key polynomial a sum, so that poly_p can hold it pending
    ka.push_back(P(nfl::uniform(0x100 + t)));
    kb.push_back(P(nfl::uniform(0x200 + t)));
    key.push_back(ka[t] + kb[t]);
  }
  S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  const S in = a + b, cd = c * d;
  for (int mode = 0; mode < 4; ++mode) {
    const bool centered = (mode & 1) != 0, floor = (mode & 2) != 0;
    S w0, w1, o0, o1;
    by_hand<T, D, M, K>(w0, w1, in, key, alpha, centered, floor);
    nfl::key_switch_ntt(o0, o1, in, key.data(), alpha, centered, floor);
    CHECK(same(o0, w0) && same(o1, w1), "poly: key_switch_ntt equals the sequence written by hand");
    CHECK(!same(o0, o1), "poly: the two components differ");
    S x(in), y1;
    nfl::key_switch_ntt(x, y1, x, key.data(), alpha, centered, floor);
    CHECK(same(x, w0) && same(y1, w1), "poly: out0 may be the input");
    // poly_p: the input, a key polynomial and the output's old value pending; sharers keep their values
    PP pka(ka[1]), pkb(kb[1]);
    std::vector<PP> pkey;
    for (size_t t = 0; t < 2 * dnum; ++t) pkey.push_back(PP(key[t]));
    pkey[1] = pka + pkb;
    SP pa(a), pb(b), pc(c), pd(d);
    SP pin = pa + pb;
    SP out0 = pc * pd, out1 = pc + pd;
    SP keep = out0;
    nfl::key_switch_ntt(out0, out1, pin, pkey.data(), alpha, centered, floor);
    SP z = out0 + pc;
    S want_z = w0 + c;
    CHECK(same(out0.poly_obj(), w0) && same(out1.poly_obj(), w1), "poly_p: key_switch_ntt of a pending input with a pending key polynomial");
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of out0's old value keeps it");
    CHECK(same(pin.poly_obj(), in) && same(pkey[1].poly_obj(), key[1]), "poly_p: key_switch_ntt leaves its input and key as they were");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after key_switch_ntt sees the result");
    SP sharer = pin;
    nfl::key_switch_ntt(pin, out1, pin, pkey.data(), alpha, centered, floor);
    CHECK(same(pin.poly_obj(), w0) && same(out1.poly_obj(), w1) && same(sharer.poly_obj(), in), "poly_p: out0 may be the input; its sharer keeps the input");
  }
  // device_batch against the poly path; the key batch against raw pointers
  std::vector<S> h(B), want0(B), want1(B);
  for (size_t i = 0; i < B; ++i) {
    h[i] = S(nfl::uniform(100 + i));
    nfl::key_switch_ntt(want0[i], want1[i], h[i], key.data(), alpha, true, false);
  }
  nfl::device_batch<S> src(B, 0), o0(B, 0), o1(B, 0);
  nfl::device_batch<P> kbatch(2 * dnum, 0);
  src.upload(h.data());
  kbatch.upload(key.data());
  nfl::device_batch<S>::assign_key_switch(o0, o1, src, kbatch, alpha, true, false);
  CHECK(same(polys<S>(o0), want0) && same(polys<S>(o1), want1), "device_batch: assign_key_switch equals the poly path, polynomial by polynomial");
  CHECK(same(polys<S>(src), h) && same(polys<P>(kbatch), key), "device_batch: the key switch leaves its source and key as they were");
  {
    nflhip_ctx *ctx = kbatch.ctx();
    const size_t ob = B * sizeof(S), kbytes = 2 * dnum * sizeof(P);
    void *r0 = nullptr, *r1 = nullptr, *ri = nullptr, *rk = nullptr;
    bool ok = nflhip_malloc(ctx, &r0, ob) == 0 && nflhip_malloc(ctx, &r1, ob) == 0 && nflhip_malloc(ctx, &ri, ob) == 0 && nflhip_malloc(ctx, &rk, kbytes) == 0;
    ok = ok && nflhip_memcpy_h2d(ctx, ri, h[0].cdata(), ob, kbatch.queue()) == 0 && nflhip_memcpy_h2d(ctx, rk, key[0].cdata(), kbytes, kbatch.queue()) == 0;
    ok = ok && nflhip_keyswitch_ntt_dev(ctx, r0, r1, ri, rk, B, K, alpha, NFLHIP_KEYSWITCH_CENTERED, kbatch.queue()) == 0;
    std::vector<S> g0(B), g1(B);
    ok = ok && nflhip_memcpy_d2h(ctx, g0[0].data(), r0, ob, kbatch.queue()) == 0 && nflhip_memcpy_d2h(ctx, g1[0].data(), r1, ob, kbatch.queue()) == 0;
    ok = ok && nflhip_stream_sync(ctx, kbatch.queue()) == 0;
    CHECK(ok, "raw pointers: the calls succeed");
    CHECK(same(g0, polys<S>(o0)) && same(g1, polys<S>(o1)), "the key used through a device_batch equals the key used through raw pointers");
    nflhip_free(ctx, r0), nflhip_free(ctx, r1), nflhip_free(ctx, ri), nflhip_free(ctx, rk);
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
    std::printf(g_fail ? "keyswitch: FAILED (%d)\n" : "keyswitch: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("keyswitch: exception: %s\n", e.what());
    return 2;
  }
}
