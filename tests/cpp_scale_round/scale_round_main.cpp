// tests/cpp_scale_round/scale_round_main.cpp -- BFV multiplication of the header surface (include/nfl_hip/poly_p.hpp):
//   * nfl::scale_round / nfl::scale_round_ntt on nfl::poly (host-pointer path) equal the raw entry called with ks and t spelled out;
//     the form, the floor mode and t each change the words;
//   * the same on nfl::poly_p (resident: deferred work pending on the input and on the output's old value; a copy-on-write sharer
//     keeps the old value; work recorded after sees the result);
//   * nfl::bfv_tensor_ntt<KB> / nfl::bfv_square_ntt<KB> on poly and poly_p equal the four steps of the definition written by hand
//     through the existing header calls: embed, base_convert_ntt (centred), tensor_ntt on the extended ring, scale_round_ntt of each
//     component; an output may be an input.
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU) and, on
// the CPU, against tests/cpp/mock plus the toy entries of toy_scale_round.c, tests/cpp_mulrelin, tests/cpp_keyswitch,
// tests/cpp_baseconv_ntt and tests/cpp_baseconv (tests/test_scale_round_cpp.py).
// Usage: scale_round_test.  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }

// the first L rows of `in` embedded in the extended ring, the other rows zero
template <class P, class S> static void embed(P &out, S const &in) {
  std::memset(static_cast<void *>(out.data()), 0, sizeof(typename P::value_type) * P::degree * P::nmoduli);
  std::memcpy(static_cast<void *>(out.data()), in.cdata(), sizeof(typename S::value_type) * S::degree * S::nmoduli);
}

template <class T, size_t D, size_t M, size_t L> static void run(uint64_t t, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, L> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, L> SP;
  std::printf("%s L=%zu t=%llu\n", name, L, (unsigned long long)t);
  P x(nfl::uniform(0x11)), y(nfl::uniform(0x22));
  P in = x + y;
  S sa(nfl::uniform(0x33)), sb(nfl::uniform(0x44));
  // scale_round on poly against the raw entry
  S o, of, on, onf, ot, raw;
  nfl::scale_round(o, in, t);
  CHECK(nflhip_scale_round(P::ctx(), raw.data(), in.cdata(), 1, L, t, 0) == 0 && same(o, raw), "poly: scale_round equals the raw entry with ks = the output's moduli");
  nfl::scale_round(of, in, t, true);
  CHECK(nflhip_scale_round(P::ctx(), raw.data(), in.cdata(), 1, L, t, NFLHIP_SCALE_ROUND_FLOOR) == 0 && same(of, raw), "poly: the floor mode");
  nfl::scale_round_ntt(on, in, t);
  CHECK(nflhip_scale_round_ntt(P::ctx(), raw.data(), in.cdata(), 1, L, t, 0) == 0 && same(on, raw), "poly: scale_round_ntt equals the raw entry");
  nfl::scale_round_ntt(onf, in, t, true);
  CHECK(nflhip_scale_round_ntt(P::ctx(), raw.data(), in.cdata(), 1, L, t, NFLHIP_SCALE_ROUND_FLOOR) == 0 && same(onf, raw), "poly: scale_round_ntt, floor");
  nfl::scale_round(ot, in, t + 2);
  CHECK(!same(o, of) && !same(o, on) && !same(on, onf) && !same(o, ot), "poly: the mode, the form and t each change the words");
  {
    // poly_p: the input and the output's old value pending; a sharer keeps the old value; later work sees the result
    PP px(x), py(y);
    PP pin = px + py;
    SP pa(sa), pb(sb);
    SP po = pa * pb;
    SP keep = po;
    nfl::scale_round(po, pin, t);
    SP z = po + pa;
    CHECK(same(po.poly_obj(), o), "poly_p: scale_round of a pending input equals the poly path");
    CHECK(same(keep.poly_obj(), S(sa * sb)) && same(pin.poly_obj(), in), "poly_p: the sharer of out's old value keeps it; the input stays");
    CHECK(same(z.poly_obj(), S(o + sa)), "poly_p: a sum recorded after scale_round sees the result");
    nfl::scale_round(po, pin, t, true);
    CHECK(same(po.poly_obj(), of), "poly_p: the floor mode");
    nfl::scale_round_ntt(po, pin, t);
    CHECK(same(po.poly_obj(), on), "poly_p: scale_round_ntt equals the poly path");
    nfl::scale_round_ntt(po, pin, t, true);
    CHECK(same(po.poly_obj(), onf), "poly_p: scale_round_ntt, floor");
  }
  // the BFV tensor product against its four steps written by hand
  S a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef)), c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d)), e(nfl::uniform(0xe66));
  S a0 = a + b, a1 = c, b0 = d, b1 = e;
  for (int floor = 0; floor < 2; ++floor) {
    S h[3], q[3];
    {
      P E[4], tn[3];
      const S *ins[4] = {&a0, &a1, &b0, &b1};
      for (int k = 0; k < 4; ++k) {
        embed(E[k], *ins[k]);
        nfl::base_convert_ntt(E[k], 0, L, 0, M, true);
      }
      nfl::tensor_ntt(tn[0], tn[1], tn[2], E[0], E[1], &E[2], &E[3]);
      for (int k = 0; k < 3; ++k) nfl::scale_round_ntt(h[k], tn[k], t, floor != 0);
      nfl::tensor_ntt(tn[0], tn[1], tn[2], E[0], E[1]);
      for (int k = 0; k < 3; ++k) nfl::scale_round_ntt(q[k], tn[k], t, floor != 0);
    }
    CHECK(!same(h[0], h[1]) && !same(h[0], h[2]) && !same(h[1], h[2]) && !same(h[0], q[0]) && !same(h[1], q[1]), "the components differ, the square differs from the product");
    S d0, d1, d2;
    nfl::bfv_tensor_ntt<M - L>(d0, d1, d2, a0, a1, b0, b1, t, floor != 0);
    CHECK(same(d0, h[0]) && same(d1, h[1]) && same(d2, h[2]), "poly: bfv_tensor_ntt equals the four steps written by hand");
    nfl::bfv_square_ntt<M - L>(d0, d1, d2, a0, a1, t, floor != 0);
    CHECK(same(d0, q[0]) && same(d1, q[1]) && same(d2, q[2]), "poly: bfv_square_ntt equals the four steps written by hand");
    S x0(a0), x1(a1);
    nfl::bfv_tensor_ntt<M - L>(x1, d1, x0, x0, x1, b0, b1, t, floor != 0);
    CHECK(same(x1, h[0]) && same(d1, h[1]) && same(x0, h[2]), "poly: the outputs may be the inputs");
    SP pa(a), pb(b), p1(a1), pb0(b0), pb1(b1);
    SP p0 = pa + pb, o0 = pa * pb, o1, o2;
    SP keep = o0;
    nfl::bfv_tensor_ntt<M - L>(o0, o1, o2, p0, p1, pb0, pb1, t, floor != 0);
    SP z = o2 + p1;
    CHECK(same(o0.poly_obj(), h[0]) && same(o1.poly_obj(), h[1]) && same(o2.poly_obj(), h[2]), "poly_p: bfv_tensor_ntt of a pending input");
    CHECK(same(keep.poly_obj(), S(a * b)) && same(p0.poly_obj(), a0) && same(pb1.poly_obj(), b1), "poly_p: the sharer of out0's old value keeps it; the inputs stay");
    CHECK(same(z.poly_obj(), S(h[2] + a1)), "poly_p: a sum recorded after bfv_tensor_ntt sees the result");
    SP sharer = p1;
    nfl::bfv_square_ntt<M - L>(p1, o1, p0, p0, p1, t, floor != 0);
    CHECK(same(p1.poly_obj(), q[0]) && same(o1.poly_obj(), q[1]) && same(p0.poly_obj(), q[2]) && same(sharer.poly_obj(), a1),
          "poly_p: the square over its own inputs; a sharer keeps the input");
  }
}

int main() {
  try {
    run<uint64_t, 64, 5, 2>(65537, "u64/64/5");
    run<uint64_t, 64, 5, 3>(65537, "u64/64/5");
    run<uint32_t, 128, 5, 2>(257, "u32/128/5");
    std::printf(g_fail ? "scale_round: FAILED (%d)\n" : "scale_round: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("scale_round: exception: %s\n", e.what());
    return 2;
  }
}
