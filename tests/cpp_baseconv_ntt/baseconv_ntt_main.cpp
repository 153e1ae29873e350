// tests/cpp_baseconv_ntt/baseconv_ntt_main.cpp -- the NTT-form base conversion and mod-down of the header surface
// (include/nfl_hip/poly_p.hpp, batch.hpp):
//   * nfl::base_convert_ntt / nfl::mod_down_ntt on nfl::poly (host-pointer path) and nfl::poly_p (resident: deferred work pending
//     before the call, a copy-on-write sharer keeps the old value, work recorded after sees the new one),
//   * device_batch / sharded_batch::assign_base_convert and assign_mod_down with ntt_form = true: every polynomial equal to the poly
//     path's, the sharded batch over SEVERAL shards equal to one device_batch (batches that do not divide, empty shards),
//   * the default ntt_form = false reaches the coefficient-form entries.
// Every check is an equality between two surfaces over the same entries, so the program runs against the real library (GPU; with
// "real" as the third argument it also checks inv(base_convert_ntt(fwd(x))) == base_convert(x) and the mod-down's counterpart) and,
// on the CPU, against tests/cpp/mock with NFLHIP_MOCK_DEVICES virtual devices plus the toy entries of toy_baseconv_ntt.c and
// tests/cpp_baseconv/toy_baseconv.c (tests/test_baseconv_ntt_cpu.py).
// Usage: baseconv_ntt_test <device list, e.g. 0,1,2 or 0,0,0> [batch] [real].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

template <class T, size_t D, size_t M, size_t K> static void run(const std::vector<int> &devs, size_t B, bool real, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  typedef nfl::poly_p<T, D, M> PP;
  typedef nfl::poly_p<T, D, M - K> SP;
  std::printf("%s, %zu polynomials over %zu shards\n", name, B, devs.size());
  const size_t s0 = M - K, ks = K;
  P a(nfl::uniform(0x5eed)), b(nfl::uniform(0xbeef));
  S c(nfl::uniform(0xc0de)), d(nfl::uniform(0xd00d));
  for (int mode = 0; mode < 2; ++mode) {  // centred / floor off and on
    // poly: the host-pointer entries define the words every other surface is compared with
    P s = a + b, up(s), coeff(s);
    nfl::base_convert_ntt(up, s0, ks, 0, M, mode != 0);
    nfl::base_convert(coeff, s0, ks, 0, M, mode != 0);
    CHECK(!same(up, s), "poly: base_convert_ntt changes the destination rows");
    S down, down_coeff;
    nfl::mod_down_ntt(down, s, mode != 0);
    nfl::mod_down(down_coeff, s, mode != 0);
    if (!real) CHECK(!same(up, coeff) && !same(down, down_coeff), "the NTT-form functions reach entries of their own");
    // poly_p: a pending sum converted in place; the sharer keeps the old value; work recorded after sees the new one
    PP pa(a), pb(b);
    SP pc(c), pd(d);
    PP v = pa + pb;
    PP sharer = v;
    nfl::base_convert_ntt(v, s0, ks, 0, M, mode != 0);
    PP after = v + pb;
    P want_after = up + b;
    CHECK(same(v.poly_obj(), up), "poly_p: base_convert_ntt of a pending sum, in place");
    CHECK(same(sharer.poly_obj(), s), "poly_p: the copy-on-write sharer keeps its value across base_convert_ntt");
    CHECK(same(after.poly_obj(), want_after), "poly_p: a sum recorded after base_convert_ntt sees the converted value");
    PP x = pa + pb;       // pending on the input side
    SP y = pc + pd;       // pending on the output side
    SP out = pc * pd;     // the old value of the output handle, pending too, shared with `keep`
    SP keep = out;
    nfl::mod_down_ntt(out, x, mode != 0);
    SP z = out + y;       // recorded after, on the output side
    S cd = c * d, u = c + d, want_z = down + u;
    CHECK(same(out.poly_obj(), down), "poly_p: mod_down_ntt of a pending sum");
    CHECK(same(keep.poly_obj(), cd), "poly_p: the sharer of the output's old value keeps it");
    CHECK(same(z.poly_obj(), want_z), "poly_p: a sum recorded after mod_down_ntt sees the result");
    CHECK(same(x.poly_obj(), s), "poly_p: mod_down_ntt leaves its input as it was");
  }
  // device_batch against the poly path, sharded_batch against device_batch
  std::vector<P> h(B), want_up(B), want_from(B), fill(B);
  std::vector<S> want_down(B);
  for (size_t i = 0; i < B; ++i) {
    h[i] = P(nfl::uniform(100 + i));
    fill[i] = P(nfl::uniform(900 + i));
    want_up[i] = h[i];
    nfl::base_convert_ntt(want_up[i], s0, ks, 0, M, true);
    nfl::mod_down_ntt(want_down[i], h[i]);
    // from another batch, D = the first M - K rows: rows D converted, the other rows keep the destination's words
    P t(h[i]);
    nfl::base_convert_ntt(t, s0, ks, 0, M - K);
    want_from[i] = fill[i];
    for (size_t j = 0; j < M - K; ++j)
      for (size_t q = 0; q < D; ++q) want_from[i](j, q) = t(j, q);
  }
  const int dev0 = devs[0];
  nfl::device_batch<P> src1(B, dev0), up1(B, dev0);
  nfl::device_batch<S> dst1(B, dev0);
  nfl::sharded_batch<P> src(B, devs), up(B, devs);
  nfl::sharded_batch<S> dst(B, devs);
  if (B) {
    src1.upload(h.data());
    src.upload(h.data());
  }
  CHECK(src.shards() == devs.size() && dst.shards() == devs.size(), "one shard per entry of the device list");
  dst1.assign_mod_down(src1, false, true);
  dst.assign_mod_down(src, false, true);
  CHECK(same(polys<S>(dst1), want_down), "device_batch: assign_mod_down, NTT form");
  CHECK(same(polys<S>(dst), want_down), "sharded_batch: assign_mod_down, NTT form, shard by shard");
  CHECK(same(polys<P>(src), h) && same(polys<P>(src1), h), "the mod-down leaves its source as it was");
  if (B) {
    up1.upload(h.data());
    up.upload(h.data());
  }
  up1.assign_base_convert(up1, s0, ks, 0, M, true, true);   // in place, the mod-up
  up.assign_base_convert(up, s0, ks, 0, M, true, true);
  CHECK(same(polys<P>(up1), want_up), "device_batch: assign_base_convert in place, NTT form");
  CHECK(same(polys<P>(up), want_up), "sharded_batch: assign_base_convert in place, NTT form");
  if (B) {
    up1.upload(fill.data());
    up.upload(fill.data());
  }
  up1.assign_base_convert(src1, s0, ks, 0, M - K, false, true);   // from another batch: the rows outside D keep their words
  up.assign_base_convert(src, s0, ks, 0, M - K, false, true);
  CHECK(same(polys<P>(up1), want_from), "device_batch: assign_base_convert from another batch, NTT form");
  CHECK(same(polys<P>(up), want_from), "sharded_batch: assign_base_convert from another batch, NTT form");
  {  // the trailing argument's default is the coefficient form
    nfl::device_batch<P> e1(B, dev0), e2(B, dev0);
    nfl::device_batch<S> f1(B, dev0), f2(B, dev0);
    nfl::sharded_batch<P> e3(B, devs);
    nfl::sharded_batch<S> f3(B, devs);
    if (B) {
      e1.upload(h.data());
      e2.upload(h.data());
      e3.upload(h.data());
    }
    e1.assign_base_convert(e1, s0, ks, 0, M, true);
    e2.assign_base_convert(e2, s0, ks, 0, M, true, false);
    e3.assign_base_convert(e3, s0, ks, 0, M, true);
    f1.assign_mod_down(src1);
    f2.assign_mod_down(src1, false, false);
    f3.assign_mod_down(src);
    std::vector<P> wc(h);
    std::vector<S> wd(B);
    for (size_t i = 0; i < B; ++i) {
      nfl::base_convert(wc[i], s0, ks, 0, M, true);
      nfl::mod_down(wd[i], h[i]);
    }
    CHECK(same(polys<P>(e1), polys<P>(e2)) && same(polys<P>(e1), polys<P>(e3)) && same(polys<P>(e1), wc), "assign_base_convert: ntt_form defaults to the coefficient-form entry");
    CHECK(same(polys<S>(f1), polys<S>(f2)) && same(polys<S>(f1), polys<S>(f3)) && same(polys<S>(f1), wd), "assign_mod_down: ntt_form defaults to the coefficient-form entry");
    if (B && !real) CHECK(!same(polys<P>(e1), want_up) && !same(polys<S>(f1), want_down), "the two forms are different entries");
    if (real && B) {  // real arithmetic: the NTT-form entries between the transforms are the coefficient-form entries
      nfl::device_batch<P> g(B, dev0);
      nfl::device_batch<S> gd(B, dev0);
      g.upload(h.data());
      g.ntt_pow_phi();
      gd.assign_mod_down(g, false, true);
      gd.invntt_pow_invphi();
      CHECK(same(polys<S>(gd), wd), "inv(mod_down_ntt(fwd(x))) == mod_down(x)");
      g.assign_base_convert(g, s0, ks, 0, M, true, true);
      g.invntt_pow_invphi();
      CHECK(same(polys<P>(g), wc), "inv(base_convert_ntt(fwd(x))) == base_convert(x)");
    }
  }
}

int main(int argc, char **argv) {
  try {
    std::vector<int> devs;
    const std::string list = argc > 1 ? argv[1] : "0";
    for (size_t pos = 0; pos <= list.size();) {
      const size_t end = list.find(',', pos) == std::string::npos ? list.size() : list.find(',', pos);
      devs.push_back(std::atoi(list.substr(pos, end - pos).c_str()));
      pos = end + 1;
    }
    const size_t B = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 5;
    const bool real = argc > 3 && std::strcmp(argv[3], "real") == 0;
    run<uint64_t, 64, 4, 2>(devs, B, real, "u64/64/4 k=2");
    run<uint64_t, 1024, 2, 1>(devs, B, real, "u64/1024/2 k=1");
    run<uint32_t, 128, 3, 2>(devs, B, real, "u32/128/3 k=2");
    std::printf(g_fail ? "baseconv_ntt: FAILED (%d)\n" : "baseconv_ntt: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("baseconv_ntt: exception: %s\n", e.what());
    return 2;
  }
}
