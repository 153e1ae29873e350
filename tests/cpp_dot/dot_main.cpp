// tests/cpp_dot/dot_main.cpp -- sums of products across polynomials on the header surface (include/nfl_hip/nfl.hpp):
//   * nfl::dot / nfl::dot_add on nfl::poly (the staged host entry) and on nfl::poly_p (resident: the pointer form in chunks of
//     16 terms chained through the addend, with deferred operations pending before the call and recorded after it),
//   * device_batch::assign_dot and device_batch::assign_matvec,
// every result against a host restatement in 128-bit integers.  Second translation unit: dot_tu2.cpp.
// Usage: dot_test [eager].  Exit 0 = all checks passed, 1 = a mismatch, 2 = an exception (no GPU: the library's "no CPU
// fallback" error).
#include <nfl.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

int other_tu_dot();

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

typedef unsigned __int128 u128;
// out = (add ? *add : 0) + sum_j a[j] * b[j]
template <class P> static void host_dot(P &out, const P *a, const P *b, size_t terms, const P *add) {
  typedef typename P::value_type T;
  for (size_t cm = 0; cm < P::nmoduli; ++cm) {
    const uint64_t p = P::get_modulus(cm);
    for (size_t i = 0; i < P::degree; ++i) {
      u128 s = add ? uint64_t((*add)(cm, i)) : 0;
      for (size_t j = 0; j < terms; ++j) s = (s + u128(uint64_t(a[j](cm, i))) * uint64_t(b[j](cm, i))) % p;
      out(cm, i) = T(uint64_t(s));
    }
  }
}
template <class P> static bool same(P const &a, P const &b) { return std::memcmp(a.cdata(), b.cdata(), sizeof(typename P::value_type) * P::degree * P::nmoduli) == 0; }

template <class T, size_t D, size_t M> static void run(const char *name, size_t terms) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly_p<T, D, M> PP;
  std::printf("%s, %u terms\n", name, unsigned(terms));
  std::vector<P> a(terms), b(terms);
  for (size_t j = 0; j < terms; ++j) {
    a[j] = P(nfl::uniform(0x100 + j));
    b[j] = P(nfl::uniform(0x200 + j));
  }
  for (size_t cm = 0; cm < M; ++cm)  // the largest products in one term
    for (size_t i = 0; i < D; ++i) a[0](cm, i) = b[0](cm, i) = T(P::get_modulus(cm) - 1);
  P c(nfl::uniform(0xc0de)), want, want_add, got;
  host_dot(want, a.data(), b.data(), terms, static_cast<const P *>(nullptr));
  host_dot(want_add, a.data(), b.data(), terms, &c);
  {  // poly
    nfl::dot(got, a.data(), b.data(), terms);
    CHECK(same(got, want), "poly: dot");
    got = c;
    nfl::dot_add(got, a.data(), b.data(), terms);
    CHECK(same(got, want_add), "poly: dot_add");
    std::vector<P> a2(a);
    nfl::dot(a2[0], a2.data(), b.data(), terms);
    CHECK(same(a2[0], want), "poly: the output is one of the inputs");
  }
  for (int round = 0; round < 2; ++round) {  // poly_p: deferred work pending before, more recorded after
    std::vector<PP> pa, pb;
    for (size_t j = 0; j < terms; ++j) {
      pa.push_back(PP(a[j]));
      pb.push_back(PP(b[j]));
    }
    PP pc(c);
    P s = a[terms - 1] + c;
    std::vector<P> as(a);
    as[terms - 1] = s;
    P want_s, want_after;
    host_dot(want_s, as.data(), b.data(), terms, static_cast<const P *>(nullptr));
    pa[terms - 1] = pa[terms - 1] + pc;     // pending: the last term of a is a deferred sum
    PP out = pc * pb[0];                    // the old value of the output handle, pending too, shared with `keep`
    PP keep = out;
    nfl::dot(out, pa.data(), pb.data(), terms);   // the queue runs, then the launches
    PP z = out * pc;                        // recorded after: reads the result
    want_after = want_s * c;
    CHECK(same(out.poly_obj(), want_s), "poly_p: dot with a pending term");
    CHECK(same(z.poly_obj(), want_after), "poly_p: a product recorded after the call sees the result");
    P cb = c * b[0];
    CHECK(same(keep.poly_obj(), cb), "poly_p: the sharer of the output's old value keeps it");
    PP acc = pc + pc;                       // pending addend
    P c2 = c + c, want_acc;
    host_dot(want_acc, as.data(), b.data(), terms, &c2);
    nfl::dot_add(acc, pa.data(), pb.data(), terms);
    CHECK(same(acc.poly_obj(), want_acc), "poly_p: dot_add onto a pending sum");
    nfl::dot(pa[0], pa.data(), pb.data(), terms);
    CHECK(same(pa[0].poly_obj(), want_s), "poly_p: the output is one of the inputs");
  }
  {  // device_batch
    const size_t G = 5;
    std::vector<P> ha(G * terms), hb(G * terms), w(G), want_d(G), want_m(G);
    for (size_t k = 0; k < G * terms; ++k) {
      ha[k] = P(nfl::uniform(0x300 + k));
      hb[k] = P(nfl::uniform(0x400 + k));
    }
    for (size_t g = 0; g < G; ++g) {
      host_dot(want_d[g], &ha[g * terms], &hb[g * terms], terms, static_cast<const P *>(nullptr));
      host_dot(want_m[g], &ha[g * terms], &hb[0], terms, static_cast<const P *>(nullptr));
    }
    nfl::device_batch<P> da(G * terms), db(G * terms), dv(terms), out(G);
    da.upload(ha.data());
    db.upload(hb.data());
    dv.upload(hb.data());
    out.assign_dot(da, db, terms);
    out.download(w.data());
    bool ok = true;
    for (size_t g = 0; g < G; ++g) ok &= same(w[g], want_d[g]);
    CHECK(ok, "device_batch: assign_dot");
    out.assign_matvec(da, dv);
    out.download(w.data());
    ok = true;
    for (size_t g = 0; g < G; ++g) ok &= same(w[g], want_m[g]);
    CHECK(ok, "device_batch: assign_matvec");
    bool threw = false;
    try {
      nfl::device_batch<P> small(G - 1);
      small.assign_dot(da, db, terms);
    } catch (std::runtime_error const &) {
      threw = true;
    }
    CHECK(threw, "operands of the wrong size throw std::runtime_error");
  }
}

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "eager") == 0) nfl::set_deferred(false);
    run<uint64_t, 1024, 2>("u64/1024/2", 5);
    run<uint64_t, 4096, 4>("u64/4096/4", 20);
    run<uint32_t, 1024, 3>("u32/1024/3", 17);
    run<uint16_t, 128, 2>("u16/128/2", 33);
    run<uint64_t, 64, 94>("u64/64/94", 3);
    CHECK(other_tu_dot() == 0, "second translation unit");
    std::printf(g_fail ? "dot: FAILED (%d)\n" : "dot: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("dot: exception: %s\n", e.what());
    return 2;
  }
}
