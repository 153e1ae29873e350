// tests/cpp_baseconv/sharded_main.cpp -- sharded_batch::assign_base_convert / assign_mod_down over SEVERAL shards: everything a
// shard computes must be word for word what the same polynomials give in ONE device_batch, for batch sizes that do not divide by
// the number of shards and for more shards than polynomials (empty shards); batches that are split differently are refused.
// Usage: sharded_baseconv <device list, e.g. 0,1,2,3 or 0,0,0> [batch].  Runs against the real library (GPU: several shards on
// device 0) and, on the CPU, against tests/cpp/mock with NFLHIP_MOCK_DEVICES virtual devices plus the toy entries of
// toy_baseconv.c -- every buffer belongs to one device there, so a shard enqueued on the wrong context fails loudly
// (tests/test_cpp_baseconv.py).  Exit code 0 = identical, 1 = a mismatch, 2 = an exception.
#include <nfl.hpp>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, what)                                                                   \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_fail; } \
  } while (0)

template <class P, class B> static std::vector<typename P::value_type> words_of(const B &b) {
  std::vector<P> h(b.size());
  if (b.size()) b.download(h.data());
  std::vector<typename P::value_type> w;
  for (auto &p : h) w.insert(w.end(), p.begin(), p.end());
  return w;
}
template <class P> static std::vector<typename P::value_type> words(const nfl::device_batch<P> &b) { return words_of<P>(b); }
template <class P> static std::vector<typename P::value_type> words(const nfl::sharded_batch<P> &b) { return words_of<P>(b); }
template <class F> static bool throws(F f) {
  try {
    f();
  } catch (std::runtime_error const &) {
    return true;
  }
  return false;
}

template <class T, size_t D, size_t M, size_t K> static void run(const std::vector<int> &devs, size_t B, const char *name) {
  typedef nfl::poly<T, D, M> P;
  typedef nfl::poly<T, D, M - K> S;
  std::printf("%s, %zu polynomials over %zu shards\n", name, B, devs.size());
  const int dev0 = devs[0];
  nfl::device_batch<P> a1(B, dev0), u1(B, dev0);
  nfl::device_batch<S> y1(B, dev0);
  nfl::sharded_batch<P> a(B, devs), u(B, devs);
  nfl::sharded_batch<S> y(B, devs);
  a1.set(nfl::uniform(0x1234));
  a.set(nfl::uniform(0x1234));
  u1.set(nfl::uniform(0x77));
  u.set(nfl::uniform(0x77));
  CHECK(a.shards() == devs.size() && y.shards() == devs.size(), "one shard per entry of the device list");
  CHECK(words(a) == words(a1) && words(u) == words(u1), "the operands, generated in place");
  for (int floor = 0; floor < 2; ++floor) {
    y1.assign_mod_down(a1, floor != 0);
    y.assign_mod_down(a, floor != 0);
    CHECK(words(y) == words(y1), "assign_mod_down, shard by shard");
  }
  CHECK(words(a) == words(a1), "the mod-down leaves its source as it was");
  for (int centered = 0; centered < 2; ++centered) {
    u1.assign_base_convert(a1, M - K, K, 0, M - K, centered != 0);   // from another batch: the rows outside D keep u's words
    u.assign_base_convert(a, M - K, K, 0, M - K, centered != 0);
    CHECK(words(u) == words(u1), "assign_base_convert from another batch");
    u1.assign_base_convert(u1, 0, M - K, 0, M, centered != 0);       // in place, the mod-up
    u.assign_base_convert(u, 0, M - K, 0, M, centered != 0);
    CHECK(words(u) == words(u1), "assign_base_convert in place");
  }
  // batches that are split differently are refused before anything runs
  const std::vector<T> before = words(y);
  std::vector<int> more(devs);
  more.push_back(dev0);
  CHECK(throws([&] { nfl::sharded_batch<S> z(B, more); z.assign_mod_down(a); }), "mod-down: another number of shards throws");
  CHECK(throws([&] { nfl::sharded_batch<S> z(B + 1, devs); z.assign_mod_down(a); }), "mod-down: another batch size throws");
  CHECK(throws([&] { nfl::sharded_batch<P> z(B, more); z.assign_base_convert(a, 0, 1, 1, 1); }), "base_convert: another number of shards throws");
  CHECK(throws([&] { nfl::sharded_batch<P> z(B + 1, devs); z.assign_base_convert(a, 0, 1, 1, 1); }), "base_convert: another batch size throws");
  if (devs.size() > 1 && devs[0] != devs[1]) {
    std::vector<int> swapped(devs);
    std::swap(swapped[0], swapped[1]);
    CHECK(throws([&] { nfl::sharded_batch<S> z(B, swapped); z.assign_mod_down(a); }), "mod-down: shards on other devices throw");
  }
  CHECK(words(y) == before, "a refused call writes nothing");
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
    run<uint64_t, 64, 4, 2>(devs, B, "u64/64/4 k=2");
    run<uint64_t, 64, 4, 1>(devs, B, "u64/64/4 k=1");
    run<uint32_t, 64, 3, 2>(devs, B, "u32/64/3 k=2");
    std::printf(g_fail ? "sharded baseconv: FAILED (%d)\n" : "sharded baseconv: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  } catch (std::exception const &e) {
    std::printf("sharded baseconv: exception: %s\n", e.what());
    return 2;
  }
}
