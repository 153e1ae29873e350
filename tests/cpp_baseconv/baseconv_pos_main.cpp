// baseconv_pos_main.cpp -- the per-position arithmetic of kernels_baseconv.hip on the CPU: the very functions the kernel calls
// (nfllib_amd/csrc/baseconv_pos.h, dot_reduce.h, modarith.h, compiled against the stand-in runtime header of shim/), driven by the
// table record of host_tables.cpp.  tests/test_baseconv_cpu.py feeds it words and compares the output with the Python restatement.
//
//   baseconv_pos_main record LB S0 KS D0 KD MODDOWN < moduli            -> rc, then the record's 64-bit words, one per line
//   baseconv_pos_main conv LB S0 KS D0 KD MODE PLAN NPOS < moduli, words  -> the destination words, position-major
// moduli: "nm" then nm moduli.  words: NPOS lines of nm words (row 0 .. nm - 1 of one position).  MODE bit 0 centred, bit 1 mod-down.
// PLAN 1: the register plan (all y_i first, one reduction per destination; KS <= 16); PLAN 0: the chunked plan (a reduction per
// 16 sources, y_i formed again per destination).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nfllib_amd/csrc/baseconv_pos.h"
#include "../../nfllib_amd/csrc/host_tables.h"

using namespace nflhip;

// the ModConst fields the reduction reads, as host_tables.cpp twiddles_and_modconst fills them
template <typename T> static ModConst<T> mod_const(uint64_t p) {
  typedef unsigned __int128 u128;
  const int wb = 8 * (int)sizeof(T);
  ModConst<T> m;
  memset(&m, 0, sizeof m);
  m.p = (T)p;
  m.p2 = (T)(2 * p);
  m.mu = (T)((((u128)1) << (2 * wb - 4)) / p);
  const uint64_t beta = (uint64_t)((((u128)1) << 64) % p);
  m.beta = (T)beta;
  m.beta_sh = (T)((((u128)beta) << wb) / p);
  return m;
}

template <typename T>
static void position(const std::vector<uint64_t> &P, const std::vector<uint64_t> &rec, const uint64_t *x, size_t s0, size_t ks, size_t d0,
                     size_t kd, unsigned mode, int plan, uint64_t *out) {
  typedef typename DotRed<T>::acc_t acc_t;
  const uint64_t *src = rec.data(), *dst = src + 4 * ks, *cm = dst + 8 * kd;
  const bool centred = mode & 1u, down = mode & 2u;
  std::vector<T> y(ks);
  uint64_t flo = 0, fhi = 0;
  for (size_t i = 0; i < ks; ++i) {
    y[i] = bc_y<T>((T)x[s0 + i], (T)src[4 * i], (T)src[4 * i + 1], (T)src[4 * i + 2]);
    if (centred) bc_fsum_add(flo, fhi, bc_frac<T>(y[i], src[4 * i + 3]));
  }
  const T v = (T)bc_fsum_round(flo, fhi);
  for (size_t j = 0; j < kd; ++j) {
    const ModConst<T> mc = mod_const<T>(P[d0 + j]);
    const DotRed<T> red(mc);
    acc_t acc = 0;
    for (size_t i = 0; i < ks; ++i) {
      const T yi = plan ? y[i] : bc_y<T>((T)x[s0 + i], (T)src[4 * i], (T)src[4 * i + 1], (T)src[4 * i + 2]);
      acc += (acc_t)yi * (acc_t)(T)cm[j * ks + i];
      if (!plan && (i + 1) % kDotChunk == 0 && i + 1 < ks) acc = (acc_t)red.reduce(acc);
    }
    out[j] = bc_finish<T>(red.reduce(acc), centred, v, (T)dst[8 * j + 1], (T)dst[8 * j + 2], down, (T)x[d0 + j], (T)dst[8 * j + 3],
                          (T)dst[8 * j + 4], (T)dst[8 * j]);
  }
}

int main(int argc, char **argv) {
  if (argc < 8) return 2;
  const std::string cmd = argv[1];
  const int lb = atoi(argv[2]);
  const size_t s0 = strtoull(argv[3], 0, 10), ks = strtoull(argv[4], 0, 10), d0 = strtoull(argv[5], 0, 10), kd = strtoull(argv[6], 0, 10);
  size_t nm = 0;
  if (scanf("%zu", &nm) != 1) return 2;
  std::vector<uint64_t> P(nm);
  for (size_t i = 0; i < nm; ++i)
    if (scanf("%lu", &P[i]) != 1) return 2;
  const unsigned mode = (unsigned)atoi(argv[7]);
  std::vector<uint64_t> rec;
  std::string err;
  const int rc = build_baseconv_record(lb, P, s0, ks, d0, kd, cmd == "record" ? mode != 0 : (mode & 2u) != 0, &rec, &err);
  if (cmd == "record") {
    printf("%d %s\n", rc, err.c_str());
    if (!rc)
      for (uint64_t w : rec) printf("%lu\n", w);
    return 0;
  }
  if (rc || argc < 10) return 2;
  const int plan = atoi(argv[8]);
  if (plan && ks > kDotChunk) return 2;
  const size_t npos = strtoull(argv[9], 0, 10);
  std::vector<uint64_t> x(nm), out(kd);
  for (size_t t = 0; t < npos; ++t) {
    for (size_t i = 0; i < nm; ++i)
      if (scanf("%lu", &x[i]) != 1) return 2;
    if (lb == 64) position<uint64_t>(P, rec, x.data(), s0, ks, d0, kd, mode, plan, out.data());
    else if (lb == 32) position<uint32_t>(P, rec, x.data(), s0, ks, d0, kd, mode, plan, out.data());
    else position<uint16_t>(P, rec, x.data(), s0, ks, d0, kd, mode, plan, out.data());
    for (size_t j = 0; j < kd; ++j) printf("%lu%c", out[j], j + 1 < kd ? ' ' : '\n');
  }
  return 0;
}
