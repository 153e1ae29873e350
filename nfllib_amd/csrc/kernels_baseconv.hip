// kernels_baseconv.hip -- RNS fast base conversion and mod-down by the last k moduli (include/nflhip.h "RNS base conversion").
//
// Source rows S = [s0, s0 + ks), destination rows D = [d0, d0 + kd) of one context, Q = prod_{i in S} p_i.  Per coefficient
// position, from the canonical source words x_i:
//   y_i   = x_i (Q/p_i)^-1 mod p_i                                  canonical (Shoup's multiplication by a table constant)
//   fast     out_j = (sum_i y_i c_ij) mod p_j,   c_ij = (Q/p_i) mod p_j       = (x + u Q) mod p_j, u = floor(sum_i y_i / p_i) < ks
//   centred  out_j = (sum_i y_i c_ij - v Q_j) mod p_j,  Q_j = Q mod p_j,  v = floor((sum_i f_i + 2^59) / 2^60),
//            f_i the 60-bit fixed-point image of y_i / p_i:  64-bit limbs  f_i = floor(y_i floor(2^124 / p_i) / 2^64),
//                                                           32 / 16 bits  f_i = y_i floor(2^60 / p_i)
//   mod-down (S = the last k rows, D = the rows before them, output stride nm - k rows)
//            Y_j = (x_j - conv_j) P^-1 mod p_j,  conv_j the centred (default) or the fast (floor) conversion above, P = Q.
// Why v - u is 0 or 1, and which x round which way: DESIGN.md 5.14.
//
// sum_i f_i: every f_i is below 2^60 and a context has up to 1024 rows, so the sum is kept as a 60-bit low part and a count of
// the carries out of it: no ks overflows it.  v < ks + 1 <= 1025 is a word of every limb width.
// sum_i y_i c_ij: unreduced in the double-width word, reduced once per kDotChunk = 16 terms (dot_reduce.h: bound and reduction).
// v Q_j: Shoup's multiplication (any word v -> [0, 2p), one conditional subtraction), subtracted from the canonical sum.
//
// Plans.  A thread owns one 16-byte group of coefficient positions of one polynomial (V words; V = 1: the word variant for
// misaligned pointers and rows shorter than 16 bytes).  K is the number of source rows a thread keeps in registers:
//   K = 4, 16   ks <= K: the source words are read ONCE, all loads in flight together, y_i and sum f_i formed in registers, then
//               the destination rows are walked: ks multiply-adds and one reduction per word.  (ks + kd) rows of traffic, + kd for
//               the mod-down's x_j.  Every source word is in a register before the first store, so out == in is served; there
//               the destination rows that are source rows are skipped (they hold x_j already): ks + |D \ S| rows of traffic.
//   K = 0       any ks: per destination row the sources are read again in chunks of 16 with the canonical partial sum carried
//               (1 + kd passes over the sources, kd ks Shoup multiplications per position: correct, not fast).  In place no
//               source row is written (the skip above), so the later passes read what the first one read.
// The (i, j) constants are wave-uniform: the record and ModConst are indexed by loop counters only, so they are scalar loads.
// 256 threads, grid-stride, at most 1024 workgroups (four per CU, as kernels_rescale.hip).  No LDS, no scratch.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"  // the per-position arithmetic: bc_y, bc_frac, bc_fsum_*, bc_finish

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) BcVec { T e[V]; };
struct alignas(32) BcSrc { uint64_t w, wp, p, r; };  // a source row's record (host_tables.h)

// mode bit 0: centred conversion; bit 1: mod-down (reads row d0 + j of `in`, multiplies the difference by P^-1); bit 2: in place
// (out == in): a destination row that is a source row already holds its words -- both modes give x_j for j in S -- and is skipped
template <typename T, int V, int K>
__global__ void __launch_bounds__(256) k_baseconv(T *out, const T *in, const ModConst<T> *__restrict__ mc, const uint64_t *__restrict__ rec,
                                                  unsigned logn, unsigned nm, unsigned onm, unsigned s0_arg, unsigned ks_arg, unsigned d0_arg,
                                                  unsigned kd_arg, unsigned mode_arg, size_t total) {
  typedef BcVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr int KR = K > 0 ? K : 1;
  constexpr unsigned logv = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : 3;  // V words per group
  const unsigned lv = logn - logv;  // log2 of the groups per row
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t b = t >> lv, pos = (t & ((((size_t)1) << lv) - 1u)) << logv;
    // ks, s0, d0, kd, the mode, log n and the record offset as values of THIS iteration: the sixteen loop-invariant guards
    // "i < ks", row offsets and record addresses below would otherwise be hoisted out of the grid-stride loop, all live at
    // once, and spill scalar registers (tests/test_baseconv_cpu.py reads the compiler's resource report of this file)
    unsigned ks = ks_arg, s0 = s0_arg, d0 = d0_arg, kd = kd_arg, mode = mode_arg, lg = logn;
    asm volatile("" : "+s"(ks), "+s"(s0), "+s"(d0), "+s"(kd), "+s"(mode), "+s"(lg));
    const size_t row = (size_t)1 << lg;
    size_t zero = 0;  // (an offset, not the pointer: the pointer would lose its address space and the scalar loads with it)
    asm volatile("" : "+s"(zero));
    const uint64_t *__restrict__ src = rec + zero;
    const uint64_t *__restrict__ dst = src + 4 * (size_t)ks, *__restrict__ cm = dst + 8 * (size_t)kd;
    const bool centred = (mode & 1u) != 0, down = (mode & 2u) != 0;
    const T *x = in + ((b * nm) << logn) + pos;
    T *o = out + ((b * onm) << logn) + pos;
    uint64_t flo[V], fhi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) flo[k] = fhi[k] = 0;
    T y[KR][V];
    if (K > 0) {
      Vec xv[KR];
#pragma unroll
      for (int i = 0; i < K; ++i)
        if ((unsigned)i < ks) xv[i] = *reinterpret_cast<const Vec *>(x + (s0 + i) * row);
#pragma unroll
      for (int i = 0; i < K; ++i)
        if ((unsigned)i < ks) {
          const BcSrc rc = reinterpret_cast<const BcSrc *>(src)[i];  // one 32-byte scalar load
#pragma unroll
          for (int k = 0; k < V; ++k) {
            y[i][k] = bc_y<T>(xv[i].e[k], (T)rc.w, (T)rc.wp, (T)rc.p);
            if (centred) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(y[i][k], rc.r));
          }
        }
    } else if (centred) {
      for (unsigned i = 0; i < ks; ++i) {
        const Vec xv = *reinterpret_cast<const Vec *>(x + ((size_t)(s0 + i) << logn));
        const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], p = (T)src[4 * i + 2];
        const uint64_t r = src[4 * i + 3];
#pragma unroll
        for (int k = 0; k < V; ++k) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(bc_y<T>(xv.e[k], w, wp, p), r));
      }
    }
    T v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (T)bc_fsum_round(flo[k], fhi[k]);
    for (unsigned j = 0; j < kd; ++j) {
      if ((mode & 4u) && d0 + j - s0 < ks) continue;  // (unsigned: s0 <= d0 + j < s0 + ks)
      const DotRed<T> red(mc[d0 + j]);
      const T p = (T)dst[8 * j];
      const uint64_t *__restrict__ c = cm + (size_t)j * ks;
      Vec xj = {};
      if (down) xj = *reinterpret_cast<const Vec *>(x + ((size_t)(d0 + j) << logn));
      acc_t acc[V];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = 0;
      if (K > 0) {
#pragma unroll
        for (int i = 0; i < K; ++i)  // K <= kDotChunk terms: no reduction on the way
          if ((unsigned)i < ks) {
            const T cij = (T)c[i];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += (acc_t)y[i][k] * (acc_t)cij;
          }
      } else {
        for (unsigned i = 0; i < ks; ++i) {
          const Vec xv = *reinterpret_cast<const Vec *>(x + ((size_t)(s0 + i) << logn));
          const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], pi = (T)src[4 * i + 2], cij = (T)c[i];
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += (acc_t)bc_y<T>(xv.e[k], w, wp, pi) * (acc_t)cij;
          if ((i + 1) % kDotChunk == 0 && i + 1 < ks) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = (acc_t)red.reduce(acc[k]);
          }
        }
      }
      const T qj = (T)dst[8 * j + 1], qj_sh = (T)dst[8 * j + 2], pinv = (T)dst[8 * j + 3], pinv_sh = (T)dst[8 * j + 4];
      Vec w;
#pragma unroll
      for (int k = 0; k < V; ++k) w.e[k] = bc_finish<T>(red.reduce(acc[k]), centred, v[k], qj, qj_sh, down, xj.e[k], pinv, pinv_sh, p);
      *reinterpret_cast<Vec *>(o + ((size_t)(d0 + j) << logn)) = w;
    }
  }
}

template <typename T, int V>
static void baseconv_pick(dim3 g, hipStream_t st, T *out, const T *in, const ModConst<T> *mc, const uint64_t *rec, unsigned logn, unsigned nm,
                          unsigned onm, unsigned s0, unsigned ks, unsigned d0, unsigned kd, unsigned mode, size_t total) {
  const dim3 bl(256);
  if (ks <= 4) hipLaunchKernelGGL((k_baseconv<T, V, 4>), g, bl, 0, st, out, in, mc, rec, logn, nm, onm, s0, ks, d0, kd, mode, total);
  else if (ks <= 16) hipLaunchKernelGGL((k_baseconv<T, V, 16>), g, bl, 0, st, out, in, mc, rec, logn, nm, onm, s0, ks, d0, kd, mode, total);
  else hipLaunchKernelGGL((k_baseconv<T, V, 0>), g, bl, 0, st, out, in, mc, rec, logn, nm, onm, s0, ks, d0, kd, mode, total);
}

template <typename T>
hipError_t launch_baseconv(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t s0, size_t ks,
                           size_t d0, size_t kd, int centred, int moddown, hipStream_t st) {
  if (!rec || ks == 0 || kd == 0 || s0 + ks > s.nm || d0 + kd > s.nm || s.nm > 65535) return hipErrorInvalidValue;
  if (moddown && (d0 != 0 || kd != s0 || s0 + ks != s.nm)) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const unsigned mode = (centred ? 1u : 0u) | (moddown ? 2u : 0u) | (!moddown && (const T *)out == in ? 4u : 0u), onm = (unsigned)(moddown ? kd : s.nm);
  const dim3 g((unsigned)blocks);
  if (vec) baseconv_pick<T, V>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)s.nm, onm, (unsigned)s0, (unsigned)ks, (unsigned)d0, (unsigned)kd, mode, total);
  else baseconv_pick<T, 1>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)s.nm, onm, (unsigned)s0, (unsigned)ks, (unsigned)d0, (unsigned)kd, mode, total);
  return hipGetLastError();
}

template hipError_t launch_baseconv<uint16_t>(const Shape &, const DevTables &, uint16_t *, const uint16_t *, const uint64_t *, size_t, size_t, size_t, size_t, size_t, int, int, hipStream_t);
template hipError_t launch_baseconv<uint32_t>(const Shape &, const DevTables &, uint32_t *, const uint32_t *, const uint64_t *, size_t, size_t, size_t, size_t, size_t, int, int, hipStream_t);
template hipError_t launch_baseconv<uint64_t>(const Shape &, const DevTables &, uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t, size_t, size_t, size_t, int, int, hipStream_t);

// rows [0, ks) of in = [batch][inm][n] to rows [d0, d0 + kd) of out = [batch][onm][n]: the kernel takes `nm` only as the input's rows
// per polynomial and `s0` only as the source row offset, so a gathered copy of the source rows is served by the same code
template <typename T>
hipError_t launch_baseconv_rows(const Shape &s, const DevTables &t, T *out, size_t onm, const T *in, size_t inm, const uint64_t *rec, size_t batch,
                                size_t ks, size_t d0, size_t kd, int centred, hipStream_t st) {
  if (!rec || ks == 0 || kd == 0 || ks > inm || d0 + kd > s.nm || inm > 65535 || onm > 65535 || (const T *)out == in) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const unsigned mode = centred ? 1u : 0u;
  const dim3 g((unsigned)blocks);
  if (vec) baseconv_pick<T, V>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)inm, (unsigned)onm, 0u, (unsigned)ks, (unsigned)d0, (unsigned)kd, mode, total);
  else baseconv_pick<T, 1>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)inm, (unsigned)onm, 0u, (unsigned)ks, (unsigned)d0, (unsigned)kd, mode, total);
  return hipGetLastError();
}
template hipError_t launch_baseconv_rows<uint16_t>(const Shape &, const DevTables &, uint16_t *, size_t, const uint16_t *, size_t, const uint64_t *, size_t, size_t, size_t, size_t, int, hipStream_t);
template hipError_t launch_baseconv_rows<uint32_t>(const Shape &, const DevTables &, uint32_t *, size_t, const uint32_t *, size_t, const uint64_t *, size_t, size_t, size_t, size_t, int, hipStream_t);
template hipError_t launch_baseconv_rows<uint64_t>(const Shape &, const DevTables &, uint64_t *, size_t, const uint64_t *, size_t, const uint64_t *, size_t, size_t, size_t, size_t, int, hipStream_t);

__global__ void k_warm_baseconv() {}
hipError_t warm_baseconv(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_baseconv, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
