// dot_kernel.h -- k_dot, its operand classes and its launcher (kernels_dot.hip, which see for the arithmetic, the addressing and the
// plans), apart from their instances: kernels_dot.hip instantiates the strided and the pointer form, kernels_level.hip the form whose
// second operand is a key in its parent context's layout.  Device code; include after kernels.h, modarith.h and dot_reduce.h.
#pragma once
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"  // DotRed<T>, kDotChunk

namespace nflhip {

static constexpr int kDotTile = 4;         // groups per pass of the tiled plan
static constexpr size_t kDotWorkgroups = 4096;  // grid bound over all rows (dot_launch)

template <typename T, int V> struct alignas(V * sizeof(T)) DotVec { T e[V]; };

// operand (g, j) -> its element (0, 0).  Strided: strides in WORDS.  Pointers: one group, a pointer per term.
template <typename T> struct DotStrided {
  const T *ptr;
  size_t gs, ts;
  __device__ __forceinline__ const T *at(size_t g, unsigned j) const { return ptr + g * gs + (size_t)j * ts; }
};
template <typename T> struct DotPointers {
  const T *p[kDotMaxPointers];
  __device__ __forceinline__ const T *at(size_t, unsigned j) const { return p[j]; }
};
// A key in its PARENT context's layout read by a level context of fewer rows (kernels_level.hip; include/nflhip.h "leveled key
// switching"): shared by all groups, ts in words of the parent's polynomial, and the rows from `split` on lie `hole` words further on.
// blockIdx.y is the workgroup's row, so the hole is a scalar select.
template <typename T> struct DotKeyLevel {
  const T *ptr;
  size_t ts, hole;
  unsigned split;
  __device__ __forceinline__ const T *at(size_t, unsigned j) const { return ptr + (size_t)j * ts + (blockIdx.y >= split ? hole : (size_t)0); }
};

template <typename T, int V, int G, class OpA, class OpB>
__global__ void __launch_bounds__(256) k_dot(T *out, const OpA a, const OpB b, const T *addend, const ModConst<T> *__restrict__ mc,
                                             unsigned logn, unsigned nm, unsigned logv, size_t groups, unsigned terms, size_t total) {
  typedef DotVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr unsigned U = G == 1 ? 4 : 2;  // terms in flight per thread (kDotChunk is a multiple of both)
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the 16-byte groups per row
  const DotRed<T> red(mc[m]);
  const size_t poly = (size_t)nm << logn;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t g0 = (v >> lv) * G, off = ((size_t)m << logn) + ((v & ((((size_t)1) << lv) - 1u)) << logv);
    const unsigned ng = groups - g0 < (size_t)G ? (unsigned)(groups - g0) : (unsigned)G;
    acc_t acc[G][V];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      Vec t;
      if (addend && (unsigned)g < ng) t = *reinterpret_cast<const Vec *>(addend + (g0 + g) * poly + off);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[g][k] = addend && (unsigned)g < ng ? (acc_t)t.e[k] : (acc_t)0;
    }
    for (unsigned j0 = 0; j0 < terms; j0 += U) {
      Vec bv[U], av[G][U];
#pragma unroll
      for (unsigned u = 0; u < U; ++u) {
        if (j0 + u < terms) {
          bv[u] = *reinterpret_cast<const Vec *>(b.at(g0, j0 + u) + off);  // (tiled: b is shared, at(g0, j) == at(0, j))
#pragma unroll
          for (int g = 0; g < G; ++g)
            if ((unsigned)g < ng) av[g][u] = *reinterpret_cast<const Vec *>(a.at(g0 + g, j0 + u) + off);
        }
      }
#pragma unroll
      for (unsigned u = 0; u < U; ++u) {
        if (j0 + u < terms) {
#pragma unroll
          for (int g = 0; g < G; ++g)
            if ((unsigned)g < ng) {
#pragma unroll
              for (int k = 0; k < V; ++k) acc[g][k] += (acc_t)av[g][u].e[k] * (acc_t)bv[u].e[k];
            }
        }
      }
      if ((j0 + U) % kDotChunk == 0 && j0 + U < terms) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < V; ++k) acc[g][k] = (acc_t)red.reduce(acc[g][k]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if ((unsigned)g < ng) {
        Vec w;
#pragma unroll
        for (int k = 0; k < V; ++k) w.e[k] = red.reduce(acc[g][k]);
        *reinterpret_cast<Vec *>(out + (g0 + g) * poly + off) = w;
      }
    }
  }
}

template <typename T, int G, class OpA, class OpB>
static hipError_t dot_launch(const Shape &s, const DevTables &t, T *out, const OpA &a, const OpB &b, const T *addend, bool aligned,
                             size_t groups, size_t terms, hipStream_t st) {
  if (terms == 0 || terms > kDotMaxTerms || s.nm > 65535) return hipErrorInvalidValue;
  if (groups == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = aligned && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t ntiles = (groups + G - 1) / G, total = (ntiles * s.n) >> logv;
  // grid-stride over a bounded grid: kDotWorkgroups over all rows, 16 per CU.  The u64 kernels hold 76 - 112 VGPRs, 4 to 6 waves
  // per SIMD, so 4 to 6 of these 4-wave workgroups are resident per CU and the rest queue behind them and even out the tail.
  // Measured at 1024 / 2048 / 4096: the dense dot does not tell them apart, the matrix-vector form gains 12 - 14 %
  // from 1024 to the larger two, either plan.
  size_t blocks = (total + 255) / 256, cap = kDotWorkgroups / s.nm ? kDotWorkgroups / s.nm : 1;
  if (blocks > cap) blocks = cap;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g((unsigned)blocks, (unsigned)s.nm), bl(256);
  if (vec) hipLaunchKernelGGL((k_dot<T, V, G, OpA, OpB>), g, bl, 0, st, out, a, b, addend, mc, (unsigned)s.logn, (unsigned)s.nm, logv, groups, (unsigned)terms, total);
  else hipLaunchKernelGGL((k_dot<T, 1, G, OpA, OpB>), g, bl, 0, st, out, a, b, addend, mc, (unsigned)s.logn, (unsigned)s.nm, logv, groups, (unsigned)terms, total);
  return hipGetLastError();
}

}  // namespace nflhip
