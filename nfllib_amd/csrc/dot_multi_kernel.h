// dot_multi_kernel.h -- k_dot_multi, its argument classes and its launcher (kernels_dot_multi.hip, which see for the arithmetic, the
// addressing and the two forms), apart from their instances: kernels_dot_multi.hip instantiates the dense layout,
// kernels_level_rotate.hip the one whose second operands are components of keys in their parent context's layout.  Device code;
// include after kernels.h, modarith.h and dot_reduce.h.
#pragma once
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"  // DotRed<T>, kDotChunk

namespace nflhip {

static constexpr unsigned kDotMultiRegTerms = 8;     // the register form's last size
static constexpr int kDotMultiTile = 2;              // groups per pass of the tiled plan (the register report)
static constexpr size_t kDotMultiWorkgroups = 4096;  // grid bound over all rows, as dot_launch

template <typename T, int V> struct alignas(V * sizeof(T)) DotMultiVec { T e[V]; };

// The output and b pointers.  bhole(m): how many words further on than in a and the outputs the words of row m lie in b_o(j) -- none
// in the dense layout; a level key's hole (DotMultiArgsLevel) for the rows from `split` on.  m is blockIdx.y: one select per workgroup.
template <typename T> struct DotMultiArgs {
  T *out[kDotMultiMaxOutputs];
  const T *b[kDotMultiMaxOutputs];
  __device__ __forceinline__ size_t bhole(unsigned) const { return 0; }
};
// b_o = a component of a key in its PARENT context's layout, read by a level context of fewer rows (kernels_level_rotate.hip;
// include/nflhip.h "rotations and linear transforms at a level"): the rows from `split` on lie `hole` words further on.
// The register form at one group per pass already holds as many uniform values as there are scalar registers, and one more across
// its loops is parked in vector lanes (2 scalar registers spilled, measured).  So the selected hole is handed to a vector register
// pair once, before the loops, and added to the thread's own offset: no scalar register lives longer than the select.
template <typename T> struct DotMultiArgsLevel {
  T *out[kDotMultiMaxOutputs];
  const T *b[kDotMultiMaxOutputs];
  size_t hole;
  unsigned split;
  __device__ __forceinline__ size_t bhole(unsigned m) const {
    size_t h = m >= split ? hole : (size_t)0;
    asm volatile("" : "+v"(h));
    return h;
  }
};

template <typename T, int V, int G, int R, class Args>
__global__ void __launch_bounds__(256) k_dot_multi(const Args args, const T *__restrict__ a, size_t a_gs, size_t a_ts, size_t b_ts,
                                                   const ModConst<T> *__restrict__ mc, unsigned logn, unsigned nm, unsigned logv,
                                                   unsigned outputs, size_t groups, unsigned terms, size_t total) {
  typedef DotMultiVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the 16-byte groups per row
  const DotRed<T> red(mc[m]);
  const size_t poly = (size_t)nm << logn, bh = args.bhole(m);
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t g0 = (v >> lv) * G, off = ((size_t)m << logn) + ((v & ((((size_t)1) << lv) - 1u)) << logv);
    const unsigned ng = groups - g0 < (size_t)G ? (unsigned)(groups - g0) : (unsigned)G;
    const T *a0 = a + g0 * a_gs + off;
    if (R) {
      Vec av[G][kDotMultiRegTerms];
#pragma unroll
      for (unsigned j = 0; j < kDotMultiRegTerms; ++j) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (j < terms && (unsigned)g < ng) {
            av[g][j] = *reinterpret_cast<const Vec *>(a0 + g * a_gs + j * a_ts);
          } else {
#pragma unroll
            for (int k = 0; k < V; ++k) av[g][j].e[k] = 0;
          }
        }
      }
      for (unsigned o = 0; o < outputs; ++o) {
        const T *bp = args.b[o] + (off + bh);
        acc_t acc[G][V];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < V; ++k) acc[g][k] = 0;
#pragma unroll
        for (unsigned j = 0; j < kDotMultiRegTerms; ++j) {
          if (j < terms) {
            const Vec bv = *reinterpret_cast<const Vec *>(bp + j * b_ts);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
              for (int k = 0; k < V; ++k) acc[g][k] += (acc_t)av[g][j].e[k] * (acc_t)bv.e[k];
          }
        }
        T *op = args.out[o] + g0 * poly + off;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if ((unsigned)g < ng) {
            Vec w;
#pragma unroll
            for (int k = 0; k < V; ++k) w.e[k] = red.reduce(acc[g][k]);
            *reinterpret_cast<Vec *>(op + g * poly) = w;
          }
        }
      }
    } else {
      constexpr unsigned U = 2;  // terms in flight per thread (kDotChunk is a multiple)
      for (unsigned o = 0; o < outputs; ++o) {
        const T *bp = args.b[o] + (off + bh);
        acc_t acc[G][V];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < V; ++k) acc[g][k] = 0;
        for (unsigned j0 = 0; j0 < terms; j0 += U) {
          Vec bv[U], av[G][U];
#pragma unroll
          for (unsigned u = 0; u < U; ++u) {
            if (j0 + u < terms) {
              bv[u] = *reinterpret_cast<const Vec *>(bp + (size_t)(j0 + u) * b_ts);
#pragma unroll
              for (int g = 0; g < G; ++g)
                if ((unsigned)g < ng) av[g][u] = *reinterpret_cast<const Vec *>(a0 + g * a_gs + (size_t)(j0 + u) * a_ts);
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
        T *op = args.out[o] + g0 * poly + off;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if ((unsigned)g < ng) {
            Vec w;
#pragma unroll
            for (int k = 0; k < V; ++k) w.e[k] = red.reduce(acc[g][k]);
            *reinterpret_cast<Vec *>(op + g * poly) = w;
          }
        }
      }
    }
  }
}

template <typename T, int G, class Args>
static hipError_t dot_multi_launch(const Shape &s, const DevTables &t, const Args &args, const T *a, size_t a_gs, size_t a_ts,
                                   size_t b_ts, bool aligned, size_t outputs, size_t groups, size_t terms, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const bool vec = aligned && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t ntiles = (groups + G - 1) / G, total = (ntiles * s.n) >> logv;
  // grid-stride over a bounded grid, as dot_launch: kDotMultiWorkgroups over all rows
  size_t blocks = (total + 255) / 256, cap = kDotMultiWorkgroups / s.nm ? kDotMultiWorkgroups / s.nm : 1;
  if (blocks > cap) blocks = cap;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g((unsigned)blocks, (unsigned)s.nm), bl(256);
  const unsigned logn = (unsigned)s.logn, nm = (unsigned)s.nm, no = (unsigned)outputs, nt = (unsigned)terms;
  const bool reg = terms <= kDotMultiRegTerms;
#define NFLHIP_DOT_MULTI_GO(VV, RR) \
  hipLaunchKernelGGL((k_dot_multi<T, VV, G, RR, Args>), g, bl, 0, st, args, a, a_gs, a_ts, b_ts, mc, logn, nm, logv, no, groups, nt, total)
  if (vec && reg) NFLHIP_DOT_MULTI_GO(V, 1);
  else if (vec) NFLHIP_DOT_MULTI_GO(V, 0);
  else if (reg) NFLHIP_DOT_MULTI_GO(1, 1);
  else NFLHIP_DOT_MULTI_GO(1, 0);
#undef NFLHIP_DOT_MULTI_GO
  return hipGetLastError();
}

}  // namespace nflhip
