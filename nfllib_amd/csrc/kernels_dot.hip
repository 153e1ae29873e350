// kernels_dot.hip -- sums of products ACROSS polynomials (include/nflhip.h "sums of products"):
//   out[g][m][i] = (addend[g][m][i] + sum_{j < terms} a(g,j)[m][i] * b(g,j)[m][i]) mod p_m        canonical words in and out.
// The inner step of an XPIR reply, of key switching and of any linear layer over NTT-form data; nothing here looks at the form.
//
// Arithmetic: the products are accumulated UNREDUCED in a double-width word and reduced once per chunk of kDotChunk terms;
// the bound and the reduction are in dot_reduce.h (shared with kernels_baseconv.hip).
//
// Addressing: blockIdx.y is the row m (its constants are scalar loads); a thread owns one 16-byte group of positions of that row
// for a TILE of up to G consecutive groups and walks the terms, U terms' loads issued ahead of their multiply chain.
//   G = 1  one group per pass: (2 terms + 1) rows of traffic per output row (+ 1 with an addend).
//   G = 4  for a second operand shared by all groups (group_stride 0): its words are loaded once and multiplied into 4
//          accumulators, so it is read once per 4 groups; the remainder tile runs the same code with fewer accumulators.
// A word variant (V = 1) serves misaligned pointers and rows shorter than 16 bytes.  The pointer form is the same body with one
// group and up to 16 pointers per operand in the kernel arguments.  No scratch, no allocation, no synchronisation.
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

template <typename T>
hipError_t launch_dot(const Shape &s, const DevTables &t, T *out, const T *a, size_t a_gs, size_t a_ts, const T *b, size_t b_gs, size_t b_ts,
                      const T *addend, size_t groups, size_t terms, int tiled, hipStream_t st) {
  const size_t poly = s.nm * s.n;
  DotStrided<T> x = {a, a_gs * poly, a_ts * poly}, y = {b, b_gs * poly, b_ts * poly};
  const bool aligned = (((uintptr_t)out | (uintptr_t)a | (uintptr_t)b | (uintptr_t)addend) & 15u) == 0;
  if (tiled && groups > 1 && (a_gs == 0 || b_gs == 0)) {
    if (b_gs != 0) { const DotStrided<T> z = x; x = y; y = z; }  // the product commutes: the shared operand is the one loaded once
    return dot_launch<T, kDotTile>(s, t, out, x, y, addend, aligned, groups, terms, st);
  }
  return dot_launch<T, 1>(s, t, out, x, y, addend, aligned, groups, terms, st);
}

template <typename T>
hipError_t launch_dot_ptrs(const Shape &s, const DevTables &t, T *out, const T *const *a, const T *const *b, size_t terms, const T *addend,
                           hipStream_t st) {
  if (terms == 0 || terms > (size_t)kDotMaxPointers) return hipErrorInvalidValue;
  DotPointers<T> x, y;
  uintptr_t bits = (uintptr_t)out | (uintptr_t)addend;
  for (size_t j = 0; j < (size_t)kDotMaxPointers; ++j) {
    x.p[j] = a[j < terms ? j : 0];
    y.p[j] = b[j < terms ? j : 0];
    bits |= (uintptr_t)x.p[j] | (uintptr_t)y.p[j];
  }
  return dot_launch<T, 1>(s, t, out, x, y, addend, (bits & 15u) == 0, 1, terms, st);
}

#define NFLHIP_DOT_INSTANCES(T)                                                                                                      \
  template hipError_t launch_dot<T>(const Shape &, const DevTables &, T *, const T *, size_t, size_t, const T *, size_t, size_t,     \
                                    const T *, size_t, size_t, int, hipStream_t);                                                    \
  template hipError_t launch_dot_ptrs<T>(const Shape &, const DevTables &, T *, const T *const *, const T *const *, size_t, const T *, \
                                         hipStream_t);
NFLHIP_DOT_INSTANCES(uint16_t)
NFLHIP_DOT_INSTANCES(uint32_t)
NFLHIP_DOT_INSTANCES(uint64_t)
#undef NFLHIP_DOT_INSTANCES

__global__ void k_warm_dot() {}
hipError_t warm_dot(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_dot, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
