// kernels_dot_multi.hip -- a small matrix product over polynomials (include/nflhip.h "sums of products, several outputs"):
//   out_o[g][m][i] = (sum_{j < terms} a(g,j)[m][i] * b_o(j)[m][i]) mod p_m        o < outputs <= 32, canonical words in and out.
// The first operand is shared by every output, each second operand by every group: the inner products of a hoisted rotation
// (a = the mod-upped digits, b_o = a component of a Galois key), several XPIR queries against one database, a linear layer with
// several output channels.  Word for word what k_dot (kernels_dot.hip) gives per output; the arithmetic is that of dot_reduce.h.
//
// Addressing as k_dot: blockIdx.y is the row m; a thread owns one 16-byte group of positions of that row for a TILE of up to G
// consecutive groups.  The output and b pointers travel by value in the kernel arguments.
//   R = 1  register-resident, terms <= kDotMultiRegTerms: the thread loads its words of a(g, j) for the whole tile ONCE, then walks
//          the outputs: b_o(j) is loaded once per tile and multiplied into G accumulators, one reduce (8 terms never wrap), one store.
//          a is read once per call, b_o once per G groups.
//   R = 0  streaming, more terms: per output the terms are walked two at a time as k_dot does, reduced every kDotChunk; a is
//          re-read per output, from cache where the tile's words still are.
// A word variant (V = 1) serves misaligned pointers and rows shorter than 16 bytes.  No scratch, no allocation, no synchronisation.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"  // DotRed<T>, kDotChunk

namespace nflhip {

static constexpr unsigned kDotMultiRegTerms = 8;     // the register form's last size
static constexpr int kDotMultiTile = 2;              // groups per pass of the tiled plan (the register report)
static constexpr size_t kDotMultiWorkgroups = 4096;  // grid bound over all rows, as dot_launch

template <typename T, int V> struct alignas(V * sizeof(T)) DotMultiVec { T e[V]; };

template <typename T> struct DotMultiArgs {
  T *out[kDotMultiMaxOutputs];
  const T *b[kDotMultiMaxOutputs];
};

template <typename T, int V, int G, int R>
__global__ void __launch_bounds__(256) k_dot_multi(const DotMultiArgs<T> args, const T *__restrict__ a, size_t a_gs, size_t a_ts, size_t b_ts,
                                                   const ModConst<T> *__restrict__ mc, unsigned logn, unsigned nm, unsigned logv,
                                                   unsigned outputs, size_t groups, unsigned terms, size_t total) {
  typedef DotMultiVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the 16-byte groups per row
  const DotRed<T> red(mc[m]);
  const size_t poly = (size_t)nm << logn;
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
        const T *bp = args.b[o] + off;
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
        const T *bp = args.b[o] + off;
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

template <typename T, int G>
static hipError_t dot_multi_launch(const Shape &s, const DevTables &t, const DotMultiArgs<T> &args, const T *a, size_t a_gs, size_t a_ts,
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
  hipLaunchKernelGGL((k_dot_multi<T, VV, G, RR>), g, bl, 0, st, args, a, a_gs, a_ts, b_ts, mc, logn, nm, logv, no, groups, nt, total)
  if (vec && reg) NFLHIP_DOT_MULTI_GO(V, 1);
  else if (vec) NFLHIP_DOT_MULTI_GO(V, 0);
  else if (reg) NFLHIP_DOT_MULTI_GO(1, 1);
  else NFLHIP_DOT_MULTI_GO(1, 0);
#undef NFLHIP_DOT_MULTI_GO
  return hipGetLastError();
}

template <typename T>
hipError_t launch_dot_multi(const Shape &s, const DevTables &t, T *const *outs, const T *a, size_t a_gs, size_t a_ts, const T *const *bs,
                            size_t b_ts, size_t outputs, size_t groups, size_t terms, int tiled, hipStream_t st) {
  if (outputs == 0 || outputs > (size_t)kDotMultiMaxOutputs || terms == 0 || terms > kDotMaxTerms || s.nm > 65535) return hipErrorInvalidValue;
  if (groups == 0) return hipSuccess;
  const size_t poly = s.nm * s.n;
  DotMultiArgs<T> args;
  uintptr_t bits = (uintptr_t)a;
  for (size_t o = 0; o < (size_t)kDotMultiMaxOutputs; ++o) {
    args.out[o] = outs[o < outputs ? o : 0];
    args.b[o] = bs[o < outputs ? o : 0];
    bits |= (uintptr_t)args.out[o] | (uintptr_t)args.b[o];
  }
  const bool aligned = (bits & 15u) == 0;
  if (tiled && groups > 1) return dot_multi_launch<T, kDotMultiTile>(s, t, args, a, a_gs * poly, a_ts * poly, b_ts * poly, aligned, outputs, groups, terms, st);
  return dot_multi_launch<T, 1>(s, t, args, a, a_gs * poly, a_ts * poly, b_ts * poly, aligned, outputs, groups, terms, st);
}

#define NFLHIP_DOT_MULTI_INSTANCES(T)                                                                                              \
  template hipError_t launch_dot_multi<T>(const Shape &, const DevTables &, T *const *, const T *, size_t, size_t, const T *const *, \
                                          size_t, size_t, size_t, size_t, int, hipStream_t);
NFLHIP_DOT_MULTI_INSTANCES(uint16_t)
NFLHIP_DOT_MULTI_INSTANCES(uint32_t)
NFLHIP_DOT_MULTI_INSTANCES(uint64_t)
#undef NFLHIP_DOT_MULTI_INSTANCES

__global__ void k_warm_dot_multi() {}
hipError_t warm_dot_multi(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_dot_multi, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
