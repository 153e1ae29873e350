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
// The kernel and its launcher are in dot_multi_kernel.h; this file holds the instances on the dense layout.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"  // DotRed<T>, kDotChunk
#include "dot_multi_kernel.h"

namespace nflhip {

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
