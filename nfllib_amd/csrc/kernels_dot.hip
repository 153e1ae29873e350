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
#include "dot_kernel.h"  // k_dot, DotStrided, DotPointers, dot_launch

namespace nflhip {

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
