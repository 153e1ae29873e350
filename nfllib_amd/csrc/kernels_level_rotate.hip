// kernels_level_rotate.hip -- the key and diagonal reads of a hoisted rotation or a slot linear transform BELOW the context's top level
// (include/nflhip.h "rotations and linear transforms at a level").  A level-l call runs rotate_run / lintrans_run (api.hip) on the
// child context C_l over the rows [0, l) and [L, nm) of its parent, as kernels_level.hip describes for the key switch.  What the child
// cannot give are the Galois keys and the plaintext diagonals, which stay the ONE top-level set in the parent's layout: keys
// [dnum_L][2][knm][n], diagonals [knm][n], with a hole of L - l rows between the child's row l - 1 and its row l.  Two kernels read
// them on all l + K rows, and each gets instances here that know the layout (KeyLevel, kernels.h):
//
// k_dot_multi<T, V, G, R, DotMultiArgsLevel<T>>  dot_multi_kernel.h: b_o = keys[m] + c knm n, a term every 2 knm n words; blockIdx.y is
//   the row, so the hole is one scalar select per workgroup, added to the thread's offset into b.  a and the outputs keep the child's dense layout.  All forms:
//   16-byte groups and words, G = 2 and 1, register and streaming.
// k_permute_mac_ntt<T, VEC, false, MacTermsLevel<T>>  permute_mac_kernel.h: the weight row of data row r is r + (r >= split ? hole : 0).
//   Chunked tiles: r is the tile's row, a scalar select.  Whole rows per tile: r is per item and a tile can straddle the split, a vector
//   select.  One staging buffer only: the two-buffer form is the measured loser and the linear transform never asks for it.
// The rows [l, L) of a key or a diagonal and the digits >= ceil(l / alpha) of a key are never addressed.  The instances of
// kernels_dot_multi.hip and kernels_lintrans.hip are the same templates on the dense layout: a template parameter tells them apart,
// nothing at run time.  u16 contexts have two moduli and so no level below the top: the u16 instances exist for the limb dispatch and
// are covered by the compiler's report alone.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "dot_multi_kernel.h"
#include "permute_mac_kernel.h"

namespace nflhip {

static bool key_level_ok(const Shape &s, const KeyLevel &kl) {  // the child's rows lie inside a parent polynomial
  return kl.split >= 1 && kl.split < s.nm && kl.knm == s.nm + kl.hole && kl.knm <= 65535;
}

// launch_dot_multi with bs[o] = the first word of component c of a key in the parent's layout (key + c knm n words)
template <typename T>
hipError_t launch_dot_multi_level(const Shape &s, const DevTables &t, T *const *outs, const T *a, size_t a_gs, size_t a_ts, const T *const *bs,
                                  size_t outputs, size_t groups, size_t terms, int tiled, const KeyLevel &kl, hipStream_t st) {
  if (outputs == 0 || outputs > (size_t)kDotMultiMaxOutputs || terms == 0 || terms > kDotMaxTerms || s.nm > 65535) return hipErrorInvalidValue;
  if (!key_level_ok(s, kl)) return hipErrorInvalidValue;
  if (groups == 0) return hipSuccess;
  const size_t poly = s.nm * s.n, b_ts = 2 * kl.knm * s.n;  // key[d][c]: two parent polynomials per term
  DotMultiArgsLevel<T> args;
  args.hole = kl.hole * s.n;
  args.split = (unsigned)kl.split;
  uintptr_t bits = (uintptr_t)a;
  for (size_t o = 0; o < (size_t)kDotMultiMaxOutputs; ++o) {
    args.out[o] = outs[o < outputs ? o : 0];
    args.b[o] = bs[o < outputs ? o : 0];
    bits |= (uintptr_t)args.out[o] | (uintptr_t)args.b[o];
  }
  const bool aligned = (bits & 15u) == 0;
  if (tiled && groups > 1) return dot_multi_launch<T, kDotMultiTile>(s, t, args, a, a_gs * poly, a_ts * poly, b_ts, aligned, outputs, groups, terms, st);
  return dot_multi_launch<T, 1>(s, t, args, a, a_gs * poly, a_ts * poly, b_ts, aligned, outputs, groups, terms, st);
}

// launch_permute_mac_ntt on R = all rows of the level context with weights[t] = a diagonal [knm][n] in the parent's layout
template <typename T>
hipError_t launch_permute_mac_ntt_level(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const T *const *weights,
                                        const uint64_t *ks, int terms, size_t batch, size_t comps, size_t in_cs, size_t out_cs, const KeyLevel &kl,
                                        hipStream_t st) {
  if (!key_level_ok(s, kl)) return hipErrorInvalidValue;
  MacTermsLevel<T> a{};
  a.split = (unsigned)kl.split;
  a.hole = (unsigned)kl.hole;
  return permute_mac_launch<T>(s, t, a, out, addend, ins, weights, ks, terms, batch, s.nm, comps, in_cs, out_cs, 0, st);
}

#define NFLHIP_LEVEL_ROTATE_INSTANCES(T)                                                                                                       \
  template hipError_t launch_dot_multi_level<T>(const Shape &, const DevTables &, T *const *, const T *, size_t, size_t, const T *const *,      \
                                                size_t, size_t, size_t, int, const KeyLevel &, hipStream_t);                                     \
  template hipError_t launch_permute_mac_ntt_level<T>(const Shape &, const DevTables &, T *, const T *, const T *const *, const T *const *,     \
                                                      const uint64_t *, int, size_t, size_t, size_t, size_t, const KeyLevel &, hipStream_t);
NFLHIP_LEVEL_ROTATE_INSTANCES(uint16_t)
NFLHIP_LEVEL_ROTATE_INSTANCES(uint32_t)
NFLHIP_LEVEL_ROTATE_INSTANCES(uint64_t)
#undef NFLHIP_LEVEL_ROTATE_INSTANCES

}  // namespace nflhip
