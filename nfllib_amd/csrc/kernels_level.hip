// kernels_level.hip -- the key read of a key switch or a multiplication BELOW the context's top level (include/nflhip.h "leveled key
// switching").  A level-l call runs the plans of kernels_keyswitch.hip and kernels_mulrelin.hip on the child context C_l over the rows
// [0, l) and [L, nm) of its parent -- l + K rows, every table the child's own.  The one thing the child cannot give is the key, which
// stays the ONE top-level key in the parent's layout [dnum_L][2][nm][n]: a polynomial pitch of nm rows, and a hole of L - l rows
// between the child's row l - 1 and its row l (the first special row).  The three kernels that read the key get an instance each that
// knows that layout (KeyLevel, kernels.h): child row r of key[d][c] is at  key + ((2 d + c) knm + r + (r >= split ? hole : 0)) n words.
// r is uniform per workgroup (k_dot: blockIdx.y) or per loop trip (the one-launch kernels), so the hole is a scalar select, and the
// rows [l, L) and the digits >= ceil(l / alpha) of the key are never addressed.
//
// k_dot<T, V, G, DotStrided, DotKeyLevel>  dot_kernel.h: the body of kernels_dot.hip with the key as its second operand, G = 1 and the
//   tiled G = 4 (the key is shared by the batch), 16-byte groups and words.
// k_tensor_modup_dot_fused<T, MrFusedArgsLevel<T>>    mulrelin_fused.h: the kernel of kernels_mulrelin.hip, the layout behind its arguments.
// k_tensor_modup_dot_fused<T, KsFusedArgsLevel<T>>    the same body as the KEY SWITCH's one-launch kernel: the source rows are the input's
//   words and the accumulators start from zero -- the words of k_modup_dot_fused (kernels_keyswitch.hip), whose steps (keyswitch_fused.h)
//   it shares, with the arguments read from the kernel-argument segment where they are used, so that no scalar register is spilled.
// The instances of kernels_dot.hip and kernels_mulrelin.hip are the same templates on the dense layout: a template parameter tells them
// apart, nothing at run time, so they compile to what they compiled to before; kernels_keyswitch.hip is untouched.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"
#include "ntt_lds.h"
#include "dot_kernel.h"
#include "keyswitch_fused.h"
#include "mulrelin_fused.h"

namespace nflhip {

static bool key_level_ok(const Shape &s, const KeyLevel &kl) {  // the child's rows lie inside a parent polynomial
  return kl.split >= 1 && kl.split < s.nm && kl.knm == s.nm + kl.hole && kl.knm <= 65535;
}

template <typename T>
hipError_t launch_dot_key_level(const Shape &s, const DevTables &t, T *out, const T *a, size_t a_gs, size_t a_ts, const T *key, const T *addend,
                                size_t groups, size_t terms, int tiled, const KeyLevel &kl, hipStream_t st) {
  if (!key_level_ok(s, kl)) return hipErrorInvalidValue;
  const size_t poly = s.nm * s.n;
  const DotStrided<T> x = {a, a_gs * poly, a_ts * poly};
  const DotKeyLevel<T> y = {key, 2 * kl.knm * s.n, kl.hole * s.n, (unsigned)kl.split};  // key[d][c]: two parent polynomials per term
  const bool aligned = (((uintptr_t)out | (uintptr_t)a | (uintptr_t)key | (uintptr_t)addend) & 15u) == 0;
  if (tiled && groups > 1) return dot_launch<T, kDotTile>(s, t, out, x, y, addend, aligned, groups, terms, st);
  return dot_launch<T, 1>(s, t, out, x, y, addend, aligned, groups, terms, st);
}

template <typename T>
hipError_t launch_modup_dot_fused_level(const Shape &s, const DevTables &t, T *acc, const T *in, const T *key, const uint64_t *const *recs,
                                        size_t batch, size_t L, size_t alpha, int centred, const KeyLevel &kl, hipStream_t st) {
  if (!recs || !acc || !in || !key || L == 0 || L >= s.nm || alpha == 0 || alpha > L || s.nm > 65535) return hipErrorInvalidValue;
  if (!key_level_ok(s, kl) || kl.split != L) return hipErrorInvalidValue;
  const size_t dnum = (L + alpha - 1) / alpha, lds = keyswitch_fused_lds(L, dnum, s.n, sizeof(T), centred);
  if (!keyswitch_fused_fits(L, dnum, s.n, sizeof(T), centred)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;  // n <= 2048: at most kFusedPos positions per thread
  const size_t cap = (size_t)1 << 20;
  const KsFusedArgsLevel<T> args = {{{acc, in, in, in, in, key, (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, recs, nullptr, batch,
                                      (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha, (unsigned)dnum, centred ? 1u : 0u},
                                     (unsigned)kl.knm, (unsigned)kl.split, (unsigned)kl.hole}};
  hipLaunchKernelGGL((k_tensor_modup_dot_fused<T, KsFusedArgsLevel<T>>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, args);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_tensor_modup_dot_fused_level(const Shape &s, const DevTables &t, T *acc, const T *a0, const T *a1, const T *b0, const T *b1,
                                               const T *key, const uint64_t *const *recs, const uint64_t *pi, size_t batch, size_t L, size_t alpha,
                                               int centred, const KeyLevel &kl, hipStream_t st) {
  if (!recs || !pi || !acc || !a0 || !a1 || !key || !b0 != !b1) return hipErrorInvalidValue;
  if (L == 0 || L >= s.nm || alpha == 0 || alpha > L || s.nm > 65535) return hipErrorInvalidValue;
  if (!key_level_ok(s, kl) || kl.split != L) return hipErrorInvalidValue;
  const size_t dnum = (L + alpha - 1) / alpha, lds = keyswitch_fused_lds(L, dnum, s.n, sizeof(T), centred);
  if (!keyswitch_fused_fits(L, dnum, s.n, sizeof(T), centred)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;  // n <= 2048: at most kFusedPos positions per thread
  const size_t cap = (size_t)1 << 20;
  const MrFusedArgsLevel<T> args = {{acc, a0, a1, b0 ? b0 : a0, b1 ? b1 : a1, key, (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, recs, pi, batch,
                                     (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha, (unsigned)dnum, centred ? 1u : 0u},
                                    (unsigned)kl.knm, (unsigned)kl.split, (unsigned)kl.hole};
  hipLaunchKernelGGL((k_tensor_modup_dot_fused<T, MrFusedArgsLevel<T>>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, args);
  return hipGetLastError();
}

#define NFLHIP_LEVEL_INSTANCES(T)                                                                                                               \
  template hipError_t launch_dot_key_level<T>(const Shape &, const DevTables &, T *, const T *, size_t, size_t, const T *, const T *, size_t,  \
                                              size_t, int, const KeyLevel &, hipStream_t);                                                     \
  template hipError_t launch_modup_dot_fused_level<T>(const Shape &, const DevTables &, T *, const T *, const T *, const uint64_t *const *,    \
                                                      size_t, size_t, size_t, int, const KeyLevel &, hipStream_t);                             \
  template hipError_t launch_tensor_modup_dot_fused_level<T>(const Shape &, const DevTables &, T *, const T *, const T *, const T *, const T *, \
                                                             const T *, const uint64_t *const *, const uint64_t *, size_t, size_t, size_t,     \
                                                             int, const KeyLevel &, hipStream_t);
NFLHIP_LEVEL_INSTANCES(uint16_t)
NFLHIP_LEVEL_INSTANCES(uint32_t)
NFLHIP_LEVEL_INSTANCES(uint64_t)
#undef NFLHIP_LEVEL_INSTANCES

}  // namespace nflhip
