// kernels_bsgs.hip -- the kernels of the baby-step giant-step slot linear transform (include/nflhip.h "BSGS slot linear transforms",
// "weighted sums of automorphisms into several outputs"; api.hip bsgs_run).  Two templates of permute_mac_multi_kernel.h get their
// instances here:
//
// k_permute_mac_multi_ntt<T, VEC, JB, Terms>  out_o = addend_o + sum_t w_{o,t} (.) sigma^NTT_{k_t}(in_t) for JB outputs per launch that
//   share the inputs and the multipliers: the inner sums V_j of n2 giant steps over the SAME key-switch sums S_i.  k_permute_mac_ntt's
//   tile plan (kernels_lintrans.hip): a workgroup owns an output tile position, stages term t's one source chunk in LDS once, reads it
//   permuted once per word -- the two bit reversals and the multiplication of aut_ntt_src are paid once, not per output -- and
//   multiplies that word by the weights of the JB outputs into JB sets of unreduced accumulators (dot_reduce.h); one reduction per
//   output after the last term.  A NULL weight (the zero diagonal) is skipped by a scalar branch.  One staging buffer (DESIGN.md 5.18
//   measured two slower).  blockIdx.y is the component.  The host loops over groups of JB outputs (NFLHIP_MAC_MULTI_JB, DESIGN.md
//   5.23).  Terms: MacMultiTerms on the dense layout, MacMultiTermsLevel on diagonals in the parent context's layout
//   (kernels_level_rotate.hip), three limb widths x (16-byte groups, words) each.
// k_permute_sum_ntt<T, VEC>  out = addend + sum_t sigma^NTT_{k_t}(in_t): the giant step's permutation, accumulated into the sums that
//   the one mod-down closes.  No weight, so a modular addition per term and no wide accumulator.  Internal: no public entry.
#include "kernels.h"
#include "permute_mac_multi_kernel.h"

namespace nflhip {

template <typename T>
hipError_t launch_permute_mac_multi_ntt(const Shape &s, const DevTables &t, T *const *outs, const T *const *addends, const T *const *ins,
                                        const T *const *weights, const uint64_t *ks, int outputs, int terms, size_t batch, size_t R, size_t comps,
                                        size_t in_cs, size_t out_cs, hipStream_t st) {
  return permute_mac_multi_launch<T>(s, t, MacMultiTerms<T, kMacMultiJB>{}, outs, addends, ins, weights, ks, outputs, terms, batch, R, comps, in_cs,
                                     out_cs, st);
}

// on R = all rows of the level context with every weight a diagonal [knm][n] in the parent's layout
template <typename T>
hipError_t launch_permute_mac_multi_ntt_level(const Shape &s, const DevTables &t, T *const *outs, const T *const *addends, const T *const *ins,
                                              const T *const *weights, const uint64_t *ks, int outputs, int terms, size_t batch, size_t comps,
                                              size_t in_cs, size_t out_cs, const KeyLevel &kl, hipStream_t st) {
  if (!(kl.split >= 1 && kl.split < s.nm && kl.knm == s.nm + kl.hole && kl.knm <= 65535)) return hipErrorInvalidValue;
  MacMultiTermsLevel<T, kMacMultiJB> a{};
  a.split = (unsigned)kl.split;
  a.hole = (unsigned)kl.hole;
  return permute_mac_multi_launch<T>(s, t, a, outs, addends, ins, weights, ks, outputs, terms, batch, s.nm, comps, in_cs, out_cs, st);
}

template <typename T>
hipError_t launch_permute_sum_ntt(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const uint64_t *ks, int terms,
                                  size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs, hipStream_t st) {
  return permute_sum_launch<T>(s, t, out, addend, ins, ks, terms, batch, R, comps, in_cs, out_cs, st);
}

#define NFLHIP_BSGS_INSTANCES(T)                                                                                                                  \
  template hipError_t launch_permute_mac_multi_ntt<T>(const Shape &, const DevTables &, T *const *, const T *const *, const T *const *,            \
                                                      const T *const *, const uint64_t *, int, int, size_t, size_t, size_t, size_t, size_t,         \
                                                      hipStream_t);                                                                                 \
  template hipError_t launch_permute_mac_multi_ntt_level<T>(const Shape &, const DevTables &, T *const *, const T *const *, const T *const *,      \
                                                            const T *const *, const uint64_t *, int, int, size_t, size_t, size_t, size_t,           \
                                                            const KeyLevel &, hipStream_t);                                                         \
  template hipError_t launch_permute_sum_ntt<T>(const Shape &, const DevTables &, T *, const T *, const T *const *, const uint64_t *, int, size_t, \
                                                size_t, size_t, size_t, size_t, hipStream_t);
NFLHIP_BSGS_INSTANCES(uint16_t)
NFLHIP_BSGS_INSTANCES(uint32_t)
NFLHIP_BSGS_INSTANCES(uint64_t)
#undef NFLHIP_BSGS_INSTANCES

}  // namespace nflhip
