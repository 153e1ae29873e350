// kernels_lintrans.hip -- the weighted sum of NTT-form automorphisms (include/nflhip.h "weighted sums of automorphisms"):
//   out[g][j][i] = addend[g][j][i] + sum_{t < terms} w_t[j][i] * in_t[g][j][src_{k_t}(i)]   mod p_j, canonical,
// on [batch][R][n] word blocks in the dense layout over the first R moduli of the context, src_k = aut_ntt_src (out[i] = in[src_k(i)]
// is what kernels_automorph.hip writes in NTT form); w_t = [>= R][n] with row stride n, shared by the batch.  The step of a slot
// linear transform that multiplies the key-switch sums by the plaintext diagonals and adds them up before the one mod-down.
//
// The tile plan of k_permute_add_ntt (kernels_rotate.hip) turned round: a workgroup owns an OUTPUT tile -- a chunk of C = n / 2^b
// slots of one row, at most kNttChunkBytes, or several whole rows when a row is shorter -- and a thread owns fixed 16-byte groups of
// it (words in the word variant) with one unreduced double-width accumulator per word (dot_reduce.h).  Per term the workgroup stages
// the ONE source chunk that fills its tile (aut_ntt_src(first slot, k_t) >> chunk_log: an odd multiplier keeps the low bits of the
// exponent, which are the high bits of the slot index, so chunks map one to one) in LDS with 16-byte loads, reads it permuted and
// multiplies by w_t's words, loaded coalesced at the output positions.  After the last term: one reduction, the addend added mod
// p_j, 16-byte stores.  Every input and weight word is read once, every output word written once.
// One staging buffer, two barriers per term, is what serves (LDS <= kNttChunkBytes).  DB: two staging buffers -- the loads of term
// t + 1 are issued into registers before term t is consumed and written to the other buffer after it, one barrier per term; it
// measured 20 - 30 % SLOWER (more registers and twice the LDS cost more than the overlap gains) and is kept behind
// NFLHIP_MAC_DOUBLE_BUFFER as the measured alternative.
// blockIdx.y is the component of a call on several (in, out, addend) sets a fixed stride apart that share ks and weights.
// The kernel and its launcher are in permute_mac_kernel.h; this file holds the instances on the dense layout.
#include "kernels.h"
#include "permute_mac_kernel.h"

namespace nflhip {

template <typename T>
hipError_t launch_permute_mac_ntt(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const T *const *weights,
                                  const uint64_t *ks, int terms, size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs,
                                  int double_buffer, hipStream_t st) {
  return permute_mac_launch<T>(s, t, MacTerms<T>{}, out, addend, ins, weights, ks, terms, batch, R, comps, in_cs, out_cs, double_buffer, st);
}

#define NFLHIP_LINTRANS_INSTANCES(T)                                                                                                  \
  template hipError_t launch_permute_mac_ntt<T>(const Shape &, const DevTables &, T *, const T *, const T *const *, const T *const *, \
                                                const uint64_t *, int, size_t, size_t, size_t, size_t, size_t, int, hipStream_t);
NFLHIP_LINTRANS_INSTANCES(uint16_t)
NFLHIP_LINTRANS_INSTANCES(uint32_t)
NFLHIP_LINTRANS_INSTANCES(uint64_t)
#undef NFLHIP_LINTRANS_INSTANCES

__global__ void k_warm_lintrans() {}
hipError_t warm_lintrans(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_lintrans, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
