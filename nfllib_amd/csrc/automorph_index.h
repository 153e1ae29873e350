// automorph_index.h -- the index maps of the NTT-form Galois automorphisms, shared by kernels_automorph.hip (where they were written)
// and kernels_rotate.hip.  All index arithmetic is 32-bit: 2n divides 2^32, so a product that wraps still has the right residue
// mod 2n.
#pragma once
#include <hip/hip_runtime.h>

namespace nflhip {

static constexpr size_t kNttChunkBytes = 16384;  // staged input chunk of the NTT-form tile plans

__device__ __forceinline__ unsigned aut_rev(unsigned x, unsigned logn) { return __brev(x) >> (32u - logn); }

// source slot of NTT-form output slot j
__device__ __forceinline__ unsigned aut_ntt_src(unsigned j, unsigned k, unsigned logn, unsigned mask2n) {
  return aut_rev(((k * (2u * aut_rev(j, logn) + 1u)) & mask2n) >> 1, logn);
}

static inline unsigned aut_inverse_mod_2n(unsigned k, unsigned mask2n) {  // k odd: Newton's iteration doubles the correct low bits
  unsigned x = k;  // correct to 3 bits
  for (int i = 0; i < 5; ++i) x *= 2u - k * x;
  return x & mask2n;
}

}  // namespace nflhip
