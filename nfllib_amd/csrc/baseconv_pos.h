// baseconv_pos.h -- the per-position arithmetic of the RNS base conversion (kernels_baseconv.hip), apart from the kernel's loops and
// addressing so that tests/cpp_baseconv can compile the very same functions for the CPU and check them word for word against the
// Python-integer restatement.  Device code; include after modarith.h and dot_reduce.h.
#pragma once
#include "dot_reduce.h"
#include "modarith.h"

namespace nflhip {

// the fixed-point image of y / p, 60 fraction bits (r: the record's reciprocal word -- floor(2^124 / p) for 64-bit limbs, where the
// image is the high word of the product; floor(2^60 / p) for 32- and 16-bit limbs, where it is the product itself, below 2^60)
template <typename T> __device__ __forceinline__ uint64_t bc_frac(T y, uint64_t r) { return (uint64_t)y * r; }
template <> __device__ __forceinline__ uint64_t bc_frac<uint64_t>(uint64_t y, uint64_t r) { return __umul64hi(y, r); }

static constexpr uint64_t kBcOne = (uint64_t)1 << 60;  // 1.0 in the fixed point of sum f_i

// sum f_i as a 60-bit low part and the count of carries out of it: every f_i is below 2^60, so lo + f is below 2^61 and hi counts
// at most one per term -- no number of terms overflows either word
__device__ __forceinline__ void bc_fsum_add(uint64_t &lo, uint64_t &hi, uint64_t f) {
  lo += f;
  hi += lo >> 60;
  lo &= kBcOne - 1u;
}
// v = floor((sum f_i + 2^59) / 2^60)
__device__ __forceinline__ uint64_t bc_fsum_round(uint64_t lo, uint64_t hi) { return hi + ((lo + (kBcOne >> 1)) >> 60); }

// y_i = x_i (Q/p_i)^-1 mod p_i, canonical
template <typename T> __device__ __forceinline__ T bc_y(T x, T w, T wp, T p) { return mul_shoup<T>(x, w, wp, p); }

// the way out of a destination word: r = (sum_i y_i c_ij) mod p_j canonical; centred: minus v Q_j; down: (x_j - r) P^-1 mod p_j
template <typename T>
__device__ __forceinline__ T bc_finish(T r, bool centred, T v, T qj, T qj_sh, bool down, T xj, T pinv, T pinv_sh, T p) {
  if (centred) r = csub<T>((T)(r + p - mul_shoup<T>(v, qj, qj_sh, p)), p);      // any word v -> v Q_j mod p canonical
  if (down) r = mul_shoup<T>((T)(xj + p - r), pinv, pinv_sh, p);                // both canonical: the difference is in (0, 2p)
  return r;
}

}  // namespace nflhip
