// dot_reduce.h -- the unreduced double-width accumulator of a sum of products and its reduction, shared by kernels_dot.hip (where it
// was written) and kernels_baseconv.hip.  Device code.
//
// The products are accumulated UNREDUCED in a double-width word and reduced once per chunk of kDotChunk terms.
//   The moduli sit two bits below the word (modarith.h), a < p <= 2^(W-2) - 1, so a product is at most (2^(W-2) - 2)^2 =
//   2^(2W-4) - 2^W + 4 and   16 products + a canonical carry-in  <=  2^(2W) - 2^(W+4) + 64 + 2^(W-2)  <  2^(2W):
//   sixteen terms never wrap the accumulator, for 16-, 32- and 64-bit limbs alike.  The carry-in is the addend or the canonical
//   result of the previous chunk.
// Reduction of the accumulator S < 2^(2W) to [0, p), for EVERY modulus with 2^(W-3) < p < 2^(W-2) -- no delta-form fold, so the
// 64-bit moduli past the 92nd (delta >= 2^32) take the same code, from ModConst fields that exist:
//   64-bit limbs: S = hi 2^64 + lo.  hi * (2^64 mod p) by Shoup's multiplication with ModConst::beta / beta_sh, any word hi ->
//     [0, 2p); lo - floor(lo c / 2^64) p with c = floor(2^64 / p) = mu >> 60 (mu = floor(2^124 / p)), any word lo -> [0, 2p);
//     their sum is below 4p < 2^64, two conditional subtractions finish.  (A one-step Barrett quotient from mu alone is up to 13
//     short on a 127-bit sum -- S - q p would not fit the word -- which is why the high word goes through beta instead.)
//   32- / 16-bit limbs: two Barrett rounds with mu = floor(2^(2W-4) / p) in 2W-bit arithmetic.  q1 = ((S >> W) mu) >> (W - 4) is in
//     (S/p - 25, S/p], so r1 = S - q1 p < 25 p < 2^(W+3); q2 = ((r1 >> 4) mu) >> (2W - 8) is in (r1/p - 2, r1/p], r2 = r1 - q2 p
//     < 3p fits the word, two conditional subtractions finish.  Every intermediate product is below 2^(2W-1).
//
#pragma once
#include "modarith.h"
#include "table_types.h"  // ModConst<T>

namespace nflhip {

static constexpr unsigned kDotChunk = 16;  // terms per reduction: the bound above

// the accumulator of a limb width and its reduction
template <typename T> struct DotRed;
template <> struct DotRed<uint64_t> {
  typedef unsigned __int128 acc_t;
  uint64_t p, beta, beta_sh, c;
  __device__ __forceinline__ explicit DotRed(const ModConst<uint64_t> &m) : p(m.p), beta(m.beta), beta_sh(m.beta_sh), c(m.mu >> 60) {}
  __device__ __forceinline__ uint64_t reduce(acc_t s) const {
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const uint64_t x = mul_shoup_lazy<uint64_t>(hi, beta, beta_sh, p);  // hi 2^64 mod p, in [0, 2p)
    const uint64_t y = lo - __umul64hi(lo, c) * p;                      // lo mod p, in [0, 2p)
    return reduce4<uint64_t>(x + y, p);
  }
};
template <> struct DotRed<uint32_t> {
  typedef uint64_t acc_t;
  uint32_t p, mu;
  __device__ __forceinline__ explicit DotRed(const ModConst<uint32_t> &m) : p(m.p), mu(m.mu) {}
  __device__ __forceinline__ uint32_t reduce(acc_t s) const {
    const uint64_t q1 = ((s >> 32) * mu) >> 28;
    const uint64_t r1 = s - q1 * p;                                     // < 25 p < 2^35
    const uint32_t q2 = (uint32_t)(((r1 >> 4) * mu) >> 56);
    return reduce4<uint32_t>((uint32_t)r1 - q2 * p, p);                 // r2 < 3p: the low word is the value
  }
};
template <> struct DotRed<uint16_t> {
  typedef uint32_t acc_t;
  uint32_t p, mu;
  __device__ __forceinline__ explicit DotRed(const ModConst<uint16_t> &m) : p(m.p), mu(m.mu) {}
  __device__ __forceinline__ uint16_t reduce(acc_t s) const {
    const uint32_t q1 = ((s >> 16) * mu) >> 12;
    const uint32_t r1 = s - q1 * p;                                     // < 25 p < 2^19
    const uint32_t q2 = ((r1 >> 4) * mu) >> 24;
    uint32_t r = r1 - q2 * p;                                           // < 3p
    r = r >= 2u * p ? r - 2u * p : r;
    return (uint16_t)(r >= p ? r - p : r);
  }
};

}  // namespace nflhip
