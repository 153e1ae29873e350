// ntt_lds.h -- whole-row negacyclic transforms in LDS, shared by the one-launch kernels that transform a row they have just
// formed (kernels_rescale.hip k_rescale_ntt_fused, kernels_decompose.hip k_decompose_ntt_fused).  The project's lazy Harvey
// butterflies over the psi table (kernels_generic.hip: merged-twiddle Cooley-Tukey forward, mirrored Gentleman-Sande inverse).
#pragma once
#include "kernels.h"
#include "modarith.h"

namespace nflhip {

// ---------------------------------------------------------------------------
// whole-row transforms in LDS, two stages per barrier (the butterflies and the table walk of kernels_generic.hip
// k_ntt_fwd_lds / k_ntt_inv_lds with logi = logn).  Every pass starts with a barrier; the caller adds the one at the end.
// ---------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void resc_fwd_bfly(T &a, T &b, const Tw<T> w, T p, T p2) {
  const T x = csub<T>(a, p2);                              // [0,4p) -> [0,2p)
  const T m = mul_shoup_lazy<T>(b, w.w, w.wp, p);          // [0,2p)
  a = (T)(x + m);                                          // [0,4p)
  b = (T)(x - m + p2);                                     // [0,4p)
}
template <typename T> __device__ __forceinline__ void resc_inv_bfly(T &a, T &b, const Tw<T> w, T p, T p2) {
  const T u = a, v = b;                                    // [0,2p)
  a = csub<T>((T)(u + v), p2);
  b = mul_shoup_lazy<T>((T)(v - u + p2), w.w, w.wp, p);
}
template <typename T> __device__ __forceinline__ void resc_inv_last(T &a, T &b, const ModConst<T> &c) {  // folds n^-1, canonical
  const T u = a, v = b;
  a = mul_shoup<T>((T)(u + v), c.ninv, c.ninv_sh, c.p);
  b = mul_shoup<T>((T)(v - u + c.p2), c.w1ninv, c.w1ninv_sh, c.p);
}

// forward: canonical (or lazy, below 4p) words in, words below 4p out
template <typename T> __device__ __forceinline__ void resc_fwd_lds(T *sm, const Tw<T> *__restrict__ tw, unsigned logn, T p, T p2) {
  const unsigned n = 1u << logn;
  unsigned s = 0;
  if (logn & 1u) {  // stage 0 alone: one block, half-length n / 2
    __syncthreads();
    const Tw<T> w = tw[1];
    for (unsigned q = threadIdx.x; q < (n >> 1); q += blockDim.x) {
      T a = sm[q], b = sm[q + (n >> 1)];
      resc_fwd_bfly<T>(a, b, w, p, p2);
      sm[q] = a;
      sm[q + (n >> 1)] = b;
    }
    s = 1;
  }
  for (; s < logn; s += 2) {  // stages s and s + 1 on four words a quarter-block apart
    const unsigned lt1 = logn - s - 2u, t1 = 1u << lt1;
    __syncthreads();
    for (unsigned q = threadIdx.x; q < (n >> 2); q += blockDim.x) {
      const unsigned j = q >> lt1, o = q & (t1 - 1u);
      const unsigned base = (j << (lt1 + 2u)) + o;
      T a0 = sm[base], a1 = sm[base + t1], a2 = sm[base + 2u * t1], a3 = sm[base + 3u * t1];
      const Tw<T> w = tw[(1u << s) + j];
      resc_fwd_bfly<T>(a0, a2, w, p, p2);
      resc_fwd_bfly<T>(a1, a3, w, p, p2);
      const Tw<T> w0 = tw[(2u << s) + 2u * j], w1 = tw[(2u << s) + 2u * j + 1u];
      resc_fwd_bfly<T>(a0, a1, w0, p, p2);
      resc_fwd_bfly<T>(a2, a3, w1, p, p2);
      sm[base] = a0;
      sm[base + t1] = a1;
      sm[base + 2u * t1] = a2;
      sm[base + 3u * t1] = a3;
    }
  }
}

// inverse: canonical words in, canonical words out (n^-1 folded into the last stage); logn >= 2
template <typename T> __device__ __forceinline__ void resc_inv_lds(T *sm, const Tw<T> *__restrict__ tw, unsigned logn, const ModConst<T> &c) {
  const unsigned n = 1u << logn;
  const T p = c.p, p2 = c.p2;
  int hi = (int)logn - 1;
  if (logn & 1u) {  // stage logn - 1 alone: n / 2 blocks of two neighbours
    __syncthreads();
    const unsigned m = n >> 1;
    for (unsigned q = threadIdx.x; q < m; q += blockDim.x) {
      T a = sm[2u * q], b = sm[2u * q + 1u];
      resc_inv_bfly<T>(a, b, tw[m + (m - 1u - q)], p, p2);
      sm[2u * q] = a;
      sm[2u * q + 1u] = b;
    }
    --hi;
  }
  for (; hi >= 1; hi -= 2) {  // stages hi and hi - 1
    const unsigned lt1 = logn - (unsigned)hi - 1u, t1 = 1u << lt1;
    const unsigned mh = 1u << hi, ml = mh >> 1;
    __syncthreads();
    for (unsigned q = threadIdx.x; q < (n >> 2); q += blockDim.x) {
      const unsigned j = q >> lt1, o = q & (t1 - 1u);
      const unsigned base = (j << (lt1 + 2u)) + o;
      T a0 = sm[base], a1 = sm[base + t1], a2 = sm[base + 2u * t1], a3 = sm[base + 3u * t1];
      resc_inv_bfly<T>(a0, a1, tw[mh + (mh - 1u - 2u * j)], p, p2);       // -(psi_br[mh + 2j])^-1
      resc_inv_bfly<T>(a2, a3, tw[mh + (mh - 2u - 2u * j)], p, p2);
      if (hi > 1) {
        const Tw<T> w = tw[ml + (ml - 1u - j)];
        resc_inv_bfly<T>(a0, a2, w, p, p2);
        resc_inv_bfly<T>(a1, a3, w, p, p2);
      } else {
        resc_inv_last<T>(a0, a2, c);
        resc_inv_last<T>(a1, a3, c);
      }
      sm[base] = a0;
      sm[base + t1] = a1;
      sm[base + 2u * t1] = a2;
      sm[base + 3u * t1] = a3;
    }
  }
}

}  // namespace nflhip
