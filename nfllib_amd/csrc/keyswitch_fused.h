// keyswitch_fused.h -- the steps that the one-launch kernels k_modup_dot_fused (kernels_keyswitch.hip) and k_tensor_modup_dot_fused
// (kernels_mulrelin.hip) share, over the LDS layout of the former's header comment: Y = the L source rows, B = one work row, Vr = the
// corrections v of every digit as 16-bit words (centred mode only).  A thread touches Y, Vr and B only at its own positions
// j = threadIdx.x + k blockDim.x outside the transforms; the barrier argument is in kernels_keyswitch.hip.  Device code; include after
// modarith.h, dot_reduce.h, baseconv_pos.h and ntt_lds.h.
#pragma once
#include "baseconv_pos.h"
#include "dot_reduce.h"
#include "modarith.h"
#include "ntt_lds.h"

namespace nflhip {

static constexpr int kFusedPos = 4;  // positions per thread: n <= 2048, n / 4 threads clamped to 64 .. 1024

// digit d = rows [s0, s0 + ks) of Y, inverse-transformed: every word to y_i under its own row's record, and v of the digit into Vr
template <typename T>
__device__ __forceinline__ void ks_fused_y_pass(T *Y, uint16_t *Vr, const uint64_t *__restrict__ src, unsigned d, unsigned s0, unsigned ks,
                                                unsigned logn, unsigned n, unsigned centred) {
  for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
    uint64_t flo = 0, fhi = 0;
    for (unsigned i = 0; i < ks; ++i) {
      const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], p = (T)src[4 * i + 2];
      const T y = bc_y<T>(Y[((size_t)(s0 + i) << logn) + j], w, wp, p);
      Y[((size_t)(s0 + i) << logn) + j] = y;
      if (centred) bc_fsum_add(flo, fhi, bc_frac<T>(y, src[4 * i + 3]));
    }
    if (centred) Vr[(size_t)d * n + j] = (uint16_t)bc_fsum_round(flo, fhi);  // v <= ks <= 1024
  }
}

// conv_r of digit d (r not a row of the digit) into B, forward-transformed under p_r; words in [0, 4p) on return, after the barrier
// that orders foreign butterflies before own-position loads
template <typename T>
__device__ __forceinline__ void ks_fused_conv_row(T *B, const T *Y, const uint16_t *Vr, const uint64_t *__restrict__ src, const DotRed<T> &red,
                                                  const Tw<T> *__restrict__ psi_r, unsigned d, unsigned s0, unsigned ks, unsigned r, unsigned nm,
                                                  unsigned logn, unsigned n, unsigned centred, T p) {
  typedef typename DotRed<T>::acc_t acc_t;
  const uint64_t *__restrict__ dst = src + 4 * (size_t)ks, *__restrict__ c = dst + 8 * (size_t)nm + (size_t)r * ks;
  const T qj = (T)dst[8 * r + 1], qj_sh = (T)dst[8 * r + 2];
  for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
    acc_t acc = 0;
    for (unsigned i = 0; i < ks; ++i) {
      acc += (acc_t)Y[((size_t)(s0 + i) << logn) + j] * (acc_t)(T)c[i];
      if ((i + 1) % kDotChunk == 0 && i + 1 < ks) acc = (acc_t)red.reduce(acc);  // a full chunk behind, more to come
    }
    B[j] = bc_finish<T>(red.reduce(acc), centred != 0, centred ? (T)Vr[(size_t)d * n + j] : (T)0, qj, qj_sh, false, (T)0, (T)0, (T)0, p);
  }
  resc_fwd_lds<T>(B, psi_r, logn, p, (T)(2 * p));
  __syncthreads();
}

}  // namespace nflhip
