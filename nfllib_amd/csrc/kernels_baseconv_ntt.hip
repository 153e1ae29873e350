// kernels_baseconv_ntt.hip -- the RNS base conversion and the mod-down by the last k moduli on NTT-form data (include/nflhip.h
// "RNS base conversion, NTT form").  The conversion itself only exists in coefficient form (kernels_baseconv.hip), so
//   mod-up    out row j = NTT_j(conv_j(INTT_i(in row i), i in S))                       for j in D \ S; rows of D in S are the input's
//   mod-down  Y_j = (x_j - NTT_j(conv_j(INTT_i(in row i), i in the last k rows))) P^-1 mod p_j, x_j the NTT-form input row
// with conv exactly the map of k_baseconv: every per-position step is a function of baseconv_pos.h / dot_reduce.h, so the words
// behind the transforms are those of the coefficient path.
//
// Plans:
//   fused  -- ONE launch: a workgroup owns one polynomial and loops over the batch.  LDS holds the ks source rows (first the
//             NTT-form words, then their inverse transforms, then y_i), one work row B and, in centred mode, a row of v:
//                 (ks + 1 + c) n sizeof(T) <= 64 KiB,   c = 1 centred, 0 fast            (baseconv_ntt_fused_lds, kernels.h)
//             Per destination row the canonical conv_j is formed in B, forward-transformed under p_j and stored (mod-up) or
//             combined with x_j (mod-down).  ks rows read, |D \ S| written (+ kd read for the mod-down), no scratch.
//             The transforms are those of ntt_lds.h (kernels_rescale.hip k_rescale_ntt_fused).
//   stream -- k_moddown_ntt_combine, the element-wise tail of the composed mod-down (api.hip baseconv_ntt_composed):
//             out row j = (in row j - out row j) P^-1 mod p_j.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"
#include "ntt_lds.h"

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) BcnVec { T e[V]; };

// mode bit 0: centred conversion; bit 1: mod-down (out is the dense [batch][kd][n]); bit 2: in place (out == in): a destination
// row that is a source row is left alone -- out of place it is copied.  out and in may be the same buffer: no __restrict__.
template <typename T>
__global__ void __launch_bounds__(1024) k_bconv_ntt_fused(T *out, const T *in, const Tw<T> *__restrict__ psi, const ModConst<T> *__restrict__ mc,
                                                          const uint64_t *__restrict__ rec, unsigned logn, unsigned nm, unsigned onm, unsigned s0,
                                                          unsigned ks, unsigned d0, unsigned kd, unsigned mode, size_t batch) {
  typedef typename DotRed<T>::acc_t acc_t;
  extern __shared__ uint4 bcn_lds_raw[];
  const unsigned n = 1u << logn;
  T *Y = reinterpret_cast<T *>(bcn_lds_raw), *B = Y + ((size_t)ks << logn), *Vr = B + n;  // (Vr only exists in centred mode)
  const bool centred = (mode & 1u) != 0, down = (mode & 2u) != 0, inplace = (mode & 4u) != 0;
  const uint64_t *__restrict__ src = rec, *__restrict__ dst = rec + 4 * (size_t)ks, *__restrict__ cm = dst + 8 * (size_t)kd;
  for (size_t b = blockIdx.x; b < batch; b += gridDim.x) {
    const T *x = in + ((b * nm) << logn);
    T *o = out + ((b * onm) << logn);
    // every source row into LDS and through its inverse transform.  A row's loads are ordered before its butterflies by the
    // transform's first barrier, and the rows do not share a word.
    for (unsigned i = 0; i < ks; ++i) {
      T *Yi = Y + ((size_t)i << logn);
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x) Yi[j] = x[((size_t)(s0 + i) << logn) + j];
      const ModConst<T> ci = mc[s0 + i];
      resc_inv_lds<T>(Yi, psi + ((size_t)(s0 + i) << logn), logn, ci);
    }
    __syncthreads();
    // from here to the end of the polynomial a thread touches Y and Vr only at its own indices j
    for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
      uint64_t flo = 0, fhi = 0;
      for (unsigned i = 0; i < ks; ++i) {
        const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], p = (T)src[4 * i + 2];
        const T y = bc_y<T>(Y[((size_t)i << logn) + j], w, wp, p);
        Y[((size_t)i << logn) + j] = y;
        if (centred) bc_fsum_add(flo, fhi, bc_frac<T>(y, src[4 * i + 3]));
      }
      if (centred) Vr[j] = (T)bc_fsum_round(flo, fhi);
    }
    for (unsigned jj = 0; jj < kd; ++jj) {
      const unsigned r = d0 + jj;
      if (!down && r - s0 < ks) {  // (unsigned: s0 <= r < s0 + ks) the conversion of a source row is the row itself
        if (!inplace)
          for (unsigned j = threadIdx.x; j < n; j += blockDim.x) o[((size_t)r << logn) + j] = x[((size_t)r << logn) + j];
        continue;
      }
      const DotRed<T> red(mc[r]);
      const T p = (T)dst[8 * jj], qj = (T)dst[8 * jj + 1], qj_sh = (T)dst[8 * jj + 2], pinv = (T)dst[8 * jj + 3], pinv_sh = (T)dst[8 * jj + 4];
      const uint64_t *__restrict__ c = cm + (size_t)jj * ks;
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
        acc_t acc = 0;
        for (unsigned i = 0; i < ks; ++i) {
          acc += (acc_t)Y[((size_t)i << logn) + j] * (acc_t)(T)c[i];
          if ((i + 1) % kDotChunk == 0 && i + 1 < ks) acc = (acc_t)red.reduce(acc);  // a full chunk behind, more to come
        }
        // (the conversion alone: the mod-down's difference is taken after the transform, against the NTT-form x_j)
        B[j] = bc_finish<T>(red.reduce(acc), centred, centred ? Vr[j] : (T)0, qj, qj_sh, false, (T)0, (T)0, (T)0, p);
      }
      resc_fwd_lds<T>(B, psi + ((size_t)r << logn), logn, p, (T)(2 * p));
      __syncthreads();
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
        const T t = reduce4<T>(B[j], p);
        o[((size_t)r << logn) + j] = down ? mul_shoup<T>((T)(x[((size_t)r << logn) + j] + p - t), pinv, pinv_sh, p) : t;  // in (0, 2p)
      }
      // (B[j] is rewritten next by the thread that just read it; the transform's first barrier orders the rest)
    }
    __syncthreads();  // the next polynomial's loads overwrite Y
  }
}

// the composed mod-down's last pass: out row j = (in row j + p_j - out row j) P^-1 mod p_j, in = [batch][nm][n] NTT form, out the
// dense [batch][kd][n] holding the forward-transformed conversion (canonical).  A thread owns one 16-byte group of positions of one
// polynomial (V = 1: the word variant for misaligned pointers and short rows) and walks the kept rows four at a time.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_moddown_ntt_combine(T *__restrict__ out, const T *__restrict__ in, const uint64_t *__restrict__ dst,
                                                             unsigned logn, unsigned nm, unsigned kd, unsigned logv, size_t total) {
  typedef BcnVec<T, V> Vec;
  constexpr unsigned U = 4;
  const unsigned lv = logn - logv;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t b = t >> lv, pos = (t & ((((size_t)1) << lv) - 1u)) << logv;
    const T *x = in + ((b * nm) << logn) + pos;
    T *o = out + ((b * kd) << logn) + pos;
    for (unsigned j0 = 0; j0 < kd; j0 += U) {
      Vec xv[U], yv[U];
#pragma unroll
      for (unsigned u = 0; u < U; ++u)
        if (j0 + u < kd) {
          xv[u] = *reinterpret_cast<const Vec *>(x + ((size_t)(j0 + u) << logn));
          yv[u] = *reinterpret_cast<const Vec *>(o + ((size_t)(j0 + u) << logn));
        }
#pragma unroll
      for (unsigned u = 0; u < U; ++u)
        if (j0 + u < kd) {
          const uint64_t *__restrict__ d = dst + 8 * (size_t)(j0 + u);
          const T p = (T)d[0], pinv = (T)d[3], pinv_sh = (T)d[4];
          Vec w;
#pragma unroll
          for (int k = 0; k < V; ++k) w.e[k] = mul_shoup<T>((T)(xv[u].e[k] + p - yv[u].e[k]), pinv, pinv_sh, p);  // both canonical: in (0, 2p)
          *reinterpret_cast<Vec *>(o + ((size_t)(j0 + u) << logn)) = w;
        }
    }
  }
}

template <typename T>
hipError_t launch_baseconv_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t s0,
                                     size_t ks, size_t d0, size_t kd, int centred, int moddown, hipStream_t st) {
  if (!rec || ks == 0 || kd == 0 || s0 + ks > s.nm || d0 + kd > s.nm || s.nm > 65535) return hipErrorInvalidValue;
  if (moddown && (d0 != 0 || kd != s0 || s0 + ks != s.nm)) return hipErrorInvalidValue;
  const size_t lds = baseconv_ntt_fused_lds(ks, s.n, sizeof(T), centred);
  if (lds > kBaseconvNttLdsBytes || s.logn < 2) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;
  const size_t cap = (size_t)1 << 20;
  const unsigned mode = (centred ? 1u : 0u) | (moddown ? 2u : 0u) | (!moddown && (const T *)out == in ? 4u : 0u), onm = (unsigned)(moddown ? kd : s.nm);
  hipLaunchKernelGGL((k_bconv_ntt_fused<T>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, out, in,
                     (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, rec, (unsigned)s.logn, (unsigned)s.nm, onm, (unsigned)s0, (unsigned)ks,
                     (unsigned)d0, (unsigned)kd, mode, batch);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_moddown_ntt_combine(const Shape &s, T *out, const T *in, const uint64_t *rec, size_t batch, size_t k, hipStream_t st) {
  if (!rec || k == 0 || k >= s.nm || s.nm > 65535) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;  // grid-stride, four workgroups per CU at most (kernels_rescale.hip)
  const uint64_t *dst = rec + 4 * k;  // the record's destination part (host_tables.h)
  const dim3 g((unsigned)blocks), bl(256);
  if (vec) hipLaunchKernelGGL((k_moddown_ntt_combine<T, V>), g, bl, 0, st, out, in, dst, (unsigned)s.logn, (unsigned)s.nm, (unsigned)(s.nm - k), logv, total);
  else hipLaunchKernelGGL((k_moddown_ntt_combine<T, 1>), g, bl, 0, st, out, in, dst, (unsigned)s.logn, (unsigned)s.nm, (unsigned)(s.nm - k), logv, total);
  return hipGetLastError();
}

#define NFLHIP_BASECONV_NTT_INSTANCES(T)                                                                                                     \
  template hipError_t launch_baseconv_ntt_fused<T>(const Shape &, const DevTables &, T *, const T *, const uint64_t *, size_t, size_t, size_t, \
                                                   size_t, size_t, int, int, hipStream_t);                                                   \
  template hipError_t launch_moddown_ntt_combine<T>(const Shape &, T *, const T *, const uint64_t *, size_t, size_t, hipStream_t);
NFLHIP_BASECONV_NTT_INSTANCES(uint16_t)
NFLHIP_BASECONV_NTT_INSTANCES(uint32_t)
NFLHIP_BASECONV_NTT_INSTANCES(uint64_t)
#undef NFLHIP_BASECONV_NTT_INSTANCES

__global__ void k_warm_bconv_ntt() {}
hipError_t warm_baseconv_ntt(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_bconv_ntt, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
