// kernels_keyswitch.hip -- hybrid (RNS-digit) key switching on NTT-form data (include/nflhip.h "hybrid key switching").
//
// in = [batch][L][n], the first L rows of a context of nm moduli; digits S_d = [d alpha, min((d + 1) alpha, L)), dnum of them.  Per
// digit the mod-up U_d is the base conversion of rows S_d to every row of the context (kernels_baseconv.hip: y_i, sum_i y_i c_ij,
// the centred correction v Q_j), with the record of the pair (S_d) -> (0, nm) that build_baseconv_record computes for
// nflhip_baseconv_ntt_dev: recs[d].  Every per-position step is a function of baseconv_pos.h / dot_reduce.h, so the words are those
// of that entry.  For j in S_d the conversion is x_j itself (c_ij = 0 for i != j in S_d, y_j (Q/p_j) = x_j, Q_j = 0).
//
// k_modup_digits<T, V, K> -- the composed plan's streaming pass, coefficient form in and out.  A thread owns one 16-byte group of
//   positions of one polynomial (V words; V = 1: the word variant for misaligned pointers and rows shorter than 16 bytes) and walks
//   the digits: per digit it reads the digit's source words ONCE (K = 4, 16: |S_d| <= K, all in registers; K = 0: any alpha, the
//   sources are read again per destination row in chunks of 16 with the canonical partial sum carried, as k_baseconv's K = 0 plan),
//   forms y_i and sum f_i, and writes every row of U_d into out = [batch][dnum][nm][n]; rows j in S_d are written as x_j, so that the
//   forward transform returns the input's words.  L rows read, dnum nm rows written.  Sums unreduced, one reduction per kDotChunk
//   terms.  The records and ModConst are indexed by loop counters only: scalar loads.  256 threads, grid-stride, no LDS.
//
// k_modup_dot_fused<T> -- ONE launch from the NTT-form input to the two sums acc_c = sum_d U_d key[d][c] (NTT form, canonical).  A
//   workgroup owns one polynomial and loops over the batch; n / 4 threads clamped to 64 .. 1024, rows of at most 2048 words, so a
//   thread owns at most kFusedPos = 4 positions j = threadIdx.x + k blockDim.x.  LDS: Y = the L source rows (the NTT-form words, then
//   their inverse transforms, then y_i under the row's own digit -- y_i depends on no other digit), one work row B and, in centred
//   mode, v of every digit as 16-bit words (v <= alpha <= 1024):
//       (L + 1) n sizeof(T) + [centred] 2 dnum n  <=  64 KiB                                  (keyswitch_fused_lds, kernels.h)
//   Per destination row j the two accumulators of a position live in registers (acc_t, one reduction per kDotChunk digits); per
//   digit the term is the NTT-form input word x_j re-read from global memory when j is in S_d, else the canonical conv_j formed in B,
//   forward-transformed under p_j and reduced.  L rows and the key (once per polynomial) read, 2 nm rows written:
//   acc = [2][batch][nm][n], component-major, so that one mod-down of 2 batch polynomials lands in out0 then out1.
//   Barriers: outside the transforms a thread touches Y, V and B only at its own positions.  After the inverse transforms one
//   barrier orders their last butterflies before the y_i pass; that pass and every conv_j pass read and write own positions only.
//   resc_fwd_lds starts with a barrier (own-position stores of B before foreign butterflies) and is followed by one (foreign
//   butterflies before own-position loads); the next conv_j store into B[j] is by the thread that just read B[j], and the next
//   transform's first barrier orders it before anything else.  The barrier at the end of a polynomial orders the last reads of Y
//   before the next polynomial's loads.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"
#include "ntt_lds.h"
#include "keyswitch_fused.h"  // kFusedPos and the steps k_modup_dot_fused shares with kernels_mulrelin.hip

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) KsVec { T e[V]; };
struct alignas(32) KsSrc { uint64_t w, wp, p, r; };  // a source row's record (host_tables.h)

template <typename T, int V, int K>
__global__ void __launch_bounds__(256) k_modup_digits(T *__restrict__ out, const T *__restrict__ in, const ModConst<T> *__restrict__ mc,
                                                      const uint64_t *const *__restrict__ recs, unsigned logn, unsigned nm, unsigned L_arg,
                                                      unsigned alpha_arg, unsigned dnum_arg, unsigned centred_arg, size_t total) {
  typedef KsVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr int KR = K > 0 ? K : 1;
  constexpr unsigned logv = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : 3;
  const unsigned lv = logn - logv;  // log2 of the groups per row
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t b = t >> lv, pos = (t & ((((size_t)1) << lv) - 1u)) << logv;
    // the loop-invariant guards and offsets as values of THIS iteration, as k_baseconv: hoisted out of the grid-stride loop they
    // would all be live at once (tests/test_keyswitch_cpu.py reads the compiler's resource report of this file)
    unsigned L = L_arg, alpha = alpha_arg, dnum = dnum_arg, centred = centred_arg, lg = logn;
    asm volatile("" : "+s"(L), "+s"(alpha), "+s"(dnum), "+s"(centred), "+s"(lg));
    const T *x = in + ((b * L) << lg) + pos;
    for (unsigned d = 0; d < dnum; ++d) {
      const unsigned s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
      const uint64_t *__restrict__ src = recs[d];
      const uint64_t *__restrict__ dst = src + 4 * (size_t)ks, *__restrict__ cm = dst + 8 * (size_t)nm;
      T *o = out + (((b * dnum + d) * nm) << lg) + pos;
      uint64_t flo[V], fhi[V];
#pragma unroll
      for (int k = 0; k < V; ++k) flo[k] = fhi[k] = 0;
      T y[KR][V];
      Vec xv[KR];
      if (K > 0) {
#pragma unroll
        for (int i = 0; i < K; ++i)
          if ((unsigned)i < ks) xv[i] = *reinterpret_cast<const Vec *>(x + ((size_t)(s0 + i) << lg));
#pragma unroll
        for (int i = 0; i < K; ++i)
          if ((unsigned)i < ks) {
            const KsSrc rc = reinterpret_cast<const KsSrc *>(src)[i];  // one 32-byte scalar load
#pragma unroll
            for (int k = 0; k < V; ++k) {
              y[i][k] = bc_y<T>(xv[i].e[k], (T)rc.w, (T)rc.wp, (T)rc.p);
              if (centred) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(y[i][k], rc.r));
            }
          }
      } else if (centred) {
        for (unsigned i = 0; i < ks; ++i) {
          const Vec xi = *reinterpret_cast<const Vec *>(x + ((size_t)(s0 + i) << lg));
          const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], p = (T)src[4 * i + 2];
          const uint64_t r = src[4 * i + 3];
#pragma unroll
          for (int k = 0; k < V; ++k) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(bc_y<T>(xi.e[k], w, wp, p), r));
        }
      }
      T v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = (T)bc_fsum_round(flo[k], fhi[k]);
      for (unsigned j = 0; j < nm; ++j) {
        if (j - s0 < ks) {  // (unsigned: s0 <= j < s0 + ks) a row of the digit: the input's words
          *reinterpret_cast<Vec *>(o + ((size_t)j << lg)) = *reinterpret_cast<const Vec *>(x + ((size_t)j << lg));
          continue;
        }
        const DotRed<T> red(mc[j]);
        const T p = (T)dst[8 * j];
        const uint64_t *__restrict__ c = cm + (size_t)j * ks;
        acc_t acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0;
        if (K > 0) {
#pragma unroll
          for (int i = 0; i < K; ++i)  // K <= kDotChunk terms: no reduction on the way
            if ((unsigned)i < ks) {
              const T cij = (T)c[i];
#pragma unroll
              for (int k = 0; k < V; ++k) acc[k] += (acc_t)y[i][k] * (acc_t)cij;
            }
        } else {
          for (unsigned i = 0; i < ks; ++i) {
            const Vec xi = *reinterpret_cast<const Vec *>(x + ((size_t)(s0 + i) << lg));
            const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], pi = (T)src[4 * i + 2], cij = (T)c[i];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += (acc_t)bc_y<T>(xi.e[k], w, wp, pi) * (acc_t)cij;
            if ((i + 1) % kDotChunk == 0 && i + 1 < ks) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
              for (int k = 0; k < V; ++k) acc[k] = (acc_t)red.reduce(acc[k]);
            }
          }
        }
        const T qj = (T)dst[8 * j + 1], qj_sh = (T)dst[8 * j + 2];
        Vec w;
#pragma unroll
        for (int k = 0; k < V; ++k) w.e[k] = bc_finish<T>(red.reduce(acc[k]), centred != 0, v[k], qj, qj_sh, false, (T)0, (T)0, (T)0, p);
        *reinterpret_cast<Vec *>(o + ((size_t)j << lg)) = w;
      }
    }
  }
}

template <typename T, int V>
static void modup_digits_pick(dim3 g, hipStream_t st, T *out, const T *in, const ModConst<T> *mc, const uint64_t *const *recs, unsigned logn,
                              unsigned nm, unsigned L, unsigned alpha, unsigned dnum, unsigned centred, size_t total) {
  const dim3 bl(256);
  if (alpha <= 4) hipLaunchKernelGGL((k_modup_digits<T, V, 4>), g, bl, 0, st, out, in, mc, recs, logn, nm, L, alpha, dnum, centred, total);
  else if (alpha <= 16) hipLaunchKernelGGL((k_modup_digits<T, V, 16>), g, bl, 0, st, out, in, mc, recs, logn, nm, L, alpha, dnum, centred, total);
  else hipLaunchKernelGGL((k_modup_digits<T, V, 0>), g, bl, 0, st, out, in, mc, recs, logn, nm, L, alpha, dnum, centred, total);
}

template <typename T>
hipError_t launch_modup_digits(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *const *recs, size_t batch, size_t L,
                               size_t alpha, int centred, hipStream_t st) {
  if (!recs || L == 0 || L >= s.nm || alpha == 0 || alpha > L || s.nm > 65535 || (const T *)out == in) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv, dnum = (L + alpha - 1) / alpha;
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g((unsigned)blocks);
  if (vec) modup_digits_pick<T, V>(g, st, out, in, mc, recs, (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha, (unsigned)dnum, centred ? 1u : 0u, total);
  else modup_digits_pick<T, 1>(g, st, out, in, mc, recs, (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha, (unsigned)dnum, centred ? 1u : 0u, total);
  return hipGetLastError();
}

template <typename T>
__global__ void __launch_bounds__(1024) k_modup_dot_fused(T *__restrict__ accout, const T *__restrict__ in, const T *__restrict__ key,
                                                          const Tw<T> *__restrict__ psi, const ModConst<T> *__restrict__ mc,
                                                          const uint64_t *const *__restrict__ recs, unsigned logn, unsigned nm, unsigned L,
                                                          unsigned alpha, unsigned dnum, unsigned centred, size_t batch) {
  typedef typename DotRed<T>::acc_t acc_t;
  extern __shared__ uint4 ks_lds_raw[];
  const unsigned n = 1u << logn;
  T *Y = reinterpret_cast<T *>(ks_lds_raw), *B = Y + ((size_t)L << logn);
  uint16_t *Vr = reinterpret_cast<uint16_t *>(B + n);  // [dnum][n], centred mode only
  for (size_t b = blockIdx.x; b < batch; b += gridDim.x) {
    const T *x = in + ((b * L) << logn);
    T *o0 = accout + ((b * nm) << logn), *o1 = accout + (((batch + b) * nm) << logn);
    // every source row into LDS and through its inverse transform.  A row's loads are ordered before its butterflies by the
    // transform's first barrier, and the rows do not share a word.
    for (unsigned i = 0; i < L; ++i) {
      T *Yi = Y + ((size_t)i << logn);
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x) Yi[j] = x[((size_t)i << logn) + j];
      const ModConst<T> ci = mc[i];
      resc_inv_lds<T>(Yi, psi + ((size_t)i << logn), logn, ci);
    }
    __syncthreads();
    // from here to the end of the polynomial a thread touches Y, Vr and B only at its own positions outside the transforms
    for (unsigned d = 0; d < dnum; ++d) {
      const unsigned s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
      ks_fused_y_pass<T>(Y, Vr, recs[d], d, s0, ks, logn, n, centred);
    }
    for (unsigned r = 0; r < nm; ++r) {
      const ModConst<T> cr = mc[r];
      const DotRed<T> red(cr);
      const T p = (T)cr.p;
      acc_t a0[kFusedPos], a1[kFusedPos];
#pragma unroll
      for (int k = 0; k < kFusedPos; ++k) a0[k] = a1[k] = 0;
      for (unsigned d = 0; d < dnum; ++d) {
        const unsigned s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
        const T *k0 = key + (((size_t)(2 * d) * nm + r) << logn), *k1 = k0 + ((size_t)nm << logn);
        const bool own = r - s0 < ks;  // (unsigned: s0 <= r < s0 + ks) a row of the digit: the NTT-form input word
        if (!own) {
          ks_fused_conv_row<T>(B, Y, Vr, recs[d], red, psi + ((size_t)r << logn), d, s0, ks, r, nm, logn, n, centred, p);
        }
#pragma unroll
        for (int k = 0; k < kFusedPos; ++k) {
          const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
          if (j < n) {
            const T u = own ? x[((size_t)r << logn) + j] : reduce4<T>(B[j], p);
            a0[k] += (acc_t)u * (acc_t)k0[j];
            a1[k] += (acc_t)u * (acc_t)k1[j];
          }
        }
        if ((d + 1) % kDotChunk == 0 && d + 1 < dnum) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
          for (int k = 0; k < kFusedPos; ++k) {
            a0[k] = (acc_t)red.reduce(a0[k]);
            a1[k] = (acc_t)red.reduce(a1[k]);
          }
        }
        // (B[j] is rewritten next by the thread that just read it; the transform's first barrier orders the rest)
      }
#pragma unroll
      for (int k = 0; k < kFusedPos; ++k) {
        const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
        if (j < n) {
          o0[((size_t)r << logn) + j] = red.reduce(a0[k]);
          o1[((size_t)r << logn) + j] = red.reduce(a1[k]);
        }
      }
    }
    __syncthreads();  // the next polynomial's loads overwrite Y
  }
}

template <typename T>
hipError_t launch_modup_dot_fused(const Shape &s, const DevTables &t, T *acc, const T *in, const T *key, const uint64_t *const *recs, size_t batch,
                                  size_t L, size_t alpha, int centred, hipStream_t st) {
  if (!recs || L == 0 || L >= s.nm || alpha == 0 || alpha > L || s.nm > 65535) return hipErrorInvalidValue;
  const size_t dnum = (L + alpha - 1) / alpha, lds = keyswitch_fused_lds(L, dnum, s.n, sizeof(T), centred);
  if (!keyswitch_fused_fits(L, dnum, s.n, sizeof(T), centred)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;  // n <= 2048: at most kFusedPos positions per thread
  const size_t cap = (size_t)1 << 20;
  hipLaunchKernelGGL((k_modup_dot_fused<T>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, acc, in, key,
                     (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, recs, (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha,
                     (unsigned)dnum, centred ? 1u : 0u, batch);
  return hipGetLastError();
}

#define NFLHIP_KEYSWITCH_INSTANCES(T)                                                                                                        \
  template hipError_t launch_modup_digits<T>(const Shape &, const DevTables &, T *, const T *, const uint64_t *const *, size_t, size_t, size_t, \
                                             int, hipStream_t);                                                                              \
  template hipError_t launch_modup_dot_fused<T>(const Shape &, const DevTables &, T *, const T *, const T *, const uint64_t *const *, size_t,  \
                                                size_t, size_t, int, hipStream_t);
NFLHIP_KEYSWITCH_INSTANCES(uint16_t)
NFLHIP_KEYSWITCH_INSTANCES(uint32_t)
NFLHIP_KEYSWITCH_INSTANCES(uint64_t)
#undef NFLHIP_KEYSWITCH_INSTANCES

__global__ void k_warm_keyswitch() {}
hipError_t warm_keyswitch(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_keyswitch, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
