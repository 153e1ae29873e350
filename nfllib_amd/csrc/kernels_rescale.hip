// kernels_rescale.hip -- RNS rescale: exact division with rounding by the LAST modulus q = p_L of the chain (L = nm - 1).
//
// For every coefficient position, X in [0, Q) is the integer behind the nm input words; the nm - 1 output words are the
// residues of Y = floor((X + h) / q) mod Q / q, h = (q - 1) / 2 (include/nflhip.h "RNS rescale").  In RNS arithmetic
//   r = (x_L + h) mod q,      y_i = (x_i + h - r) q^-1 mod p_i       (X + h - r is the multiple of q below X + h),
// with r < q < 2 p_i (one bit length per limb width), so one conditional subtraction takes r into row i, and h < p_i.
// Input [batch][nm][n], output the dense [batch][nm - 1][n]: the strides differ, the operands never overlap (api.hip).
//
// Plans:
//   stream -- coefficient form in ONE pass: a thread owns one 16-byte group of coefficient positions of one polynomial, reads
//             the dropped row's words once, and walks the kept rows four loads at a time.  (2 nm - 1) rows of traffic per
//             polynomial.  A word path (one position per thread) serves misaligned pointers and rows shorter than 16 bytes.
//             The same kernel in two other modes is the element-wise part of the composed NTT-form plan (expand, combine).
//   fused  -- NTT form in ONE launch: r only exists in coefficient form, so a workgroup owns one polynomial, inverse-
//             transforms the dropped row in LDS (buffer A) and forms r there; per kept row it writes d_i = (h - r) mod p_i
//             into buffer B, forward-transforms B under p_i and stores (x_i + NTT_i(d_i)) q^-1 mod p_i.  The same
//             (2 nm - 1) rows of traffic, no scratch.  LDS = two rows; rows up to 32 KiB (launch_rescale_ntt_fused; api.hip
//             runs it by default below 32 KiB and the composed plan from there on, profiles/r08_rescale.txt).
//             The transforms are the project's lazy Harvey butterflies over the psi table (kernels_generic.hip: merged-
//             twiddle Cooley-Tukey forward, mirrored Gentleman-Sande inverse), two stages per barrier.
#include "kernels.h"
#include "modarith.h"

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) RescVec { T e[V]; };

// ---------------------------------------------------------------------------
// streaming kernel.  MODE 0: coefficient-form rescale (in -> out).  MODE 1: expand (aux = inverse-transformed dropped rows
// [batch][n] -> out row i = (h - r) mod p_i).  MODE 2: combine (out row i = (in row i + out row i) q^-1 mod p_i).
// ---------------------------------------------------------------------------
template <typename T, int MODE, int V>
__global__ void __launch_bounds__(256) k_rescale_stream(T *__restrict__ out, const T *__restrict__ in, const T *__restrict__ aux,
                                                        const ModConst<T> *__restrict__ mc, const RescConst<T> *__restrict__ rc,
                                                        unsigned logn, unsigned nm, unsigned logv, size_t total) {
  typedef RescVec<T, V> Vec;
  constexpr unsigned U = 4;  // kept rows in flight per thread
  const unsigned kept = nm - 1u;
  const T q = mc[kept].p, h = rc[0].h;
  const unsigned lv = logn - logv;  // log2 of the groups per row
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t b = v >> lv, j = (v & ((((size_t)1) << lv) - 1u)) << logv;
    const T *x = in + ((b * nm) << logn) + j;
    T *o = out + ((b * kept) << logn) + j;
    Vec r;
    if (MODE != 2) {
      const Vec t = MODE == 0 ? *reinterpret_cast<const Vec *>(x + ((size_t)kept << logn))
                              : *reinterpret_cast<const Vec *>(aux + (b << logn) + j);
#pragma unroll
      for (int k = 0; k < V; ++k) r.e[k] = csub<T>((T)(t.e[k] + h), q);
    }
    for (unsigned i0 = 0; i0 < kept; i0 += U) {
      Vec xv[U], yv[U];
#pragma unroll
      for (unsigned u = 0; u < U; ++u) {
        if (i0 + u < kept) {
          if (MODE != 1) xv[u] = *reinterpret_cast<const Vec *>(x + ((size_t)(i0 + u) << logn));
          if (MODE == 2) yv[u] = *reinterpret_cast<const Vec *>(o + ((size_t)(i0 + u) << logn));
        }
      }
#pragma unroll
      for (unsigned u = 0; u < U; ++u) {
        if (i0 + u < kept) {
          const RescConst<T> c = rc[i0 + u];
          Vec w;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            if (MODE == 2) {
              w.e[k] = mul_shoup<T>((T)(xv[u].e[k] + yv[u].e[k]), c.qinv, c.qinv_sh, c.p);  // both canonical: below 2p
            } else {
              const T ri = csub<T>(r.e[k], c.p);
              if (MODE == 1) w.e[k] = (T)(h >= ri ? h - ri : h + c.p - ri);
              else w.e[k] = mul_shoup<T>((T)(xv[u].e[k] + h + c.p - ri), c.qinv, c.qinv_sh, c.p);  // in (0, 3p)
            }
          }
          *reinterpret_cast<Vec *>(o + ((size_t)(i0 + u) << logn)) = w;
        }
      }
    }
  }
}

template <typename T, int MODE>
static hipError_t rescale_stream(const Shape &s, const DevTables &t, T *out, const T *in, const T *aux, size_t batch, hipStream_t st) {
  if (s.nm < 2 || !t.resc) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const uintptr_t align = (uintptr_t)out | (uintptr_t)in | (uintptr_t)aux;
  const bool vec = align % 16 == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  // grid-stride, four 256-thread workgroups per CU at most (kernels_generic.hip stream_blocks: more resident waves only add
  // DRAM page conflicts), every thread with four rows in flight
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const RescConst<T> *rc = (const RescConst<T> *)t.resc;
  const dim3 g((unsigned)blocks), bl(256);
  if (vec) hipLaunchKernelGGL((k_rescale_stream<T, MODE, V>), g, bl, 0, st, out, in, aux, mc, rc, (unsigned)s.logn, (unsigned)s.nm, logv, total);
  else hipLaunchKernelGGL((k_rescale_stream<T, MODE, 1>), g, bl, 0, st, out, in, aux, mc, rc, (unsigned)s.logn, (unsigned)s.nm, logv, total);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_rescale_coeff(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st) {
  return rescale_stream<T, 0>(s, t, out, in, nullptr, batch, st);
}
template <typename T>
hipError_t launch_rescale_expand(const Shape &s, const DevTables &t, T *out, const T *dropped, size_t batch, hipStream_t st) {
  return rescale_stream<T, 1>(s, t, out, out, dropped, batch, st);  // (`in` is not read in this mode)
}
template <typename T>
hipError_t launch_rescale_combine(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st) {
  return rescale_stream<T, 2>(s, t, out, in, nullptr, batch, st);
}

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

// fused NTT-form rescale: workgroup = polynomial, LDS = A (the dropped row, then r) + B (d_i, then its transform)
template <typename T>
__global__ void __launch_bounds__(1024) k_rescale_ntt_fused(T *__restrict__ out, const T *__restrict__ in, const Tw<T> *__restrict__ psi,
                                                            const ModConst<T> *__restrict__ mc, const RescConst<T> *__restrict__ rc,
                                                            unsigned logn, unsigned nm, size_t batch) {
  extern __shared__ uint4 resc_lds_raw[];
  const unsigned n = 1u << logn, kept = nm - 1u;
  T *A = reinterpret_cast<T *>(resc_lds_raw), *B = A + n;
  const ModConst<T> cq = mc[kept];
  const T h = rc[0].h;
  for (size_t b = blockIdx.x; b < batch; b += gridDim.x) {
    const T *x = in + ((b * nm) << logn);
    T *o = out + ((b * kept) << logn);
    for (unsigned j = threadIdx.x; j < n; j += blockDim.x) A[j] = x[((size_t)kept << logn) + j];
    resc_inv_lds<T>(A, psi + ((size_t)kept << logn), logn, cq);
    __syncthreads();
    // from here to the end of the polynomial a thread touches A only at its own indices j
    for (unsigned j = threadIdx.x; j < n; j += blockDim.x) A[j] = csub<T>((T)(A[j] + h), cq.p);
    for (unsigned i = 0; i < kept; ++i) {
      const RescConst<T> c = rc[i];
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
        const T ri = csub<T>(A[j], c.p);
        B[j] = (T)(h >= ri ? h - ri : h + c.p - ri);
      }
      resc_fwd_lds<T>(B, psi + ((size_t)i << logn), logn, c.p, (T)(2 * c.p));
      __syncthreads();
      for (unsigned j = threadIdx.x; j < n; j += blockDim.x)
        o[((size_t)i << logn) + j] = mul_shoup<T>((T)(x[((size_t)i << logn) + j] + reduce4<T>(B[j], c.p)), c.qinv, c.qinv_sh, c.p);
      // (B[j] is rewritten next by the thread that just read it; the transform's first barrier orders the rest)
    }
    __syncthreads();
  }
}

static constexpr size_t kFusedLdsBytes = 65536;  // two rows: u64 up to 4096, u32 up to 8192, u16 up to 16384 words

template <typename T>
hipError_t launch_rescale_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st) {
  if (s.nm < 2 || !t.resc) return hipErrorInvalidValue;
  const size_t lds = 2 * s.n * sizeof(T);
  if (lds > kFusedLdsBytes || s.logn < 2) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;
  const size_t cap = (size_t)1 << 20;
  hipLaunchKernelGGL((k_rescale_ntt_fused<T>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, out, in,
                     (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, (const RescConst<T> *)t.resc, (unsigned)s.logn, (unsigned)s.nm, batch);
  return hipGetLastError();
}

#define NFLHIP_RESCALE_INSTANCES(T)                                                                                        \
  template hipError_t launch_rescale_coeff<T>(const Shape &, const DevTables &, T *, const T *, size_t, hipStream_t);      \
  template hipError_t launch_rescale_ntt_fused<T>(const Shape &, const DevTables &, T *, const T *, size_t, hipStream_t);  \
  template hipError_t launch_rescale_expand<T>(const Shape &, const DevTables &, T *, const T *, size_t, hipStream_t);     \
  template hipError_t launch_rescale_combine<T>(const Shape &, const DevTables &, T *, const T *, size_t, hipStream_t);
NFLHIP_RESCALE_INSTANCES(uint16_t)
NFLHIP_RESCALE_INSTANCES(uint32_t)
NFLHIP_RESCALE_INSTANCES(uint64_t)
#undef NFLHIP_RESCALE_INSTANCES

__global__ void k_warm_rescale() {}
hipError_t warm_rescale(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_rescale, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
