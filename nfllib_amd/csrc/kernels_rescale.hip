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
#include "ntt_lds.h"  // resc_fwd_lds / resc_inv_lds: the whole-row transforms in LDS

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
