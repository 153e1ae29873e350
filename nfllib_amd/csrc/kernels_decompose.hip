// kernels_decompose.hip -- gadget decomposition: the base-2^w digits of every row of a coefficient-form polynomial, and the
// companion scaling by the gadget's powers (include/nflhip.h "gadget decomposition").
//
// Context with nm moduli of `bits` = W - 2 bits (2^(bits-1) < p < 2^bits), digit width 1 <= w <= bits - 1, B = 2^w,
// l = ceil(bits / w) digits per word, terms = nm l.  Term j = m l + t is digit t of row m.  For the canonical word x of row m:
//   unsigned   d_t = (x >> w t) & (B - 1)                                                         in [0, B)
//   signed     c = x if x <= (p_m - 1) / 2 else x - p_m (the centred representative), r_0 = c,
//              d_t = ((r_t + B/2) mod B) - B/2 in [-B/2, B/2),  r_(t+1) = (r_t - d_t) / B  for t < l - 1,   d_(l-1) = r_(l-1).
// Either way sum_t d_t B^t = x (unsigned) or c (signed), which is x mod p_m.
//
// No carry chain: r_(t+1) = floor((r_t + B/2) / B), and nested floors collapse (floor((floor(a / B) + k) / B) =
// floor((a + k B) / B^2)), so
//   r_t = floor((c + H_t) / B^t),   H_t = (B/2) (1 + B + ... + B^(t-1)) < B^t,   H_(t+1) = H_t B + B/2,
// an add and an arithmetic shift from the centred word; every digit is formed on its own (DecDigit::digit), the compact kernel's
// thread forms only its term's.  w t <= bits - 1 for every t < l, so |c| + H_t < 2^(bits-1) + 2^(bits-1) fits the signed word.
//
// The top digit: |d_(l-1)| <= B/2.  |r_0| <= (p - 1) / 2 <= 2^(bits-1) - 1 and |r_(t+1)| <= |r_t| / B + 1/2, hence
//   |r_t| <= (2^(bits-1) - 1) / B^t + (1/2) (1 + 1/B + ...) < 2^(bits-1-wt) + 1      (the geometric sum is at most B / (2 (B - 1)) <= 1);
// at t = l - 1, w l >= bits gives bits - 1 - w (l - 1) <= w - 1, and an integer strictly below 2^(w-1) + 1 is at most B/2.
// So a signed digit lies in [-B/2, B/2] and, as w <= bits - 1, |d| <= 2^(bits-2) < p for every modulus: the word of a negative
// digit is p_m' + d; the compact formats hold it for w <= 7 / 15 / 31 (B/2 <= 64 / 16384 / 2^30; an unsigned digit <= 2^w - 1).
//
// gadget_mul: out[b][j = (m, t)][m'][i] = in[b][m][i] 2^(w t) mod p_m for m' = m, 0 elsewhere.  2^(w t) <= 2^(bits-1) < p_m is its
// own canonical residue, so the factor is a shift and the product the exact Barrett multiplication of modarith.h.
//
// Kernels:
//   k_decompose_stream   words out [batch][terms][nm][n]: blockIdx.y = the input row m (its constants are scalar loads); a thread owns
//                        one 16-byte group of positions of that row, reads it once, and for t = 0 .. l - 1 forms digit t in
//                        registers and stores it to the nm rows of term (m, t): l nm 16-byte stores per 16-byte load.  MODE 2 is
//                        gadget_mul with the same ownership (zeros for m' != m).  V = 1: the word path for misaligned pointers
//                        and rows shorter than 16 bytes.
//   k_decompose_compact  compact out [batch][terms][n], one signed integer per coefficient: blockIdx.y = the term; a thread owns E
//                        consecutive positions -- 16 output bytes, or 16 input bytes where that is more -- so several 16-byte loads
//                        feed one 16-byte store.  E = 1: the word path.
//   k_decompose_ntt_fused  NTT-form words in ONE launch: a workgroup owns one output polynomial (b, j); every thread forms its share
//                        of digit t of row m once and keeps it in registers; per output row m' the workgroup spreads the digit into
//                        ONE LDS row, forward-transforms it with the radix-4 lazy transform of ntt_lds.h and stores canonical words.
//                        1x the output of traffic against 3x for the composed plan (stream, then the forward launcher in place:
//                        api.hip).  Rows up to 32 KiB; api.hip runs it by default for rows of up to 2048 words (profiles/r11_decompose.txt).
#include "kernels.h"
#include "modarith.h"
#include "ntt_lds.h"

namespace nflhip {

static constexpr size_t kDecompWorkgroups = 4096;    // grid bound over all rows / terms, as kernels_dot.hip
static constexpr size_t kDecompFusedLds = 32768;     // one row: u64 up to 4096, u32 up to 8192, u16 up to 16384 words

template <typename T, int V> struct alignas(V * sizeof(T)) DecVec { T e[V]; };

template <typename T> struct DecSigned { typedef int32_t type; };  // a signed word that holds |c| + H_t < 2^bits
template <> struct DecSigned<uint64_t> { typedef int64_t type; };

// the constants of one digit position t
template <typename T> struct DecDigit {
  typedef typename DecSigned<T>::type S;
  S H, half, mask;    // H_t (0: unsigned), B/2 (0: unsigned), B - 1
  unsigned sh;        // w t
  bool raw;           // signed and t == l - 1: the top digit is r_t itself
  __device__ __forceinline__ DecDigit(unsigned w, unsigned t, unsigned l, bool sgn) {
    mask = (S)(((S)1 << w) - 1);
    half = sgn ? (S)((S)1 << (w - 1u)) : (S)0;
    H = 0;
    for (unsigned k = 0; k < t; ++k) H = step(H, w);
    sh = w * t;
    raw = sgn && t + 1u == l;
  }
  // H_(t+1) = H_t B + B/2, in the unsigned word: the step past the last digit (never used) may wrap
  __device__ __forceinline__ S step(S h, unsigned w) const { return (S)(T)((T)((T)h << w) + (T)half); }
  __device__ __forceinline__ void next(unsigned w, unsigned l) {  // t -> t + 1
    H = step(H, w);
    sh += w;
    raw = half != 0 && sh + w == w * l;
  }
  __device__ __forceinline__ S digit(S c) const {
    const S r = (S)((S)(c + H) >> sh);  // arithmetic shift: the floor
    return raw ? r : (S)((S)((S)(r + half) & mask) - half);
  }
};
// the word whose digits are taken: the centred representative (signed) or x itself
template <typename T> __device__ __forceinline__ typename DecSigned<T>::type dec_centre(T x, T p, bool sgn) {
  typedef typename DecSigned<T>::type S;
  return sgn && x > (T)((p - 1u) >> 1) ? (S)((S)x - (S)p) : (S)x;
}
template <typename T> __device__ __forceinline__ T dec_word(typename DecSigned<T>::type d, T p) {  // d < 0 stands for p + d
  typedef typename DecSigned<T>::type S;
  return (T)(d < 0 ? (S)((S)p + d) : d);
}

// MODE 0 / 1: unsigned / signed digits.  MODE 2: gadget_mul.
template <typename T, int V, int MODE>
__global__ void __launch_bounds__(256) k_decompose_stream(T *__restrict__ out, const T *__restrict__ in, const ModConst<T> *__restrict__ mc,
                                                          unsigned logn, unsigned nm, unsigned logv, unsigned w, unsigned l, size_t total) {
  typedef DecVec<T, V> Vec;
  typedef typename DecSigned<T>::type S;
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the groups per row
  const ModConst<T> cm = mc[m];
  const size_t terms = (size_t)nm * l;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t b = v >> lv, j = (v & ((((size_t)1) << lv) - 1u)) << logv;
    const Vec x = *reinterpret_cast<const Vec *>(in + ((b * nm + m) << logn) + j);
    T *o = out + (((b * terms + (size_t)m * l) * nm) << logn) + j;  // row 0 of term (m, 0); a term is nm rows
    if (MODE == 2) {
      for (unsigned t = 0; t < l; ++t, o += (size_t)nm << logn) {
        Vec y;
#pragma unroll
        for (int k = 0; k < V; ++k) y.e[k] = barrett<T>::mul(x.e[k], (T)((T)1 << (w * t)), cm.p, cm.mu);
        for (unsigned r = 0; r < nm; ++r) {
          Vec q;
#pragma unroll
          for (int k = 0; k < V; ++k) q.e[k] = r == m ? y.e[k] : (T)0;
          *reinterpret_cast<Vec *>(o + ((size_t)r << logn)) = q;
        }
      }
    } else {
      S c[V];
#pragma unroll
      for (int k = 0; k < V; ++k) c[k] = dec_centre<T>(x.e[k], cm.p, MODE == 1);
      DecDigit<T> dg(w, 0, l, MODE == 1);
      for (unsigned t = 0; t < l; ++t, o += (size_t)nm << logn, dg.next(w, l)) {
        S d[V];
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = dg.digit(c[k]);
        if (MODE == 0) {  // a digit in [0, B) is the same word in every row
          Vec y;
#pragma unroll
          for (int k = 0; k < V; ++k) y.e[k] = (T)d[k];
          for (unsigned r = 0; r < nm; ++r) *reinterpret_cast<Vec *>(o + ((size_t)r << logn)) = y;
        } else {
          for (unsigned r = 0; r < nm; ++r) {
            const T p = mc[r].p;
            Vec y;
#pragma unroll
            for (int k = 0; k < V; ++k) y.e[k] = dec_word<T>(d[k], p);
            *reinterpret_cast<Vec *>(o + ((size_t)r << logn)) = y;
          }
        }
      }
    }
  }
}

template <typename T, typename O, int E>
__global__ void __launch_bounds__(256) k_decompose_compact(O *__restrict__ out, const T *__restrict__ in, const ModConst<T> *__restrict__ mc,
                                                           unsigned logn, unsigned nm, unsigned loge, unsigned w, unsigned l, int sgn,
                                                           size_t total) {
  constexpr int NI = E * sizeof(T) >= 16 ? (int)(E * sizeof(T) / 16) : 1;  // 16-byte loads per thread
  constexpr int VI = E / NI;
  constexpr int NO = E * sizeof(O) >= 16 ? (int)(E * sizeof(O) / 16) : 1;  // 16-byte stores per thread
  constexpr int VO = E / NO;
  typedef DecVec<T, VI> VecI;
  typedef DecVec<O, VO> VecO;
  const unsigned jt = blockIdx.y, m = jt / l, t = jt - m * l, le = logn - loge;
  const T p = mc[m].p;
  const DecDigit<T> dg(w, t, l, sgn != 0);
  const size_t terms = (size_t)nm * l;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t b = v >> le, i = (v & ((((size_t)1) << le) - 1u)) << loge;
    const T *x = in + ((b * nm + m) << logn) + i;
    O *o = out + ((b * terms + jt) << logn) + i;
    VecI xv[NI];
#pragma unroll
    for (int q = 0; q < NI; ++q) xv[q] = *reinterpret_cast<const VecI *>(x + q * VI);
    O d[E];
#pragma unroll
    for (int k = 0; k < E; ++k) d[k] = (O)dg.digit(dec_centre<T>(xv[k / VI].e[k % VI], p, sgn != 0));
#pragma unroll
    for (int q = 0; q < NO; ++q) {
      VecO y;
#pragma unroll
      for (int k = 0; k < VO; ++k) y.e[k] = d[q * VO + k];
      *reinterpret_cast<VecO *>(o + q * VO) = y;
    }
  }
}

// grid over x for `total` threads' worth of work, `rows` of them over y
static inline dim3 dec_grid(size_t total, size_t rows) {
  // grid-stride over a bounded grid: kDecompWorkgroups over all rows, 16 per CU (the rule of kernels_dot.hip dot_launch)
  size_t blocks = (total + 255) / 256, cap = kDecompWorkgroups / rows ? kDecompWorkgroups / rows : 1;
  if (blocks > cap) blocks = cap;
  return dim3((unsigned)blocks, (unsigned)rows);
}
static inline unsigned dec_digits(const Shape &s, unsigned w) { return ((unsigned)s.limb_bits - 2u + w - 1u) / w; }
static inline bool dec_width_ok(const Shape &s, int w) { return w >= 1 && w <= s.limb_bits - 3; }

template <typename T, int MODE>
static hipError_t decompose_stream(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, hipStream_t st) {
  if (!dec_width_ok(s, w) || s.nm > 65535) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  const unsigned l = dec_digits(s, (unsigned)w);
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g = dec_grid(total, s.nm), bl(256);
  if (vec) hipLaunchKernelGGL((k_decompose_stream<T, V, MODE>), g, bl, 0, st, out, in, mc, (unsigned)s.logn, (unsigned)s.nm, logv, (unsigned)w, l, total);
  else hipLaunchKernelGGL((k_decompose_stream<T, 1, MODE>), g, bl, 0, st, out, in, mc, (unsigned)s.logn, (unsigned)s.nm, logv, (unsigned)w, l, total);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_decompose_words(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, int sgn, hipStream_t st) {
  return sgn ? decompose_stream<T, 1>(s, t, out, in, batch, w, st) : decompose_stream<T, 0>(s, t, out, in, batch, w, st);
}
template <typename T>
hipError_t launch_gadget_mul(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, hipStream_t st) {
  return decompose_stream<T, 2>(s, t, out, in, batch, w, st);
}

template <typename T, typename O>
static hipError_t decompose_compact(const Shape &s, const DevTables &t, O *out, const T *in, size_t batch, int w, int sgn, hipStream_t st) {
  if (!dec_width_ok(s, w) || w > (int)(8 * sizeof(O)) - 1) return hipErrorInvalidValue;
  const unsigned l = dec_digits(s, (unsigned)w);
  if (s.nm * l > 65535) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr int E = sizeof(O) <= sizeof(T) ? 16 / sizeof(O) : 16 / sizeof(T);  // 16 bytes of the narrower side
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % E == 0;
  unsigned loge = 0;
  if (vec) while ((1u << loge) < (unsigned)E) ++loge;
  const size_t total = (batch * s.n) >> loge;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g = dec_grid(total, s.nm * l), bl(256);
  if (vec) hipLaunchKernelGGL((k_decompose_compact<T, O, E>), g, bl, 0, st, out, in, mc, (unsigned)s.logn, (unsigned)s.nm, loge, (unsigned)w, l, sgn, total);
  else hipLaunchKernelGGL((k_decompose_compact<T, O, 1>), g, bl, 0, st, out, in, mc, (unsigned)s.logn, (unsigned)s.nm, loge, (unsigned)w, l, sgn, total);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_decompose_compact(const Shape &s, const DevTables &t, void *out, int format, const T *in, size_t batch, int w, int sgn,
                                    hipStream_t st) {
  switch (format) {
    case 1: return decompose_compact<T, int8_t>(s, t, (int8_t *)out, in, batch, w, sgn, st);
    case 2: return decompose_compact<T, int16_t>(s, t, (int16_t *)out, in, batch, w, sgn, st);
    case 3: return decompose_compact<T, int32_t>(s, t, (int32_t *)out, in, batch, w, sgn, st);
    default: return hipErrorInvalidValue;
  }
}

// NTT-form words in one launch: workgroup = output polynomial (b, j); K positions per thread, i = threadIdx.x + k blockDim.x
template <typename T, int K>
__global__ void __launch_bounds__(1024) k_decompose_ntt_fused(T *__restrict__ out, const T *__restrict__ in, const Tw<T> *__restrict__ psi,
                                                              const ModConst<T> *__restrict__ mc, unsigned logn, unsigned nm, unsigned w,
                                                              unsigned l, int sgn, size_t polys) {
  typedef typename DecSigned<T>::type S;
  extern __shared__ uint4 dec_lds_raw[];
  T *sm = reinterpret_cast<T *>(dec_lds_raw);
  const unsigned n = 1u << logn, terms = nm * l;
  for (size_t g = blockIdx.x; g < polys; g += gridDim.x) {
    const size_t b = g / terms;
    const unsigned jt = (unsigned)(g - b * terms), m = jt / l, t = jt - m * l;
    const T pm = mc[m].p;
    const DecDigit<T> dg(w, t, l, sgn != 0);
    const T *x = in + ((b * nm + m) << logn);
    T *o = out + ((g * nm) << logn);
    S d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned i = threadIdx.x + (unsigned)k * blockDim.x;
      d[k] = i < n ? dg.digit(dec_centre<T>(x[i], pm, sgn != 0)) : (S)0;
    }
    for (unsigned r = 0; r < nm; ++r) {
      const T p = mc[r].p;
      // a thread wrote and now rewrites sm only at its own indices i; the transform's first barrier orders the rest
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const unsigned i = threadIdx.x + (unsigned)k * blockDim.x;
        if (i < n) sm[i] = dec_word<T>(d[k], p);
      }
      resc_fwd_lds<T>(sm, psi + ((size_t)r << logn), logn, p, (T)(2 * p));
      __syncthreads();
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const unsigned i = threadIdx.x + (unsigned)k * blockDim.x;
        if (i < n) o[((size_t)r << logn) + i] = reduce4<T>(sm[i], p);
      }
    }
    __syncthreads();
  }
}

template <typename T>
hipError_t launch_decompose_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, int sgn, hipStream_t st) {
  if (!dec_width_ok(s, w)) return hipErrorInvalidValue;
  const size_t lds = s.n * sizeof(T);
  if (lds > kDecompFusedLds || s.logn < 2) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;
  const unsigned l = dec_digits(s, (unsigned)w), per = (unsigned)((s.n + threads - 1) / threads);  // positions per thread: <= 4, 8 or 16
  const size_t polys = batch * s.nm * l, cap = (size_t)1 << 20;
  const dim3 g((unsigned)(polys < cap ? polys : cap)), bl(threads);
  const size_t sh = lds < 16 ? 16 : lds;
  const Tw<T> *psi = (const Tw<T> *)t.psi;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  // 32 KiB over 1024 threads: at most 32 / sizeof(T) positions per thread
  constexpr unsigned kMaxPer = 32 / sizeof(T);
  if (per > kMaxPer) return hipErrorNotSupported;
  if (per <= 4) hipLaunchKernelGGL((k_decompose_ntt_fused<T, 4>), g, bl, sh, st, out, in, psi, mc, (unsigned)s.logn, (unsigned)s.nm, (unsigned)w, l, sgn, polys);
  else if (per <= 8) hipLaunchKernelGGL((k_decompose_ntt_fused<T, (kMaxPer < 8 ? kMaxPer : 8)>), g, bl, sh, st, out, in, psi, mc, (unsigned)s.logn, (unsigned)s.nm, (unsigned)w, l, sgn, polys);
  else hipLaunchKernelGGL((k_decompose_ntt_fused<T, kMaxPer>), g, bl, sh, st, out, in, psi, mc, (unsigned)s.logn, (unsigned)s.nm, (unsigned)w, l, sgn, polys);
  return hipGetLastError();
}

#define NFLHIP_DECOMPOSE_INSTANCES(T)                                                                                                  \
  template hipError_t launch_decompose_words<T>(const Shape &, const DevTables &, T *, const T *, size_t, int, int, hipStream_t);     \
  template hipError_t launch_decompose_compact<T>(const Shape &, const DevTables &, void *, int, const T *, size_t, int, int, hipStream_t); \
  template hipError_t launch_decompose_ntt_fused<T>(const Shape &, const DevTables &, T *, const T *, size_t, int, int, hipStream_t); \
  template hipError_t launch_gadget_mul<T>(const Shape &, const DevTables &, T *, const T *, size_t, int, hipStream_t);
NFLHIP_DECOMPOSE_INSTANCES(uint16_t)
NFLHIP_DECOMPOSE_INSTANCES(uint32_t)
NFLHIP_DECOMPOSE_INSTANCES(uint64_t)
#undef NFLHIP_DECOMPOSE_INSTANCES

__global__ void k_warm_decompose() {}
hipError_t warm_decompose(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_decompose, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
