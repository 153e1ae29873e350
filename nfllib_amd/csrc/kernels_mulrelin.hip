// kernels_mulrelin.hip -- the tensor product of two degree-1 ciphertexts in NTT form (include/nflhip.h "ciphertext multiplication"):
//   out0 = a0 (.) b0,   out1 = a0 (.) b1 + a1 (.) b0,   out2 = a1 (.) b1        row by row mod p_m, canonical words in and out.
// Nothing here looks at the form, as kernels_dot.hip.
//
// k_tensor_ntt<T, VEC, SQUARE> -- one streaming pass.  blockIdx.y is the row m (its constants are scalar loads); a thread owns
//   16-byte groups of positions of that row (VEC = false: the word variant for pointers off 16 bytes and rows shorter than 16
//   bytes) and grid-strides over the batch * n words of the row.  The four input groups are loaded before anything is stored, so
//   an output may be exactly an input.  out1 is accumulated UNREDUCED in acc_t of dot_reduce.h -- two products never wrap it --
//   and reduced once; out0 and out2 take the same reduction.  SQUARE: b is a itself, two reads instead of four, out1 = 2 a0 a1
//   (still below 2^(2W-3)).  4 rows read (2 squared), 3 written.
//
//   The launcher serves two callers.  The public entry: every block dense [batch][rows][n].  The multiplication's merged plan
//   (api.hip mulrelin_run): `pi` given -- a device array of nm pairs (pi_m, its Shoup companion), pi_m = P mod p_m for the kept
//   rows m < rows -- then out0 and out1 are written as pi_m d_c with a polynomial pitch of their own (the [2][batch][nm][n] layout
//   of the key-switch sums) over orows >= rows rows, the rows past `rows` as zeros, and out2 with a third pitch (L rows dense, or
//   embedded in nm rows: the mod-up's source buffer either way).  The pitches are in words.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"
#include "ntt_lds.h"
#include "keyswitch_fused.h"  // kFusedPos and the steps the one-launch kernel shares with k_modup_dot_fused

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) TnVec { T e[V]; };

template <typename T, bool VEC, bool SQUARE>
__global__ void __launch_bounds__(256) k_tensor_ntt(T *out0, T *out1, T *out2, const T *a0, const T *a1, const T *b0, const T *b1,
                                                    const ModConst<T> *__restrict__ mc, const uint64_t *__restrict__ pi, unsigned logn,
                                                    unsigned rows, size_t ipitch, size_t pitch01, size_t pitch2, size_t total) {
  constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
  constexpr unsigned logv = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : 3;
  typedef TnVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the groups per row
  const size_t roff = (size_t)m << logn;
  if (m >= rows) {  // a row past the inputs (the scaled layout only): zeros in the two sums
    Vec z;
#pragma unroll
    for (int k = 0; k < V; ++k) z.e[k] = 0;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
      const size_t o = (v >> lv) * pitch01 + roff + ((v & ((((size_t)1) << lv) - 1u)) << logv);
      *reinterpret_cast<Vec *>(out0 + o) = z;
      *reinterpret_cast<Vec *>(out1 + o) = z;
    }
    return;
  }
  const ModConst<T> cm = mc[m];
  const DotRed<T> red(cm);
  const T p = (T)cm.p, w = pi ? (T)pi[2 * m] : (T)0, wp = pi ? (T)pi[2 * m + 1] : (T)0;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (size_t)gridDim.x * blockDim.x) {
    const size_t b = v >> lv, pos = roff + ((v & ((((size_t)1) << lv) - 1u)) << logv);
    const size_t i = b * ipitch + pos;
    const Vec x0 = *reinterpret_cast<const Vec *>(a0 + i), x1 = *reinterpret_cast<const Vec *>(a1 + i);
    Vec y0 = x0, y1 = x1;
    if (!SQUARE) {
      y0 = *reinterpret_cast<const Vec *>(b0 + i);
      y1 = *reinterpret_cast<const Vec *>(b1 + i);
    }
    Vec d0, d1, d2;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const acc_t cross = (acc_t)x0.e[k] * (acc_t)y1.e[k];
      d0.e[k] = red.reduce((acc_t)x0.e[k] * (acc_t)y0.e[k]);
      d1.e[k] = red.reduce(SQUARE ? cross + cross : cross + (acc_t)x1.e[k] * (acc_t)y0.e[k]);
      d2.e[k] = red.reduce((acc_t)x1.e[k] * (acc_t)y1.e[k]);
      if (pi) {
        d0.e[k] = mul_shoup<T>(d0.e[k], w, wp, p);
        d1.e[k] = mul_shoup<T>(d1.e[k], w, wp, p);
      }
    }
    *reinterpret_cast<Vec *>(out0 + b * pitch01 + pos) = d0;
    *reinterpret_cast<Vec *>(out1 + b * pitch01 + pos) = d1;
    *reinterpret_cast<Vec *>(out2 + b * pitch2 + pos) = d2;
  }
}

static constexpr size_t kTensorWorkgroups = 4096;  // grid bound over all rows, as kernels_dot.hip

template <typename T, bool VEC>
static void tensor_pick(dim3 g, hipStream_t st, bool square, T *out0, T *out1, T *out2, const T *a0, const T *a1, const T *b0, const T *b1,
                        const ModConst<T> *mc, const uint64_t *pi, unsigned logn, unsigned rows, size_t ipitch, size_t pitch01, size_t pitch2,
                        size_t total) {
  const dim3 bl(256);
  if (square) hipLaunchKernelGGL((k_tensor_ntt<T, VEC, true>), g, bl, 0, st, out0, out1, out2, a0, a1, a0, a1, mc, pi, logn, rows, ipitch, pitch01, pitch2, total);
  else hipLaunchKernelGGL((k_tensor_ntt<T, VEC, false>), g, bl, 0, st, out0, out1, out2, a0, a1, b0, b1, mc, pi, logn, rows, ipitch, pitch01, pitch2, total);
}

template <typename T>
hipError_t launch_tensor_ntt(const Shape &s, const DevTables &t, T *out0, T *out1, T *out2, const T *a0, const T *a1, const T *b0, const T *b1,
                             size_t batch, size_t rows, size_t orows, size_t pitch01, size_t pitch2, const uint64_t *pi, hipStream_t st) {
  const bool square = !b0 && !b1;
  if (!out0 || !out1 || !out2 || !a0 || !a1 || (!square && (!b0 || !b1))) return hipErrorInvalidValue;
  if (rows == 0 || rows > s.nm || orows < rows || orows > s.nm || s.nm > 65535) return hipErrorInvalidValue;
  if (orows != rows && !pi) return hipErrorInvalidValue;  // rows of zeros belong to the scaled layout
  if (pitch01 < orows * s.n || pitch2 < rows * s.n) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  constexpr size_t V = 16 / sizeof(T);
  const uintptr_t bits = (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out2 | (uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)b0 | (uintptr_t)b1;
  const bool vec = (bits & 15u) == 0 && s.n % V == 0 && pitch01 % V == 0 && pitch2 % V == 0;
  unsigned logv = 0;
  if (vec) while (((size_t)1 << logv) < V) ++logv;
  const size_t total = (batch * s.n) >> logv;  // groups of one row over the batch
  size_t blocks = (total + 255) / 256, cap = kTensorWorkgroups / orows ? kTensorWorkgroups / orows : 1;
  if (blocks > cap) blocks = cap;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g((unsigned)blocks, (unsigned)orows);
  if (vec) tensor_pick<T, true>(g, st, square, out0, out1, out2, a0, a1, b0, b1, mc, pi, (unsigned)s.logn, (unsigned)rows, rows * s.n, pitch01, pitch2, total);
  else tensor_pick<T, false>(g, st, square, out0, out1, out2, a0, a1, b0, b1, mc, pi, (unsigned)s.logn, (unsigned)rows, rows * s.n, pitch01, pitch2, total);
  return hipGetLastError();
}

// k_tensor_modup_dot_fused<T> -- ONE launch from the four NTT-form inputs to the two sums A_c = E(pi d_c) + sum_d U_d key[d][c], U_d the
// mod-up of d2 = a1 (.) b1: k_modup_dot_fused (kernels_keyswitch.hip, which see for the LDS layout, the thread ownership and the
// barrier argument -- all unchanged) with three differences.  The source rows enter LDS as the products a1 b1, formed at the load.  A
// digit's own rows re-form that product from global memory where the key switch re-reads its input.  And on a kept row r < L the two
// accumulators of a position start from pi_r d_0 and pi_r d_1, formed from the four input words of the position and reduced to
// canonical words: the carry-in of nflhip_dot_dev's addend, so that the bound of dot_reduce.h (16 products and a canonical carry-in)
// holds as it stands and the words are those of the merged plan.  d0, d1, d2 never touch memory.  b0 == b1 == nullptr: the square.
//
// Scalar registers.  Ten pointers and seven sizes in the kernel arguments, the row's constants, a digit's record pointers and the
// loop state are more uniform values than the 100-odd scalar registers hold, and the compiler does not reload a kernel argument: it
// parks what does not fit in vector lanes.  So the arguments travel as ONE struct, the kernel's only argument, and every POINTER is
// read from the kernel-argument segment where it is used (MR_ARG: a scalar load from constant memory through a pointer the compiler
// cannot see through, so the value lives from that load to its last use nearby and not across the loops).  The seven sizes are read
// once.  No scalar register is spilled (tests/test_mulrelin_cpu.py).
template <typename T> struct MrFusedArgs {
  T *accout;
  const T *a0, *a1, *b0, *b1, *key;
  const Tw<T> *psi;
  const ModConst<T> *mc;
  const uint64_t *const *recs;
  const uint64_t *pi;
  size_t batch;
  unsigned logn, nm, L, alpha, dnum, centred;
};
template <typename T> __device__ __forceinline__ const __attribute__((address_space(4))) MrFusedArgs<T> *mr_fused_args() {
  const __attribute__((address_space(4))) MrFusedArgs<T> *p =
      (const __attribute__((address_space(4))) MrFusedArgs<T> *)__builtin_amdgcn_kernarg_segment_ptr();  // the struct is argument 0: offset 0
  asm volatile("" : "+s"(p));
  return p;
}
#define MR_ARG(field) (mr_fused_args<T>()->field)

template <typename T>
__global__ void __launch_bounds__(1024) k_tensor_modup_dot_fused(const MrFusedArgs<T> args_in_the_kernarg_segment) {
  typedef typename DotRed<T>::acc_t acc_t;
  (void)args_in_the_kernarg_segment;
  const unsigned logn = MR_ARG(logn), nm = MR_ARG(nm), L = MR_ARG(L), alpha = MR_ARG(alpha), dnum = MR_ARG(dnum), centred = MR_ARG(centred);
  const size_t batch = MR_ARG(batch);
  extern __shared__ uint4 mr_lds_raw[];
  const unsigned n = 1u << logn;
  T *Y = reinterpret_cast<T *>(mr_lds_raw), *B = Y + ((size_t)L << logn);
  uint16_t *Vr = reinterpret_cast<uint16_t *>(B + n);  // [dnum][n], centred mode only
  for (size_t b = blockIdx.x; b < batch; b += gridDim.x) {
    // the polynomial's offsets, too, are formed where they are used, from values the compiler cannot hoist
    const size_t in = (b * L) << logn;
    for (unsigned i = 0; i < L; ++i) {
      T *Yi = Y + ((size_t)i << logn);
      const ModConst<T> ci = MR_ARG(mc)[i];
      const DotRed<T> ri(ci);
      size_t at = in + ((size_t)i << logn);
      asm volatile("" : "+s"(at));
      {
        const T *a1 = MR_ARG(a1), *b1 = MR_ARG(b1);
        for (unsigned j = threadIdx.x; j < n; j += blockDim.x) Yi[j] = ri.reduce((acc_t)a1[at + j] * (acc_t)b1[at + j]);
      }
      resc_inv_lds<T>(Yi, MR_ARG(psi) + ((size_t)i << logn), logn, ci);
    }
    __syncthreads();
    for (unsigned d = 0; d < dnum; ++d) {
      const unsigned s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
      ks_fused_y_pass<T>(Y, Vr, MR_ARG(recs)[d], d, s0, ks, logn, n, centred);
    }
    for (unsigned r = 0; r < nm; ++r) {
      const ModConst<T> cr = MR_ARG(mc)[r];
      const DotRed<T> red(cr);
      const T p = (T)cr.p;
      acc_t s0a[kFusedPos], s1a[kFusedPos];
#pragma unroll
      for (int k = 0; k < kFusedPos; ++k) s0a[k] = s1a[k] = 0;
      size_t at = in + ((size_t)r << logn);  // (read on the kept rows r < L only)
      asm volatile("" : "+s"(at));
      if (r < L) {  // the addend pi_r d_c as the canonical carry-in
        const T w = (T)MR_ARG(pi)[2 * r], wp = (T)MR_ARG(pi)[2 * r + 1];
        const T *a0 = MR_ARG(a0), *a1 = MR_ARG(a1), *b0 = MR_ARG(b0), *b1 = MR_ARG(b1);
#pragma unroll
        for (int k = 0; k < kFusedPos; ++k) {
          const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
          if (j < n) {
            const T u0 = a0[at + j], u1 = a1[at + j], v0 = b0[at + j], v1 = b1[at + j];
            s0a[k] = (acc_t)mul_shoup<T>(red.reduce((acc_t)u0 * (acc_t)v0), w, wp, p);
            s1a[k] = (acc_t)mul_shoup<T>(red.reduce((acc_t)u0 * (acc_t)v1 + (acc_t)u1 * (acc_t)v0), w, wp, p);
          }
          asm volatile("" ::: "memory");  // one position at a time: four positions' loads and double-width products at once do not fit 128 registers
        }
      }
      for (unsigned d = 0; d < dnum; ++d) {
        const unsigned s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
        const T *k0 = MR_ARG(key) + (((size_t)(2 * d) * nm + r) << logn), *k1 = k0 + ((size_t)nm << logn);
        const bool own = r - s0 < ks;  // (unsigned: s0 <= r < s0 + ks) a row of the digit: the NTT-form product itself
        if (!own) {
          ks_fused_conv_row<T>(B, Y, Vr, MR_ARG(recs)[d], red, MR_ARG(psi) + ((size_t)r << logn), d, s0, ks, r, nm, logn, n, centred, p);
        }
        const T *a1 = MR_ARG(a1), *b1 = MR_ARG(b1);
#pragma unroll
        for (int k = 0; k < kFusedPos; ++k) {
          const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
          if (j < n) {
            const T u = own ? red.reduce((acc_t)a1[at + j] * (acc_t)b1[at + j]) : reduce4<T>(B[j], p);
            s0a[k] += (acc_t)u * (acc_t)k0[j];
            s1a[k] += (acc_t)u * (acc_t)k1[j];
          }
        }
        if ((d + 1) % kDotChunk == 0 && d + 1 < dnum) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
          for (int k = 0; k < kFusedPos; ++k) {
            s0a[k] = (acc_t)red.reduce(s0a[k]);
            s1a[k] = (acc_t)red.reduce(s1a[k]);
          }
        }
        // (B[j] is rewritten next by the thread that just read it; the transform's first barrier orders the rest)
      }
      size_t o = (b * nm + r) << logn, ostep = (batch * nm) << logn;
      asm volatile("" : "+s"(o), "+s"(ostep));
      T *accout = MR_ARG(accout);
#pragma unroll
      for (int k = 0; k < kFusedPos; ++k) {
        const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
        if (j < n) {
          accout[o + j] = red.reduce(s0a[k]);
          accout[o + ostep + j] = red.reduce(s1a[k]);
        }
      }
    }
    __syncthreads();  // the next polynomial's loads overwrite Y
  }
}

template <typename T>
hipError_t launch_tensor_modup_dot_fused(const Shape &s, const DevTables &t, T *acc, const T *a0, const T *a1, const T *b0, const T *b1, const T *key,
                                         const uint64_t *const *recs, const uint64_t *pi, size_t batch, size_t L, size_t alpha, int centred,
                                         hipStream_t st) {
  if (!recs || !pi || !acc || !a0 || !a1 || !key || !b0 != !b1) return hipErrorInvalidValue;
  if (L == 0 || L >= s.nm || alpha == 0 || alpha > L || s.nm > 65535) return hipErrorInvalidValue;
  const size_t dnum = (L + alpha - 1) / alpha, lds = keyswitch_fused_lds(L, dnum, s.n, sizeof(T), centred);
  if (!keyswitch_fused_fits(L, dnum, s.n, sizeof(T), centred)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  unsigned threads = (unsigned)(s.n / 4);
  threads = threads < 64u ? 64u : threads > 1024u ? 1024u : threads;  // n <= 2048: at most kFusedPos positions per thread
  const size_t cap = (size_t)1 << 20;
  const MrFusedArgs<T> args = {acc, a0, a1, b0 ? b0 : a0, b1 ? b1 : a1, key, (const Tw<T> *)t.psi, (const ModConst<T> *)t.mc, recs, pi, batch,
                               (unsigned)s.logn, (unsigned)s.nm, (unsigned)L, (unsigned)alpha, (unsigned)dnum, centred ? 1u : 0u};
  hipLaunchKernelGGL((k_tensor_modup_dot_fused<T>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, args);
  return hipGetLastError();
}

#define NFLHIP_MULRELIN_INSTANCES(T)                                                                                                      \
  template hipError_t launch_tensor_modup_dot_fused<T>(const Shape &, const DevTables &, T *, const T *, const T *, const T *, const T *, \
                                                       const T *, const uint64_t *const *, const uint64_t *, size_t, size_t, size_t, int, \
                                                       hipStream_t);                                                                       \
  template hipError_t launch_tensor_ntt<T>(const Shape &, const DevTables &, T *, T *, T *, const T *, const T *, const T *, const T *,  \
                                           size_t, size_t, size_t, size_t, size_t, const uint64_t *, hipStream_t);
NFLHIP_MULRELIN_INSTANCES(uint16_t)
NFLHIP_MULRELIN_INSTANCES(uint32_t)
NFLHIP_MULRELIN_INSTANCES(uint64_t)
#undef NFLHIP_MULRELIN_INSTANCES
#undef MR_ARG

__global__ void k_warm_mulrelin() {}
hipError_t warm_mulrelin(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_mulrelin, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
