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
#include "mulrelin_fused.h"  // MrFusedArgs and k_tensor_modup_dot_fused<T, Args>

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

// k_tensor_modup_dot_fused<T, Args>, its arguments and the account of its scalar registers are in mulrelin_fused.h; here its instances
// on the context's own key layout (Args = MrFusedArgs<T>)
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
  hipLaunchKernelGGL((k_tensor_modup_dot_fused<T, MrFusedArgs<T>>), dim3((unsigned)(batch < cap ? batch : cap)), dim3(threads), lds < 16 ? 16 : lds, st, args);
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

__global__ void k_warm_mulrelin() {}
hipError_t warm_mulrelin(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_mulrelin, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
