// kernels_tensor_dot.hip -- the tensor product of degree-1 ciphertexts SUMMED over terms, in NTT form (include/nflhip.h "sums of
// ciphertext products"): for every group g, row m and position i
//   D0[g] = sum_j a0(g,j) (.) b0(g,j),   D1[g] = sum_j (a0(g,j) (.) b1(g,j) + a1(g,j) (.) b0(g,j)),   D2[g] = sum_j a1(g,j) (.) b1(g,j)
// mod p_m, canonical words in and out.  Nothing here looks at the form, as kernels_dot.hip and kernels_mulrelin.hip.
//
// k_tensor_dot_ntt<T, VEC, SQUARE> -- one streaming pass.  blockIdx.y is the row m (its constants are scalar loads); a thread owns
//   16-byte groups of positions of that row (VEC = false: the word variant for pointers off 16 bytes and rows shorter than 16
//   bytes) and grid-strides over the groups * n words of the row.  The operands are those of k_dot (DotStrided, strides in words of
//   a polynomial of `rows` rows).  Per term four loads (SQUARE: b is a itself, two loads, D1 = sum 2 a0 a1); the loads of term j + 1
//   are issued before the multiplies of term j.  The three sums stay UNREDUCED in acc_t of dot_reduce.h and never touch memory.
//   The bound there is sixteen products plus a canonical carry-in: D1 takes two products per term and goes back to a canonical
//   carry-in every kTdChunk1 = 8 terms, D0 and D2 every kDotChunk = 16.  The result is the canonical residue of the exact sum, so
//   the cadence does not change the words.  (4 terms + 3) rows of traffic per output row, (2 terms + 3) for the square.
//
//   The launcher serves two callers, as launch_tensor_ntt.  The public entry: the outputs dense [groups][rows][n].  The
//   multiplication's merged plan (api.hip mulrelin_run): `pi` given -- then D0 and D1 are written as pi_m D_c with a polynomial
//   pitch of their own over orows >= rows rows, the rows past `rows` as zeros, and D2 with a third pitch.  The pitches are in words.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"  // DotRed<T>, kDotChunk
#include "dot_kernel.h"  // DotStrided, DotVec

namespace nflhip {

static constexpr unsigned kTdChunk1 = kDotChunk / 2;  // terms per reduction of D1: two products a term

template <typename T, bool VEC, bool SQUARE>
__global__ void __launch_bounds__(256) k_tensor_dot_ntt(T *out0, T *out1, T *out2, const DotStrided<T> a0, const DotStrided<T> a1,
                                                        const DotStrided<T> b0, const DotStrided<T> b1, const ModConst<T> *__restrict__ mc,
                                                        const uint64_t *__restrict__ pi, unsigned logn, unsigned rows, unsigned terms,
                                                        size_t pitch01, size_t pitch2, size_t total) {
  constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
  constexpr unsigned logv = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : 3;
  typedef DotVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  const unsigned m = blockIdx.y, lv = logn - logv;  // lv: log2 of the 16-byte groups per row
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
    const size_t g = v >> lv, pos = roff + ((v & ((((size_t)1) << lv) - 1u)) << logv);
    acc_t s0[V], s1[V], s2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s0[k] = s1[k] = s2[k] = (acc_t)0;
    Vec x0 = *reinterpret_cast<const Vec *>(a0.at(g, 0) + pos), x1 = *reinterpret_cast<const Vec *>(a1.at(g, 0) + pos);
    Vec y0 = x0, y1 = x1;
    if (!SQUARE) {
      y0 = *reinterpret_cast<const Vec *>(b0.at(g, 0) + pos);
      y1 = *reinterpret_cast<const Vec *>(b1.at(g, 0) + pos);
    }
    for (unsigned j = 0; j < terms; ++j) {
      Vec nx0 = x0, nx1 = x1, ny0 = y0, ny1 = y1;
      if (j + 1 < terms) {  // the next term's loads, in flight under this term's multiplies
        nx0 = *reinterpret_cast<const Vec *>(a0.at(g, j + 1) + pos);
        nx1 = *reinterpret_cast<const Vec *>(a1.at(g, j + 1) + pos);
        if (!SQUARE) {
          ny0 = *reinterpret_cast<const Vec *>(b0.at(g, j + 1) + pos);
          ny1 = *reinterpret_cast<const Vec *>(b1.at(g, j + 1) + pos);
        }
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const acc_t cross = (acc_t)x0.e[k] * (acc_t)(SQUARE ? x1.e[k] : y1.e[k]);
        s0[k] += (acc_t)x0.e[k] * (acc_t)(SQUARE ? x0.e[k] : y0.e[k]);
        s1[k] += SQUARE ? cross + cross : cross + (acc_t)x1.e[k] * (acc_t)y0.e[k];
        s2[k] += (acc_t)x1.e[k] * (acc_t)(SQUARE ? x1.e[k] : y1.e[k]);
      }
      if (j + 1 < terms) {  // a full chunk behind, more to come: back to a canonical carry-in
        if ((j + 1) % kTdChunk1 == 0) {
#pragma unroll
          for (int k = 0; k < V; ++k) s1[k] = (acc_t)red.reduce(s1[k]);
        }
        if ((j + 1) % kDotChunk == 0) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            s0[k] = (acc_t)red.reduce(s0[k]);
            s2[k] = (acc_t)red.reduce(s2[k]);
          }
        }
      }
      x0 = nx0, x1 = nx1;
      if (!SQUARE) y0 = ny0, y1 = ny1;
    }
    Vec d0, d1, d2;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      d0.e[k] = red.reduce(s0[k]);
      d1.e[k] = red.reduce(s1[k]);
      d2.e[k] = red.reduce(s2[k]);
      if (pi) {
        d0.e[k] = mul_shoup<T>(d0.e[k], w, wp, p);
        d1.e[k] = mul_shoup<T>(d1.e[k], w, wp, p);
      }
    }
    *reinterpret_cast<Vec *>(out0 + g * pitch01 + pos) = d0;
    *reinterpret_cast<Vec *>(out1 + g * pitch01 + pos) = d1;
    *reinterpret_cast<Vec *>(out2 + g * pitch2 + pos) = d2;
  }
}

static constexpr size_t kTensorDotWorkgroups = 4096;  // grid bound over all rows, as kernels_dot.hip

template <typename T, bool VEC>
static void tensor_dot_pick(dim3 g, hipStream_t st, bool square, T *out0, T *out1, T *out2, const DotStrided<T> &a0, const DotStrided<T> &a1,
                            const DotStrided<T> &b0, const DotStrided<T> &b1, const ModConst<T> *mc, const uint64_t *pi, unsigned logn,
                            unsigned rows, unsigned terms, size_t pitch01, size_t pitch2, size_t total) {
  const dim3 bl(256);
  if (square) hipLaunchKernelGGL((k_tensor_dot_ntt<T, VEC, true>), g, bl, 0, st, out0, out1, out2, a0, a1, a0, a1, mc, pi, logn, rows, terms, pitch01, pitch2, total);
  else hipLaunchKernelGGL((k_tensor_dot_ntt<T, VEC, false>), g, bl, 0, st, out0, out1, out2, a0, a1, b0, b1, mc, pi, logn, rows, terms, pitch01, pitch2, total);
}

template <typename T>
hipError_t launch_tensor_dot_ntt(const Shape &s, const DevTables &t, T *out0, T *out1, T *out2, const TensorDotOperand *a0, const TensorDotOperand *a1,
                                 const TensorDotOperand *b0, const TensorDotOperand *b1, size_t groups, size_t terms, size_t rows, size_t orows,
                                 size_t pitch01, size_t pitch2, const uint64_t *pi, hipStream_t st) {
  const bool square = !b0 && !b1;
  if (!out0 || !out1 || !out2 || !a0 || !a1 || !a0->ptr || !a1->ptr || (!square && (!b0 || !b1 || !b0->ptr || !b1->ptr))) return hipErrorInvalidValue;
  if (terms == 0 || terms > kDotMaxTerms) return hipErrorInvalidValue;
  if (rows == 0 || rows > s.nm || orows < rows || orows > s.nm || s.nm > 65535) return hipErrorInvalidValue;
  if (orows != rows && !pi) return hipErrorInvalidValue;  // rows of zeros belong to the scaled layout
  if (pitch01 < orows * s.n || pitch2 < rows * s.n) return hipErrorInvalidValue;
  if (groups == 0) return hipSuccess;
  constexpr size_t V = 16 / sizeof(T);
  const size_t poly = rows * s.n;  // the operands' polynomial, in words
  uintptr_t bits = (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out2;
  DotStrided<T> op[4];
  const TensorDotOperand *const src[4] = {a0, a1, square ? a0 : b0, square ? a1 : b1};
  for (int k = 0; k < 4; ++k) {
    op[k] = {(const T *)src[k]->ptr, src[k]->group_stride * poly, src[k]->term_stride * poly};
    bits |= (uintptr_t)src[k]->ptr;
  }
  const bool vec = (bits & 15u) == 0 && s.n % V == 0 && pitch01 % V == 0 && pitch2 % V == 0;
  unsigned logv = 0;
  if (vec) while (((size_t)1 << logv) < V) ++logv;
  const size_t total = (groups * s.n) >> logv;  // 16-byte groups (words) of one row over the groups
  size_t blocks = (total + 255) / 256, cap = kTensorDotWorkgroups / orows ? kTensorDotWorkgroups / orows : 1;
  if (blocks > cap) blocks = cap;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const dim3 g((unsigned)blocks, (unsigned)orows);
  if (vec) tensor_dot_pick<T, true>(g, st, square, out0, out1, out2, op[0], op[1], op[2], op[3], mc, pi, (unsigned)s.logn, (unsigned)rows, (unsigned)terms, pitch01, pitch2, total);
  else tensor_dot_pick<T, false>(g, st, square, out0, out1, out2, op[0], op[1], op[2], op[3], mc, pi, (unsigned)s.logn, (unsigned)rows, (unsigned)terms, pitch01, pitch2, total);
  return hipGetLastError();
}

#define NFLHIP_TENSOR_DOT_INSTANCES(T)                                                                                                          \
  template hipError_t launch_tensor_dot_ntt<T>(const Shape &, const DevTables &, T *, T *, T *, const TensorDotOperand *, const TensorDotOperand *, \
                                               const TensorDotOperand *, const TensorDotOperand *, size_t, size_t, size_t, size_t, size_t, size_t, \
                                               const uint64_t *, hipStream_t);
NFLHIP_TENSOR_DOT_INSTANCES(uint16_t)
NFLHIP_TENSOR_DOT_INSTANCES(uint32_t)
NFLHIP_TENSOR_DOT_INSTANCES(uint64_t)
#undef NFLHIP_TENSOR_DOT_INSTANCES

__global__ void k_warm_tensor_dot() {}
hipError_t warm_tensor_dot(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_tensor_dot, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
