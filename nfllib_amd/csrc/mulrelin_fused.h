// mulrelin_fused.h -- k_tensor_modup_dot_fused (kernels_mulrelin.hip) apart from its instances: kernels_mulrelin.hip
// instantiates it on a key in the context's own layout, kernels_level.hip on the key of the parent context read by a level context.
// Device code; include after kernels.h and keyswitch_fused.h.
#pragma once
#include "kernels.h"
#include "keyswitch_fused.h"
#include <type_traits>

namespace nflhip {

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

// the level form's arguments: the same struct FIRST, so that MR_ARG reads both, then the key's layout (MR_LV)
template <typename T> struct MrFusedArgsLevel {
  MrFusedArgs<T> base;
  unsigned knm, split, hole;
};
#define MR_LV(field) (((const __attribute__((address_space(4))) MrFusedArgsLevel<T> *)mr_fused_args<T>())->field)
// the level form of the KEY SWITCH's one-launch kernel: the same body without the three differences above -- the source rows are the
// words of a1 (the key switch's input; a0, b0, b1 and pi are unused), a digit's own rows re-read them, and the accumulators start
// from zero.  The words are those of k_modup_dot_fused; the arguments travel as above, so no scalar register is spilled here either.
template <typename T> struct KsFusedArgsLevel {
  MrFusedArgsLevel<T> lv;
};

template <typename T, class Args>  // Args: MrFusedArgs<T> (kernels_mulrelin.hip); MrFusedArgsLevel<T>, KsFusedArgsLevel<T> (kernels_level.hip)
__global__ void __launch_bounds__(1024) k_tensor_modup_dot_fused(const Args args_in_the_kernarg_segment) {
  constexpr bool LV = !std::is_same<Args, MrFusedArgs<T>>::value, TENSOR = !std::is_same<Args, KsFusedArgsLevel<T>>::value;
  (void)args_in_the_kernarg_segment;
  extern __shared__ uint4 mr_lds_raw[];
  typedef typename DotRed<T>::acc_t acc_t;
  const unsigned logn = MR_ARG(logn), nm = MR_ARG(nm), L = MR_ARG(L), alpha = MR_ARG(alpha), dnum = MR_ARG(dnum), centred = MR_ARG(centred);
  const size_t batch = MR_ARG(batch);
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
        for (unsigned j = threadIdx.x; j < n; j += blockDim.x) Yi[j] = TENSOR ? ri.reduce((acc_t)a1[at + j] * (acc_t)b1[at + j]) : a1[at + j];
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
      if (TENSOR && r < L) {  // the addend pi_r d_c as the canonical carry-in
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
        // (LV: the key in its parent context's layout -- knm rows per polynomial, the rows from `split` on `hole` rows further on)
        const size_t kpitch = LV ? (size_t)MR_LV(knm) : (size_t)nm;
        const size_t krow = (size_t)(2 * d) * kpitch + r + (LV && r >= MR_LV(split) ? MR_LV(hole) : 0u);
        const T *k0 = MR_ARG(key) + (krow << logn), *k1 = k0 + (kpitch << logn);
        const bool own = r - s0 < ks;  // (unsigned: s0 <= r < s0 + ks) a row of the digit: the NTT-form product itself
        if (!own) {
          ks_fused_conv_row<T>(B, Y, Vr, MR_ARG(recs)[d], red, MR_ARG(psi) + ((size_t)r << logn), d, s0, ks, r, nm, logn, n, centred, p);
        }
        const T *a1 = MR_ARG(a1), *b1 = MR_ARG(b1);
#pragma unroll
        for (int k = 0; k < kFusedPos; ++k) {
          const unsigned j = threadIdx.x + (unsigned)k * blockDim.x;
          if (j < n) {
            const T u = own ? (TENSOR ? red.reduce((acc_t)a1[at + j] * (acc_t)b1[at + j]) : a1[at + j]) : reduce4<T>(B[j], p);
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

#undef MR_LV
#undef MR_ARG

}  // namespace nflhip
