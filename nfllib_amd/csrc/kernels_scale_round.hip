// kernels_scale_round.hip -- RNS scale-and-round by t/Q, the one primitive of BFV multiplication the conversions lack
// (include/nflhip.h "BFV multiplication").
//
// Rows S = [0, ks), Q = prod_S p_i; rows D = [ks, nm), kd = nm - ks.  Per coefficient position, from the canonical words x_r:
//   z_r   = t x_r mod p_r                                          every row (on S folded into the conversion's constant)
//   r_j   = conv_{S -> j}(z)            the centred conversion of k_baseconv (mode bit 0) or the fast one, j in D
//   Y_j   = (z_j - r_j) Q^-1 mod p_j    j in D                      = round(t X_c / Q) mod p_j
//   out_i = conv_{D -> i}(Y)            the centred conversion again, i in S      -> dense [batch][ks][n]
//   mode bit 1 (keep): stop at Y, dense [batch][kd][n]
// Every per-position step is a function of baseconv_pos.h / dot_reduce.h, the very ones k_baseconv calls, so the words are those of
// the composition of the existing entries.
//
// Plans.  A thread owns one 16-byte group of positions of one polynomial (V words; V = 1: the word variant for misaligned pointers
// and rows shorter than 16 bytes).  <KS, KD> are the rows a thread keeps in registers:
//   <4, 5>, <8, 9>  ks <= KS and kd <= KD: all nm words of a position are read ONCE with the loads in flight together, the kd words
//                   Y_j are formed and KEPT IN REGISTERS, their own y_j and fixed-point sum on the way, and the ks output rows are
//                   written from them: nm rows read, ks written, Y never touches memory.  KD <= kDotChunk: no reduction on the way.
//   <0, 0>          any ks, kd, keep only: per row of D the sources are read again in chunks of 16 (correct, not fast); the host
//                   layer follows it with k_baseconv from the scratch it wrote.
// The constants are wave-uniform scalar loads; ks, kd, the mode and the record offsets are made values of THIS iteration as in
// k_baseconv, for the reason given there.  256 threads, grid-stride, at most 1024 workgroups.  No LDS, no scratch.
#include "kernels.h"
#include "modarith.h"
#include "dot_reduce.h"
#include "baseconv_pos.h"
#include "host_tables.h"  // scale_round_back_offset

namespace nflhip {

template <typename T, int V> struct alignas(V * sizeof(T)) SrVec { T e[V]; };
struct alignas(32) SrSrc { uint64_t w, wp, p, r; };                  // a source row's record (host_tables.h)
struct alignas(32) SrDst { uint64_t p, q, q_sh, inv, inv_sh, t, t_sh, pad; };  // a destination row's

template <typename T, int V, int KS, int KD>
__global__ void __launch_bounds__(256) k_scale_round(T *out, const T *in, const ModConst<T> *__restrict__ mc, const uint64_t *__restrict__ rec,
                                                     unsigned logn, unsigned ks_arg, unsigned kd_arg, unsigned back_arg, unsigned mode_arg,
                                                     size_t total) {
  typedef SrVec<T, V> Vec;
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr int KSR = KS > 0 ? KS : 1, KDR = KD > 0 ? KD : 1;
  constexpr unsigned logv = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : 3;
  const unsigned lv = logn - logv;  // log2 of the groups per row
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t b = g >> lv, pos = (g & ((((size_t)1) << lv) - 1u)) << logv;
    unsigned ks = ks_arg, kd = kd_arg, mode = mode_arg, lg = logn;
    asm volatile("" : "+s"(ks), "+s"(kd), "+s"(mode), "+s"(lg));
    size_t zero = 0, back = back_arg;  // (offsets, not pointers: a pointer would lose its address space and the scalar loads with it)
    asm volatile("" : "+s"(zero), "+s"(back));
    const uint64_t *__restrict__ src = rec + zero, *__restrict__ dst = src + 4 * (size_t)ks, *__restrict__ cm = dst + 8 * (size_t)kd;
    const bool centred = (mode & 1u) != 0, keep = (mode & 2u) != 0;
    const T *x = in + ((b * (ks + kd)) << lg) + pos;
    uint64_t flo[V], fhi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) flo[k] = fhi[k] = 0;
    if (KS > 0) {
      Vec xs[KSR], xd[KDR];
#pragma unroll
      for (int i = 0; i < KS; ++i)
        if ((unsigned)i < ks) xs[i] = *reinterpret_cast<const Vec *>(x + ((size_t)i << lg));
#pragma unroll
      for (int j = 0; j < KD; ++j)
        if ((unsigned)j < kd) xd[j] = *reinterpret_cast<const Vec *>(x + ((size_t)(ks + j) << lg));
      T y[KSR][V];
#pragma unroll
      for (int i = 0; i < KS; ++i)
        if ((unsigned)i < ks) {
          const SrSrc rc = reinterpret_cast<const SrSrc *>(src)[i];
#pragma unroll
          for (int k = 0; k < V; ++k) {
            y[i][k] = bc_y<T>(xs[i].e[k], (T)rc.w, (T)rc.wp, (T)rc.p);  // (t folded into w: the y of z = t x)
            if (centred) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(y[i][k], rc.r));
          }
        }
      T v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = (T)bc_fsum_round(flo[k], fhi[k]);
      // the second conversion's record, D -> S
      const uint64_t *__restrict__ src2 = src + back, *__restrict__ dst2 = src2 + 4 * (size_t)kd, *__restrict__ cm2 = dst2 + 8 * (size_t)ks;
      T y2[KDR][V];
#pragma unroll
      for (int k = 0; k < V; ++k) flo[k] = fhi[k] = 0;
#pragma unroll
      for (int j = 0; j < KD; ++j)
        if ((unsigned)j < kd) {
          const DotRed<T> red(mc[ks + j]);
          const SrDst d = reinterpret_cast<const SrDst *>(dst)[j];
          const uint64_t *__restrict__ c = cm + (size_t)j * ks;
          acc_t acc[V];
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = 0;
#pragma unroll
          for (int i = 0; i < KS; ++i)  // KS <= kDotChunk terms: no reduction on the way
            if ((unsigned)i < ks) {
              const T cij = (T)c[i];
#pragma unroll
              for (int k = 0; k < V; ++k) acc[k] += (acc_t)y[i][k] * (acc_t)cij;
            }
          Vec w;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const T z = mul_shoup<T>(xd[j].e[k], (T)d.t, (T)d.t_sh, (T)d.p);
            w.e[k] = bc_finish<T>(red.reduce(acc[k]), centred, v[k], (T)d.q, (T)d.q_sh, true, z, (T)d.inv, (T)d.inv_sh, (T)d.p);
          }
          if (keep) {
            *reinterpret_cast<Vec *>(out + ((b * kd + j) << lg) + pos) = w;
          } else {
            const SrSrc rc = reinterpret_cast<const SrSrc *>(src2)[j];
#pragma unroll
            for (int k = 0; k < V; ++k) {
              y2[j][k] = bc_y<T>(w.e[k], (T)rc.w, (T)rc.wp, (T)rc.p);
              bc_fsum_add(flo[k], fhi[k], bc_frac<T>(y2[j][k], rc.r));
            }
          }
        }
      if (!keep) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (T)bc_fsum_round(flo[k], fhi[k]);
#pragma unroll
        for (int i = 0; i < KS; ++i)
          if ((unsigned)i < ks) {
            const DotRed<T> red(mc[i]);
            const T p = (T)dst2[8 * i], q = (T)dst2[8 * i + 1], q_sh = (T)dst2[8 * i + 2];
            const uint64_t *__restrict__ c = cm2 + (size_t)i * kd;
            acc_t acc[V];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0;
#pragma unroll
            for (int j = 0; j < KD; ++j)  // KD <= kDotChunk terms
              if ((unsigned)j < kd) {
                const T cji = (T)c[j];
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += (acc_t)y2[j][k] * (acc_t)cji;
              }
            Vec w;
#pragma unroll
            for (int k = 0; k < V; ++k) w.e[k] = bc_finish<T>(red.reduce(acc[k]), true, v[k], q, q_sh, false, (T)0, (T)0, (T)0, p);
            *reinterpret_cast<Vec *>(out + ((b * ks + i) << lg) + pos) = w;
          }
      }
    } else {  // keep only, any ks and kd
      if (centred) {
        for (unsigned i = 0; i < ks; ++i) {
          const Vec xv = *reinterpret_cast<const Vec *>(x + ((size_t)i << lg));
          const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], p = (T)src[4 * i + 2];
          const uint64_t r = src[4 * i + 3];
#pragma unroll
          for (int k = 0; k < V; ++k) bc_fsum_add(flo[k], fhi[k], bc_frac<T>(bc_y<T>(xv.e[k], w, wp, p), r));
        }
      }
      T v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = (T)bc_fsum_round(flo[k], fhi[k]);
      for (unsigned j = 0; j < kd; ++j) {
        const DotRed<T> red(mc[ks + j]);
        const uint64_t *__restrict__ d = dst + 8 * (size_t)j, *__restrict__ c = cm + (size_t)j * ks;
        const T p = (T)d[0];
        const Vec xj = *reinterpret_cast<const Vec *>(x + ((size_t)(ks + j) << lg));
        acc_t acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0;
        for (unsigned i = 0; i < ks; ++i) {
          const Vec xv = *reinterpret_cast<const Vec *>(x + ((size_t)i << lg));
          const T w = (T)src[4 * i], wp = (T)src[4 * i + 1], pi = (T)src[4 * i + 2], cij = (T)c[i];
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += (acc_t)bc_y<T>(xv.e[k], w, wp, pi) * (acc_t)cij;
          if ((i + 1) % kDotChunk == 0 && i + 1 < ks) {  // a full chunk behind, more to come: back to a canonical carry-in
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = (acc_t)red.reduce(acc[k]);
          }
        }
        Vec w;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const T z = mul_shoup<T>(xj.e[k], (T)d[5], (T)d[6], p);
          w.e[k] = bc_finish<T>(red.reduce(acc[k]), centred, v[k], (T)d[1], (T)d[2], true, z, (T)d[3], (T)d[4], p);
        }
        *reinterpret_cast<Vec *>(out + ((b * kd + j) << lg) + pos) = w;
      }
    }
  }
}

template <typename T, int V>
static hipError_t scale_round_pick(dim3 g, hipStream_t st, T *out, const T *in, const ModConst<T> *mc, const uint64_t *rec, unsigned logn, unsigned ks,
                                   unsigned kd, unsigned mode, int chunked, size_t total) {
  const dim3 bl(256);
  const unsigned back = (unsigned)scale_round_back_offset(ks, kd);
  if (chunked) hipLaunchKernelGGL((k_scale_round<T, V, 0, 0>), g, bl, 0, st, out, in, mc, rec, logn, ks, kd, back, mode, total);
  else if (ks <= 4 && kd <= 5) hipLaunchKernelGGL((k_scale_round<T, V, 4, 5>), g, bl, 0, st, out, in, mc, rec, logn, ks, kd, back, mode, total);
  else hipLaunchKernelGGL((k_scale_round<T, V, 8, 9>), g, bl, 0, st, out, in, mc, rec, logn, ks, kd, back, mode, total);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_scale_round(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t ks, int centred,
                              int keep, int chunked, hipStream_t st) {
  if (!rec || ks == 0 || ks >= s.nm || s.nm > 65535 || (const T *)out == in) return hipErrorInvalidValue;
  const size_t kd = s.nm - ks;
  if (chunked ? !keep : !scale_round_in_registers(ks, kd)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  constexpr int V = 16 / sizeof(T);
  const bool vec = (((uintptr_t)out | (uintptr_t)in) & 15u) == 0 && s.n % V == 0;
  unsigned logv = 0;
  if (vec) while ((1u << logv) < (unsigned)V) ++logv;
  const size_t total = (batch * s.n) >> logv;
  size_t blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const unsigned mode = (centred ? 1u : 0u) | (keep ? 2u : 0u);
  const dim3 g((unsigned)blocks);
  if (vec) return scale_round_pick<T, V>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)ks, (unsigned)kd, mode, chunked, total);
  return scale_round_pick<T, 1>(g, st, out, in, mc, rec, (unsigned)s.logn, (unsigned)ks, (unsigned)kd, mode, chunked, total);
}

template hipError_t launch_scale_round<uint16_t>(const Shape &, const DevTables &, uint16_t *, const uint16_t *, const uint64_t *, size_t, size_t, int, int, int, hipStream_t);
template hipError_t launch_scale_round<uint32_t>(const Shape &, const DevTables &, uint32_t *, const uint32_t *, const uint64_t *, size_t, size_t, int, int, int, hipStream_t);
template hipError_t launch_scale_round<uint64_t>(const Shape &, const DevTables &, uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t, int, int, int, hipStream_t);

__global__ void k_warm_scale_round() {}
hipError_t warm_scale_round(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_scale_round, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
