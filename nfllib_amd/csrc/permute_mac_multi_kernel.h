// permute_mac_multi_kernel.h -- k_permute_mac_multi_ntt, the several-output form of k_permute_mac_ntt (permute_mac_kernel.h), its
// weightless sibling k_permute_sum_ntt and their launchers, apart from their instances (kernels_bsgs.hip, which see for what they
// serve).  The tile plan, the staging and the accumulators are those of k_permute_mac_ntt: what is new is that the ONE staged source
// chunk of a term, read permuted ONCE per word, is multiplied by the weights of JB outputs into JB sets of unreduced accumulators.
// Device code; include after kernels.h.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "permute_mac_kernel.h"  // mac_u32x4, mac_tile_bytes, mac_add; automorph_index.h, dot_reduce.h

#ifndef NFLHIP_MAC_MULTI_JB
#define NFLHIP_MAC_MULTI_JB 2  // the outputs one launch serves: see kernels_bsgs.hip for the choice
#endif

namespace nflhip {

constexpr int kMacMultiJB = NFLHIP_MAC_MULTI_JB;

// in, k: shared by the outputs.  w[o * kMacMaxTerms + t]: NULL = the zero weight, skipped by a scalar branch.  out[o] for o < the
// launch's `nout`; addend[o] NULL or out[o].  wrow as MacTerms / MacTermsLevel.
template <typename T, int JB> struct MacMultiTerms {
  static constexpr bool kLevel = false;
  const T *in[kMacMaxTerms];
  unsigned k[kMacMaxTerms];
  const T *w[JB * kMacMaxTerms];
  T *out[JB];
  const T *addend[JB];
  __device__ __forceinline__ unsigned wrow(unsigned r) const { return r; }
};
template <typename T, int JB> struct MacMultiTermsLevel {
  static constexpr bool kLevel = true;
  const T *in[kMacMaxTerms];
  unsigned k[kMacMaxTerms];
  const T *w[JB * kMacMaxTerms];
  T *out[JB];
  const T *addend[JB];
  unsigned split, hole;
  __device__ __forceinline__ unsigned wrow(unsigned r) const { return r + (r >= split ? hole : 0u); }
};
// the weightless form: out = addend + sum_t sigma_{k_t}(in_t)
template <typename T> struct PermuteSumTerms {
  const T *in[kMacMaxTerms];
  unsigned k[kMacMaxTerms];
};

// the tile of k_permute_mac_ntt: a chunk of one row, or several whole rows.  A SECOND COPY of the decomposition written out in
// k_permute_mac_ntt, as mac_plan below is of the one in permute_mac_launch: the one-output kernel and its launcher are left word for
// word as they are so that its 12 + 6 instances keep their register counts (tests/test_level_rotate_cpu.py).  A change to the tile
// plan is made in both files; tests/test_gpu_automorphism_mac_multi.py holds the two to the same words on every tile shape.
struct MacTile {
  size_t row0, base;
  unsigned words, dst_chunk, cm0, jbase;
};
__device__ __forceinline__ MacTile mac_tile(size_t tile, unsigned logn, unsigned chunk_log, unsigned rows_per_tile, size_t rows, unsigned R) {
  MacTile m;
  const unsigned chunks_log = logn - chunk_log;
  m.dst_chunk = 0;
  if (chunks_log) {
    m.row0 = tile >> chunks_log;
    m.dst_chunk = (unsigned)(tile & ((1u << chunks_log) - 1u));
    m.base = (m.row0 << logn) + ((size_t)m.dst_chunk << chunk_log);
    m.words = 1u << chunk_log;
  } else {
    m.row0 = tile * rows_per_tile;
    const size_t nr = rows - m.row0 < rows_per_tile ? rows - m.row0 : rows_per_tile;
    m.base = m.row0 << logn;
    m.words = (unsigned)nr << logn;
  }
  m.cm0 = (unsigned)(m.row0 % R);
  m.jbase = m.dst_chunk << chunk_log;
  return m;
}

template <typename T, bool VEC, int JB, class Terms>
__global__ void __launch_bounds__(256) k_permute_mac_multi_ntt(const Terms terms_, const ModConst<T> *__restrict__ mc, unsigned nterms, unsigned nout,
                                                               unsigned logn, unsigned R, unsigned chunk_log, unsigned rows_per_tile, size_t rows,
                                                               size_t ntiles, size_t in_cs, size_t out_cs) {
  extern __shared__ uint4 mac_multi_lds_raw[];
  typedef typename std::conditional<VEC, mac_u32x4, T>::type item_t;
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr unsigned V = sizeof(item_t) / sizeof(T);
  constexpr unsigned I = (unsigned)(mac_tile_bytes<T>(VEC) / sizeof(item_t)) / 256u;
  union Item { item_t u; T w[V]; };
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;
  const size_t in_off = blockIdx.y * in_cs, out_off = blockIdx.y * out_cs;
  item_t *buf = reinterpret_cast<item_t *>(mac_multi_lds_raw);
  const T *lds = reinterpret_cast<const T *>(buf);
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const MacTile m = mac_tile(tile, logn, chunk_log, rows_per_tile, rows, R);
    const unsigned items = m.words / V;
    acc_t acc[JB][I][V];
#pragma unroll
    for (int o = 0; o < JB; ++o)
#pragma unroll
      for (unsigned i = 0; i < I; ++i)
#pragma unroll
        for (unsigned e = 0; e < V; ++e) acc[o][i][e] = 0;
    for (unsigned t = 0; t < nterms; ++t) {
      const unsigned k = terms_.k[t];
      const unsigned sbase = chunks_log ? (aut_ntt_src(m.jbase, k, logn, mask2n) >> chunk_log) << chunk_log : 0u;
      const item_t *src = reinterpret_cast<const item_t *>(terms_.in[t] + in_off + (chunks_log ? (m.row0 << logn) + sbase : m.base));
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) buf[it] = src[it];
      }
      __syncthreads();
      // the permuted words, once for every output
      Item x[I];
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) {
#pragma unroll
          for (unsigned e = 0; e < V; ++e) {
            const unsigned local = it * V + e;
            x[i].w[e] = chunks_log ? lds[aut_ntt_src(m.jbase + local, k, logn, mask2n) - sbase]
                                   : lds[(local & ~(n - 1u)) + aut_ntt_src(local & (n - 1u), k, logn, mask2n)];
          }
        }
      }
#pragma unroll
      for (int o = 0; o < JB; ++o) {
        const T *__restrict__ w = terms_.w[o * kMacMaxTerms + t];
        if (!w) continue;  // (uniform: a kernel argument)
#pragma unroll
        for (unsigned i = 0; i < I; ++i) {
          const unsigned it = threadIdx.x + i * 256u;
          if (it < items) {
            const unsigned local = it * V;
            const size_t woff = chunks_log ? ((size_t)terms_.wrow(m.cm0) << logn) + m.jbase + local
                                           : ((size_t)terms_.wrow((m.cm0 + (local >> logn)) % R) << logn) + (local & (n - 1u));
            Item wv;
            wv.u = *reinterpret_cast<const item_t *>(w + woff);
#pragma unroll
            for (unsigned e = 0; e < V; ++e) acc[o][i][e] += (acc_t)x[i].w[e] * wv.w[e];
          }
        }
      }
      __syncthreads();  // (the next term overwrites the staging area)
    }
    // per output: one reduction, the addend, the store
#pragma unroll
    for (int o = 0; o < JB; ++o) {
      if ((unsigned)o >= nout) break;
      T *out = terms_.out[o] + out_off;
      const T *addend = terms_.addend[o] ? terms_.addend[o] + out_off : nullptr;  // (out itself: a thread reads the words it writes)
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) {
          const unsigned local = it * V;
          const ModConst<T> &mm = mc[chunks_log ? m.cm0 : (m.cm0 + (local >> logn)) % R];
          const DotRed<T> red(mm);
          const T p = mm.p;
          Item r, a;
          if (addend) a.u = *reinterpret_cast<const item_t *>(addend + m.base + local);
#pragma unroll
          for (unsigned e = 0; e < V; ++e) {
            r.w[e] = red.reduce(acc[o][i][e]);
            if (addend) r.w[e] = mac_add<T>(r.w[e], a.w[e], p);
          }
          *reinterpret_cast<item_t *>(out + m.base + local) = r.u;
        }
      }
    }
  }
}

// out = addend + sum_t sigma_{k_t}(in_t) mod p_j: canonical words in, a modular addition per term, no weight and no wide accumulator
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_permute_sum_ntt(const PermuteSumTerms<T> terms_, T *out_, const T *addend_, const ModConst<T> *__restrict__ mc,
                                                         unsigned nterms, unsigned logn, unsigned R, unsigned chunk_log, unsigned rows_per_tile,
                                                         size_t rows, size_t ntiles, size_t in_cs, size_t out_cs) {
  extern __shared__ uint4 mac_sum_lds_raw[];
  typedef typename std::conditional<VEC, mac_u32x4, T>::type item_t;
  constexpr unsigned V = sizeof(item_t) / sizeof(T);
  constexpr unsigned I = (unsigned)(mac_tile_bytes<T>(VEC) / sizeof(item_t)) / 256u;
  union Item { item_t u; T w[V]; };
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;
  const size_t in_off = blockIdx.y * in_cs, out_off = blockIdx.y * out_cs;
  T *out = out_ + out_off;
  const T *addend = addend_ ? addend_ + out_off : nullptr;
  item_t *buf = reinterpret_cast<item_t *>(mac_sum_lds_raw);
  const T *lds = reinterpret_cast<const T *>(buf);
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const MacTile m = mac_tile(tile, logn, chunk_log, rows_per_tile, rows, R);
    const unsigned items = m.words / V;
    Item acc[I];
    T p[I];
#pragma unroll
    for (unsigned i = 0; i < I; ++i) {
      const unsigned it = threadIdx.x + i * 256u;
      p[i] = 0;
#pragma unroll
      for (unsigned e = 0; e < V; ++e) acc[i].w[e] = 0;
      if (it < items) {
        const unsigned local = it * V;
        p[i] = mc[chunks_log ? m.cm0 : (m.cm0 + (local >> logn)) % R].p;
        if (addend) acc[i].u = *reinterpret_cast<const item_t *>(addend + m.base + local);
      }
    }
    for (unsigned t = 0; t < nterms; ++t) {
      const unsigned k = terms_.k[t];
      const unsigned sbase = chunks_log ? (aut_ntt_src(m.jbase, k, logn, mask2n) >> chunk_log) << chunk_log : 0u;
      const item_t *src = reinterpret_cast<const item_t *>(terms_.in[t] + in_off + (chunks_log ? (m.row0 << logn) + sbase : m.base));
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) buf[it] = src[it];
      }
      __syncthreads();
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) {
#pragma unroll
          for (unsigned e = 0; e < V; ++e) {
            const unsigned local = it * V + e;
            const T x = chunks_log ? lds[aut_ntt_src(m.jbase + local, k, logn, mask2n) - sbase]
                                   : lds[(local & ~(n - 1u)) + aut_ntt_src(local & (n - 1u), k, logn, mask2n)];
            acc[i].w[e] = mac_add<T>(acc[i].w[e], x, p[i]);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (unsigned i = 0; i < I; ++i) {
      const unsigned it = threadIdx.x + i * 256u;
      if (it < items) *reinterpret_cast<item_t *>(out + m.base + it * V) = acc[i].u;
    }
  }
}

// the tile plan of permute_mac_launch
struct MacPlan {
  unsigned chunk_log, rows_per_tile;
  size_t ntiles, lds;
  dim3 grid;
};
template <typename T> static MacPlan mac_plan(const Shape &s, bool vec, size_t rows, size_t comps) {
  MacPlan p;
  const unsigned logn = (unsigned)s.logn;
  const size_t row_bytes = s.n * sizeof(T), tile_max = mac_tile_bytes<T>(vec);
  p.chunk_log = logn;
  p.rows_per_tile = 1;
  while (p.chunk_log > 0 && ((size_t)sizeof(T) << p.chunk_log) > tile_max) --p.chunk_log;
  if (p.chunk_log == logn && row_bytes < tile_max) p.rows_per_tile = (unsigned)(tile_max / row_bytes);
  p.lds = ((size_t)p.rows_per_tile << p.chunk_log) * sizeof(T);  // at most kNttChunkBytes
  p.ntiles = p.chunk_log < logn ? rows << (logn - p.chunk_log) : (rows + p.rows_per_tile - 1) / p.rows_per_tile;
  const size_t cap = (size_t)1 << 16;  // grid-stride beyond 65536 tiles per component
  p.grid = dim3((unsigned)(p.ntiles < cap ? p.ntiles : cap), (unsigned)comps);
  return p;
}

// a: the terms' class with its layout fields set.  weights = [outputs][terms], NULL entries skipped; addends NULL, or addends[o] NULL
// or outs[o].  One launch per JB outputs.
template <typename T, class Terms>
static hipError_t permute_mac_multi_launch(const Shape &s, const DevTables &t, Terms a, T *const *outs, const T *const *addends, const T *const *ins,
                                           const T *const *weights, const uint64_t *ks, int outputs, int terms, size_t batch, size_t R, size_t comps,
                                           size_t in_cs, size_t out_cs, hipStream_t st) {
  constexpr int JB = kMacMultiJB;
  if (terms < 1 || terms > kMacMaxTerms || outputs < 1 || R == 0 || R > s.nm || comps == 0 || comps > 65535) return hipErrorInvalidValue;
  const size_t rows = batch * R;
  if (rows == 0) return hipSuccess;
  const unsigned logn = (unsigned)s.logn, mask2n = (unsigned)(2 * s.n - 1);
  uintptr_t align_in = (in_cs * sizeof(T)) | (out_cs * sizeof(T));
  for (int m = 0; m < kMacMaxTerms; ++m) {
    const int q = m < terms ? m : 0;
    if ((ks[q] & 1) == 0) return hipErrorInvalidValue;
    a.in[m] = ins[q];
    a.k[m] = (unsigned)(ks[q] & mask2n);
    align_in |= (uintptr_t)ins[q];
  }
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  for (int o0 = 0; o0 < outputs; o0 += JB) {
    const int nout = outputs - o0 < JB ? outputs - o0 : JB;
    uintptr_t align = align_in;
    for (int o = 0; o < JB; ++o) {
      const bool live = o < nout;
      a.out[o] = live ? outs[o0 + o] : nullptr;
      a.addend[o] = live && addends ? addends[o0 + o] : nullptr;
      align |= (uintptr_t)a.out[o] | (uintptr_t)a.addend[o];
      for (int m = 0; m < kMacMaxTerms; ++m) {
        a.w[o * kMacMaxTerms + m] = live && m < terms ? weights[(size_t)(o0 + o) * terms + m] : nullptr;
        align |= (uintptr_t)a.w[o * kMacMaxTerms + m];
      }
    }
    const bool vec = align % 16 == 0 && (s.n * sizeof(T)) % 16 == 0;
    const MacPlan p = mac_plan<T>(s, vec, rows, comps);
    if (vec)
      hipLaunchKernelGGL((k_permute_mac_multi_ntt<T, true, JB, Terms>), p.grid, dim3(256), p.lds, st, a, mc, (unsigned)terms, (unsigned)nout, logn,
                         (unsigned)R, p.chunk_log, p.rows_per_tile, rows, p.ntiles, in_cs, out_cs);
    else
      hipLaunchKernelGGL((k_permute_mac_multi_ntt<T, false, JB, Terms>), p.grid, dim3(256), p.lds, st, a, mc, (unsigned)terms, (unsigned)nout, logn,
                         (unsigned)R, p.chunk_log, p.rows_per_tile, rows, p.ntiles, in_cs, out_cs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
static hipError_t permute_sum_launch(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const uint64_t *ks, int terms,
                                     size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs, hipStream_t st) {
  if (terms < 1 || terms > kMacMaxTerms || R == 0 || R > s.nm || comps == 0 || comps > 65535) return hipErrorInvalidValue;
  const size_t rows = batch * R;
  if (rows == 0) return hipSuccess;
  const unsigned logn = (unsigned)s.logn, mask2n = (unsigned)(2 * s.n - 1);
  PermuteSumTerms<T> a;
  uintptr_t align = (uintptr_t)out | (uintptr_t)addend | (in_cs * sizeof(T)) | (out_cs * sizeof(T));
  for (int m = 0; m < kMacMaxTerms; ++m) {
    const int q = m < terms ? m : 0;
    if ((ks[q] & 1) == 0) return hipErrorInvalidValue;
    a.in[m] = ins[q];
    a.k[m] = (unsigned)(ks[q] & mask2n);
    align |= (uintptr_t)ins[q];
  }
  const bool vec = align % 16 == 0 && (s.n * sizeof(T)) % 16 == 0;
  const MacPlan p = mac_plan<T>(s, vec, rows, comps);
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  if (vec)
    hipLaunchKernelGGL((k_permute_sum_ntt<T, true>), p.grid, dim3(256), p.lds, st, a, out, addend, mc, (unsigned)terms, logn, (unsigned)R, p.chunk_log,
                       p.rows_per_tile, rows, p.ntiles, in_cs, out_cs);
  else
    hipLaunchKernelGGL((k_permute_sum_ntt<T, false>), p.grid, dim3(256), p.lds, st, a, out, addend, mc, (unsigned)terms, logn, (unsigned)R, p.chunk_log,
                       p.rows_per_tile, rows, p.ntiles, in_cs, out_cs);
  return hipGetLastError();
}

}  // namespace nflhip
