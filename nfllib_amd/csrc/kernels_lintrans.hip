// kernels_lintrans.hip -- the weighted sum of NTT-form automorphisms (include/nflhip.h "weighted sums of automorphisms"):
//   out[g][j][i] = addend[g][j][i] + sum_{t < terms} w_t[j][i] * in_t[g][j][src_{k_t}(i)]   mod p_j, canonical,
// on [batch][R][n] word blocks in the dense layout over the first R moduli of the context, src_k = aut_ntt_src (out[i] = in[src_k(i)]
// is what kernels_automorph.hip writes in NTT form); w_t = [>= R][n] with row stride n, shared by the batch.  The step of a slot
// linear transform that multiplies the key-switch sums by the plaintext diagonals and adds them up before the one mod-down.
//
// The tile plan of k_permute_add_ntt (kernels_rotate.hip) turned round: a workgroup owns an OUTPUT tile -- a chunk of C = n / 2^b
// slots of one row, at most kNttChunkBytes, or several whole rows when a row is shorter -- and a thread owns fixed 16-byte groups of
// it (words in the word variant) with one unreduced double-width accumulator per word (dot_reduce.h).  Per term the workgroup stages
// the ONE source chunk that fills its tile (aut_ntt_src(first slot, k_t) >> chunk_log: an odd multiplier keeps the low bits of the
// exponent, which are the high bits of the slot index, so chunks map one to one) in LDS with 16-byte loads, reads it permuted and
// multiplies by w_t's words, loaded coalesced at the output positions.  After the last term: one reduction, the addend added mod
// p_j, 16-byte stores.  Every input and weight word is read once, every output word written once.
// One staging buffer, two barriers per term, is what serves (LDS <= kNttChunkBytes).  DB: two staging buffers -- the loads of term
// t + 1 are issued into registers before term t is consumed and written to the other buffer after it, one barrier per term; it
// measured 20 - 30 % SLOWER (more registers and twice the LDS cost more than the overlap gains) and is kept behind
// NFLHIP_MAC_DOUBLE_BUFFER as the measured alternative.
// blockIdx.y is the component of a call on several (in, out, addend) sets a fixed stride apart that share ks and weights.
#include <type_traits>

#include "kernels.h"
#include "automorph_index.h"  // aut_ntt_src, kNttChunkBytes
#include "dot_reduce.h"       // DotRed, kDotChunk

namespace nflhip {

static_assert(kMacMaxTerms <= (int)kDotChunk, "one chunk of dot_reduce.h: the accumulator is reduced once, after the last term");

template <typename T> struct MacTerms {
  const T *in[kMacMaxTerms];
  const T *w[kMacMaxTerms];
  unsigned k[kMacMaxTerms];  // the multiplier, reduced mod 2n
};

typedef unsigned mac_u32x4 __attribute__((ext_vector_type(4)));  // (a native vector: arrays of it stay in registers)

// the largest tile: kNttChunkBytes of 16-byte groups; the word variant keeps 8 words per thread for every limb width
template <typename T> __host__ __device__ constexpr size_t mac_tile_bytes(bool vec) {
  return vec || 2048 * sizeof(T) > kNttChunkBytes ? kNttChunkBytes : 2048 * sizeof(T);
}

template <typename T> __device__ __forceinline__ T mac_add(T x, T y, T p) {
  const T s = (T)(x + y);  // both below p <= 2^(W-2): no wrap
  return s >= p ? (T)(s - p) : s;
}

template <typename T, bool VEC, bool DB>
__global__ void __launch_bounds__(256) k_permute_mac_ntt(const MacTerms<T> terms_, T *out_, const T *addend_,
                                                         const ModConst<T> *__restrict__ mc, unsigned nterms, unsigned logn, unsigned R,
                                                         unsigned chunk_log, unsigned rows_per_tile, size_t rows, size_t ntiles, size_t in_cs,
                                                         size_t out_cs) {
  extern __shared__ uint4 mac_lds_raw[];
  typedef typename std::conditional<VEC, mac_u32x4, T>::type item_t;   // what a thread moves at once
  typedef typename DotRed<T>::acc_t acc_t;
  constexpr unsigned V = sizeof(item_t) / sizeof(T);                   // words per item
  constexpr unsigned I = (unsigned)(mac_tile_bytes<T>(VEC) / sizeof(item_t)) / 256u;  // items per thread of a full tile
  union Item { item_t u; T w[V]; };
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;  // 0 when a tile is whole rows
  const size_t in_off = blockIdx.y * in_cs, out_off = blockIdx.y * out_cs;
  T *out = out_ + out_off;
  const T *addend = addend_ ? addend_ + out_off : nullptr;  // (may be out itself: a thread reads the words it writes)
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    size_t row0, base;
    unsigned words, dst_chunk = 0;
    if (chunks_log) {
      row0 = tile >> chunks_log;
      dst_chunk = (unsigned)(tile & ((1u << chunks_log) - 1u));
      base = (row0 << logn) + ((size_t)dst_chunk << chunk_log);
      words = 1u << chunk_log;
    } else {
      row0 = tile * rows_per_tile;
      const size_t nr = rows - row0 < rows_per_tile ? rows - row0 : rows_per_tile;
      base = row0 << logn;
      words = (unsigned)nr << logn;
    }
    const unsigned cm0 = (unsigned)(row0 % R), jbase = dst_chunk << chunk_log, items = words / V;
    // where term t's source tile starts, in words from in_t: the tile itself when it is whole rows
    auto src_base = [&](unsigned t, unsigned &sbase) {
      sbase = chunks_log ? (aut_ntt_src(jbase, terms_.k[t], logn, mask2n) >> chunk_log) << chunk_log : 0u;
      return in_off + (chunks_log ? (row0 << logn) + sbase : base);
    };
    acc_t acc[I][V];
#pragma unroll
    for (unsigned i = 0; i < I; ++i)
#pragma unroll
      for (unsigned e = 0; e < V; ++e) acc[i][e] = 0;
    // (a vector never straddles a row: n is a multiple of V)
    auto consume = [&](unsigned t, const T *lds, unsigned sbase) {
      const T *__restrict__ w = terms_.w[t];
      const unsigned k = terms_.k[t];
      Item wv[I];
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) {
          const unsigned local = it * V;
          const size_t woff = chunks_log ? ((size_t)cm0 << logn) + jbase + local
                                         : ((size_t)((cm0 + (local >> logn)) % R) << logn) + (local & (n - 1u));
          wv[i].u = *reinterpret_cast<const item_t *>(w + woff);
        }
      }
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) {
#pragma unroll
          for (unsigned e = 0; e < V; ++e) {
            const unsigned local = it * V + e;
            const T x = chunks_log ? lds[aut_ntt_src(jbase + local, k, logn, mask2n) - sbase]
                                   : lds[(local & ~(n - 1u)) + aut_ntt_src(local & (n - 1u), k, logn, mask2n)];
            acc[i][e] += (acc_t)x * wv[i].w[e];
          }
        }
      }
    };
    if constexpr (DB) {
      item_t *buf0 = reinterpret_cast<item_t *>(mac_lds_raw);
      item_t *buf1 = buf0 + (((size_t)rows_per_tile << chunk_log) / V);
      item_t r[I];
      unsigned sbase, snext = 0;
      const item_t *src = reinterpret_cast<const item_t *>(terms_.in[0] + src_base(0, sbase));
#pragma unroll
      for (unsigned i = 0; i < I; ++i) {
        const unsigned it = threadIdx.x + i * 256u;
        if (it < items) buf0[it] = src[it];
      }
      __syncthreads();
      for (unsigned t = 0; t < nterms; ++t) {
        item_t *cur = (t & 1u) ? buf1 : buf0, *nxt = (t & 1u) ? buf0 : buf1;
        const bool more = t + 1u < nterms;
        if (more) {  // the next term's loads are in flight while this one is consumed
          src = reinterpret_cast<const item_t *>(terms_.in[t + 1u] + src_base(t + 1u, snext));
#pragma unroll
          for (unsigned i = 0; i < I; ++i) {
            const unsigned it = threadIdx.x + i * 256u;
            if (it < items) r[i] = src[it];
          }
        }
        consume(t, reinterpret_cast<const T *>(cur), sbase);
        if (more) {
#pragma unroll
          for (unsigned i = 0; i < I; ++i) {
            const unsigned it = threadIdx.x + i * 256u;
            if (it < items) nxt[it] = r[i];
          }
        }
        sbase = snext;
        __syncthreads();  // (nxt is complete; cur is free for the term after, or for the next tile)
      }
    } else {
      item_t *buf = reinterpret_cast<item_t *>(mac_lds_raw);
      for (unsigned t = 0; t < nterms; ++t) {
        unsigned sbase;
        const item_t *src = reinterpret_cast<const item_t *>(terms_.in[t] + src_base(t, sbase));
#pragma unroll
        for (unsigned i = 0; i < I; ++i) {
          const unsigned it = threadIdx.x + i * 256u;
          if (it < items) buf[it] = src[it];
        }
        __syncthreads();
        consume(t, reinterpret_cast<const T *>(buf), sbase);
        __syncthreads();  // (the next term overwrites the staging area)
      }
    }
    // one reduction, the addend, the store
#pragma unroll
    for (unsigned i = 0; i < I; ++i) {
      const unsigned it = threadIdx.x + i * 256u;
      if (it < items) {
        const unsigned local = it * V;
        const ModConst<T> &m = mc[chunks_log ? cm0 : (cm0 + (local >> logn)) % R];
        const DotRed<T> red(m);
        const T p = m.p;
        Item o, a;
        if (addend) a.u = *reinterpret_cast<const item_t *>(addend + base + local);
#pragma unroll
        for (unsigned e = 0; e < V; ++e) {
          o.w[e] = red.reduce(acc[i][e]);
          if (addend) o.w[e] = mac_add<T>(o.w[e], a.w[e], p);
        }
        *reinterpret_cast<item_t *>(out + base + local) = o.u;
      }
    }
  }
}

template <typename T>
hipError_t launch_permute_mac_ntt(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const T *const *weights,
                                  const uint64_t *ks, int terms, size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs,
                                  int double_buffer, hipStream_t st) {
  if (terms < 1 || terms > kMacMaxTerms || R == 0 || R > s.nm || comps == 0 || comps > 65535) return hipErrorInvalidValue;
  const size_t rows = batch * R;
  if (rows == 0) return hipSuccess;
  const unsigned logn = (unsigned)s.logn, mask2n = (unsigned)(2 * s.n - 1);
  MacTerms<T> a{};
  uintptr_t align = (uintptr_t)out | (uintptr_t)addend | (in_cs * sizeof(T)) | (out_cs * sizeof(T));
  for (int m = 0; m < kMacMaxTerms; ++m) {
    const int q = m < terms ? m : 0;
    if ((ks[q] & 1) == 0) return hipErrorInvalidValue;
    a.in[m] = ins[q];
    a.w[m] = weights[q];
    a.k[m] = (unsigned)(ks[q] & mask2n);
    align |= (uintptr_t)ins[q] | (uintptr_t)weights[q];
  }
  const size_t row_bytes = s.n * sizeof(T);
  const bool vec = align % 16 == 0 && row_bytes % 16 == 0;
  unsigned chunk_log = logn, rows_per_tile = 1;
  const size_t tile_max = mac_tile_bytes<T>(vec);
  while (chunk_log > 0 && ((size_t)sizeof(T) << chunk_log) > tile_max) --chunk_log;
  if (chunk_log == logn && row_bytes < tile_max) rows_per_tile = (unsigned)(tile_max / row_bytes);
  const size_t tile_bytes = ((size_t)rows_per_tile << chunk_log) * sizeof(T);  // at most kNttChunkBytes
  const size_t ntiles = chunk_log < logn ? rows << (logn - chunk_log) : (rows + rows_per_tile - 1) / rows_per_tile;
  const size_t lds = double_buffer ? 2 * tile_bytes : tile_bytes;
  const size_t cap = (size_t)1 << 16;  // grid-stride beyond 65536 tiles per component
  const dim3 g((unsigned)(ntiles < cap ? ntiles : cap), (unsigned)comps), b(256);
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
#define NFLHIP_MAC_LAUNCH(VEC, DB)                                                                                                          \
  hipLaunchKernelGGL((k_permute_mac_ntt<T, VEC, DB>), g, b, lds, st, a, out, addend, mc, (unsigned)terms, logn, (unsigned)R, chunk_log, \
                     rows_per_tile, rows, ntiles, in_cs, out_cs)
  if (vec && !double_buffer) NFLHIP_MAC_LAUNCH(true, false);
  else if (vec) NFLHIP_MAC_LAUNCH(true, true);
  else if (!double_buffer) NFLHIP_MAC_LAUNCH(false, false);
  else NFLHIP_MAC_LAUNCH(false, true);
#undef NFLHIP_MAC_LAUNCH
  return hipGetLastError();
}

#define NFLHIP_LINTRANS_INSTANCES(T)                                                                                                  \
  template hipError_t launch_permute_mac_ntt<T>(const Shape &, const DevTables &, T *, const T *, const T *const *, const T *const *, \
                                                const uint64_t *, int, size_t, size_t, size_t, size_t, size_t, int, hipStream_t);
NFLHIP_LINTRANS_INSTANCES(uint16_t)
NFLHIP_LINTRANS_INSTANCES(uint32_t)
NFLHIP_LINTRANS_INSTANCES(uint64_t)
#undef NFLHIP_LINTRANS_INSTANCES

__global__ void k_warm_lintrans() {}
hipError_t warm_lintrans(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_lintrans, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
