// kernels_automorph.hip -- Galois automorphisms sigma_k : a(X) -> a(X^k) mod (X^n + 1), k odd, on [rows][n] word blocks.
//
// Both maps are written as GATHERS, so every output word is stored exactly once, in order, with 16-byte stores:
//   coefficient form  out[o] = +-in[i0 mod n],  i0 = o * k^-1 mod 2n,  minus (p - x, 0 stays 0) when i0 >= n
//   NTT form          out[j] = in[rev(((k * (2 rev(j) + 1)) mod 2n) >> 1)]   (rev = log2(n)-bit reversal; no arithmetic)
// (include/nflhip.h states both maps; DESIGN.md "Galois automorphisms" derives them.)  All index arithmetic is 32-bit:
// 2n divides 2^32, so a product that wraps still has the right residue mod 2n.  No index tables.
//
// Plans (launch_automorphism picks one per call):
//   tile  -- a workgroup stages a contiguous TILE of the input in LDS with 16-byte loads, then writes every output's image
//            of that tile.  NTT form: the tile is a chunk of C = n / 2^b contiguous slots, and the chunk property (an odd
//            multiplier keeps the low bits of the exponent, which are the HIGH bits of the slot index) makes the image of
//            one input chunk exactly one output chunk, whatever the degree.  Coefficient form: the tile is one or more
//            WHOLE rows (residue classes are strided, so a row has no smaller closed piece); rows up to kCoeffStageBytes.
//            Every output of a multi call is written from the same staged tile: the input is read once.
//   l2    -- coefficient form, rows above kCoeffStageBytes (64-bit limbs at n = 16384 .. 65536): a workgroup writes one
//            contiguous output chunk and gathers its words straight from global memory; the grid is remapped so that all
//            chunks of a row run on ONE XCD, whose 4 MiB L2 then holds the row while its scattered reads are served.
#include "kernels.h"
#include "automorph_index.h"  // aut_rev, aut_ntt_src, aut_inverse_mod_2n, kNttChunkBytes

namespace nflhip {

static constexpr int kAutMaxOut = 16;            // include/nflhip.h NFLHIP_AUTOMORPHISM_MAX_OUTPUTS
static constexpr size_t kCoeffStageBytes = 65536;  // largest row the coefficient-form tile plan stages whole
static constexpr size_t kL2ChunkBytes = 16384;   // output chunk of one workgroup of the l2 plan

template <typename T> struct AutOuts {
  T *out[kAutMaxOut];
  unsigned k[kAutMaxOut];     // the multiplier, reduced mod 2n
  unsigned kinv[kAutMaxOut];  // its inverse mod 2n
  int count;
};

template <typename T> __device__ __forceinline__ T aut_neg(T x, T p) { return x ? (T)(p - x) : (T)0; }

// one output word of the tile plan: `local` is the output word's offset inside its tile-sized destination block
template <typename T, bool NTT>
__device__ __forceinline__ T aut_tile_word(const T *lds, unsigned local, unsigned logn, unsigned chunk_log, unsigned dst_chunk,
                                           unsigned src_chunk, unsigned k, unsigned kinv, unsigned mask2n, const ModConst<T> *mc,
                                           unsigned cm0, unsigned nm) {
  if (NTT) {
    if (chunk_log < logn) {  // one chunk of a row
      const unsigned j = (dst_chunk << chunk_log) + local;
      return lds[aut_ntt_src(j, k, logn, mask2n) - (src_chunk << chunk_log)];
    }
    const unsigned r = local >> logn, j = local & ((1u << logn) - 1u);
    return lds[(r << logn) + aut_ntt_src(j, k, logn, mask2n)];
  }
  const unsigned r = local >> logn, o = local & ((1u << logn) - 1u);
  const unsigned i0 = (o * kinv) & mask2n;
  const T x = lds[(r << logn) + (i0 & ((1u << logn) - 1u))];
  return (i0 >> logn) ? aut_neg(x, mc[r ? (cm0 + r) % nm : cm0].p) : x;
}

// Tile plan.  Tile t covers `tile_words` contiguous input words: rows [t * rows_per_tile, ...) when chunk_log == logn, else
// chunk (t mod n/C) of row (t / (n/C)).  VEC: tiles and rows are whole 16-byte vectors and every pointer is 16-byte aligned.
template <typename T, bool NTT, bool VEC>
__global__ void __launch_bounds__(1024) k_automorph_tile(const T *__restrict__ in, AutOuts<T> outs, const ModConst<T> *__restrict__ mc,
                                                         unsigned logn, unsigned nm, unsigned chunk_log, unsigned rows_per_tile,
                                                         size_t rows, size_t ntiles) {
  extern __shared__ uint4 aut_lds_raw[];
  T *lds = reinterpret_cast<T *>(aut_lds_raw);
  constexpr unsigned V = VEC ? 16u / sizeof(T) : 1u;
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;  // 0 when a tile is whole rows
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    size_t row0, base;
    unsigned words, src_chunk = 0;
    if (chunks_log) {
      row0 = t >> chunks_log;
      src_chunk = (unsigned)(t & ((1u << chunks_log) - 1u));
      base = (row0 << logn) + ((size_t)src_chunk << chunk_log);
      words = 1u << chunk_log;
    } else {
      row0 = t * rows_per_tile;
      const size_t nr = rows - row0 < rows_per_tile ? rows - row0 : rows_per_tile;
      base = row0 << logn;
      words = (unsigned)nr << logn;
    }
    // stage: coalesced 16-byte loads, four in flight per thread
    if (VEC) {
      const uint4 *src = reinterpret_cast<const uint4 *>(in + base);
      uint4 *dst = aut_lds_raw;
      const unsigned nv = words / V;
      unsigned v = threadIdx.x;
      for (; v + 3u * blockDim.x < nv; v += 4u * blockDim.x) {
        const uint4 a = src[v], b = src[v + blockDim.x], c = src[v + 2u * blockDim.x], d = src[v + 3u * blockDim.x];
        dst[v] = a;
        dst[v + blockDim.x] = b;
        dst[v + 2u * blockDim.x] = c;
        dst[v + 3u * blockDim.x] = d;
      }
      for (; v < nv; v += blockDim.x) dst[v] = src[v];
    } else {
      for (unsigned w = threadIdx.x; w < words; w += blockDim.x) lds[w] = in[base + w];
    }
    __syncthreads();
    const unsigned cm0 = (unsigned)(row0 % nm);
    for (int m = 0; m < outs.count; ++m) {
      const unsigned k = outs.k[m], kinv = outs.kinv[m];
      unsigned dst_chunk = 0;
      size_t obase = base;
      if (NTT && chunks_log) {  // the output chunk this input chunk fills: the forward image of its first slot, by k^-1
        const unsigned j0 = src_chunk << chunk_log;
        dst_chunk = aut_ntt_src(j0, kinv, logn, mask2n) >> chunk_log;
        obase = (row0 << logn) + ((size_t)dst_chunk << chunk_log);
      }
      T *out = outs.out[m] + obase;
      if (VEC) {
        for (unsigned v = threadIdx.x; v < words / V; v += blockDim.x) {
          union { uint4 u; T w[V]; } pk;
#pragma unroll
          for (unsigned e = 0; e < V; ++e)
            pk.w[e] = aut_tile_word<T, NTT>(lds, v * V + e, logn, chunk_log, dst_chunk, src_chunk, k, kinv, mask2n, mc, cm0, nm);
          reinterpret_cast<uint4 *>(out)[v] = pk.u;
        }
      } else {
        for (unsigned w = threadIdx.x; w < words; w += blockDim.x)
          out[w] = aut_tile_word<T, NTT>(lds, w, logn, chunk_log, dst_chunk, src_chunk, k, kinv, mask2n, mc, cm0, nm);
      }
    }
    __syncthreads();  // (the next tile overwrites the staging area)
  }
}

// l2 plan (coefficient form, large rows).  Logical tile t = output chunk (t mod n/C) of row (t / (n/C)); the physical workgroup b
// runs tile (b mod 8) * per_xcd + b / 8, so a run of per_xcd consecutive tiles -- whole rows -- shares the blocks that
// are dealt to one XCD (placement only changes speed, never the result).
template <typename T>
__global__ void __launch_bounds__(256) k_automorph_l2(const T *__restrict__ in, AutOuts<T> outs, const ModConst<T> *__restrict__ mc,
                                                      unsigned logn, unsigned nm, unsigned chunk_log, size_t ntiles, size_t per_xcd) {
  constexpr unsigned V = 16u / sizeof(T);
  const size_t t = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u;
  if (t >= ntiles) return;
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;
  const size_t row = t >> chunks_log;
  const unsigned chunk = (unsigned)(t & ((1u << chunks_log) - 1u));
  const T *src = in + (row << logn);
  const T p = mc[row % nm].p;
  for (int m = 0; m < outs.count; ++m) {
    const unsigned kinv = outs.kinv[m];
    T *out = outs.out[m] + (row << logn) + ((size_t)chunk << chunk_log);
    for (unsigned v = threadIdx.x; v < (1u << chunk_log) / V; v += blockDim.x) {
      union { uint4 u; T w[V]; } pk;
#pragma unroll
      for (unsigned e = 0; e < V; ++e) {
        const unsigned o = (chunk << chunk_log) + v * V + e;
        const unsigned i0 = (o * kinv) & mask2n;
        const T x = src[i0 & (n - 1u)];
        pk.w[e] = (i0 >> logn) ? aut_neg(x, p) : x;
      }
      reinterpret_cast<uint4 *>(out)[v] = pk.u;
    }
  }
}

template <typename T>
hipError_t launch_automorphism(const Shape &s, const DevTables &t, T *const *outs, const uint64_t *ks, int count, const T *in,
                               int ntt_form, size_t batch, hipStream_t st) {
  if (count < 1 || count > kAutMaxOut) return hipErrorInvalidValue;
  const size_t rows = batch * s.nm;
  if (rows == 0) return hipSuccess;
  const unsigned logn = (unsigned)s.logn, mask2n = (unsigned)(2 * s.n - 1);
  AutOuts<T> a{};
  a.count = count;
  uintptr_t align = (uintptr_t)in;
  for (int m = 0; m < count; ++m) {
    if ((ks[m] & 1) == 0) return hipErrorInvalidValue;
    a.out[m] = outs[m];
    a.k[m] = (unsigned)(ks[m] & mask2n);
    a.kinv[m] = aut_inverse_mod_2n(a.k[m], mask2n);
    align |= (uintptr_t)outs[m];
  }
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  const size_t row_bytes = s.n * sizeof(T);
  const bool vec = align % 16 == 0 && row_bytes % 16 == 0;
  if (!ntt_form && row_bytes > kCoeffStageBytes) {
    if (!vec) return hipErrorInvalidValue;  // (rows this long are whole vectors: only a misaligned pointer gets here)
    unsigned chunk_log = logn;
    while (((size_t)sizeof(T) << chunk_log) > kL2ChunkBytes) --chunk_log;
    const size_t ntiles = rows << (logn - chunk_log);
    const size_t per_xcd = (ntiles + 7) / 8;
    hipLaunchKernelGGL((k_automorph_l2<T>), dim3((unsigned)(per_xcd * 8)), dim3(256), 0, st, in, a, mc, logn, (unsigned)s.nm,
                       chunk_log, ntiles, per_xcd);
    return hipGetLastError();
  }
  // tile plan: NTT form in chunks of at most kNttChunkBytes; coefficient form in whole rows, several per tile when short
  unsigned chunk_log = logn, rows_per_tile = 1;
  if (ntt_form) {
    while (chunk_log > 0 && ((size_t)sizeof(T) << chunk_log) > kNttChunkBytes) --chunk_log;
  }
  if (chunk_log == logn && row_bytes < kNttChunkBytes) rows_per_tile = (unsigned)(kNttChunkBytes / row_bytes);
  const size_t tile_words = (size_t)rows_per_tile << chunk_log;
  const size_t ntiles = chunk_log < logn ? rows << (logn - chunk_log) : (rows + rows_per_tile - 1) / rows_per_tile;
  const size_t lds = tile_words * sizeof(T);
  const unsigned threads = lds >= 65536 ? 1024u : lds >= 32768 ? 512u : 256u;
  const size_t cap = (size_t)1 << 20;  // grid-stride beyond a million tiles
  const dim3 g((unsigned)(ntiles < cap ? ntiles : cap)), b(threads);
  const unsigned nm = (unsigned)s.nm;
  if (ntt_form) {
    if (vec) hipLaunchKernelGGL((k_automorph_tile<T, true, true>), g, b, lds, st, in, a, mc, logn, nm, chunk_log, rows_per_tile, rows, ntiles);
    else hipLaunchKernelGGL((k_automorph_tile<T, true, false>), g, b, lds, st, in, a, mc, logn, nm, chunk_log, rows_per_tile, rows, ntiles);
  } else {
    if (vec) hipLaunchKernelGGL((k_automorph_tile<T, false, true>), g, b, lds, st, in, a, mc, logn, nm, chunk_log, rows_per_tile, rows, ntiles);
    else hipLaunchKernelGGL((k_automorph_tile<T, false, false>), g, b, lds, st, in, a, mc, logn, nm, chunk_log, rows_per_tile, rows, ntiles);
  }
  return hipGetLastError();
}

template hipError_t launch_automorphism<uint16_t>(const Shape &, const DevTables &, uint16_t *const *, const uint64_t *, int,
                                                  const uint16_t *, int, size_t, hipStream_t);
template hipError_t launch_automorphism<uint32_t>(const Shape &, const DevTables &, uint32_t *const *, const uint64_t *, int,
                                                  const uint32_t *, int, size_t, hipStream_t);
template hipError_t launch_automorphism<uint64_t>(const Shape &, const DevTables &, uint64_t *const *, const uint64_t *, int,
                                                  const uint64_t *, int, size_t, hipStream_t);

__global__ void k_warm_automorph() {}
hipError_t warm_automorph(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_automorph, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
