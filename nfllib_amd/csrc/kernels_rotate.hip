// kernels_rotate.hip -- the last step of a hoisted rotation (include/nflhip.h "hoisted rotations"): for up to 32 pairs (in, out, k)
//   out = sigma^NTT_k(in [+ c0])      on [rows][n] word blocks, rows = batch * L, the DENSE layout over the first L moduli,
// the NTT-form permutation of kernels_automorph.hip (out[j] = in[aut_ntt_src(j, k)], no arithmetic) with one input per output and,
// for the pairs that ask for it, the words of c0 added mod p_(row mod L) while the input is staged.
//
// The tile plan of k_automorph_tile: a workgroup stages a contiguous tile of ONE pair's input in LDS with 16-byte loads -- a chunk
// of C = n / 2^b slots of a row, at most kNttChunkBytes, or several whole rows when a row is shorter -- and writes the one output
// chunk that tile fills (the image of its first slot under k^-1; an odd multiplier keeps the low bits of the exponent, which are the
// high bits of the slot index) with 16-byte stores.  blockIdx.y is the pair.  Every word is read once and written once.
#include "kernels.h"
#include "automorph_index.h"  // aut_ntt_src, aut_inverse_mod_2n, kNttChunkBytes

namespace nflhip {

template <typename T> struct RotPairs {
  const T *in[kRotateMaxPairs];
  T *out[kRotateMaxPairs];
  unsigned k[kRotateMaxPairs];     // the multiplier, reduced mod 2n
  unsigned kinv[kRotateMaxPairs];  // its inverse mod 2n
  unsigned add;                    // bit p: c0 is added to pair p's input
};

template <typename T> __device__ __forceinline__ T rot_add(T x, T y, T p) {
  const T s = (T)(x + y);  // both below p <= 2^(W-2): no wrap
  return s >= p ? (T)(s - p) : s;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_permute_add_ntt(const RotPairs<T> pairs, const T *__restrict__ c0, const ModConst<T> *__restrict__ mc,
                                                         unsigned logn, unsigned L, unsigned chunk_log, unsigned rows_per_tile, size_t rows,
                                                         size_t ntiles) {
  extern __shared__ uint4 rot_lds_raw[];
  T *lds = reinterpret_cast<T *>(rot_lds_raw);
  constexpr unsigned V = VEC ? 16u / sizeof(T) : 1u;
  const unsigned n = 1u << logn, mask2n = 2u * n - 1u;
  const unsigned chunks_log = logn - chunk_log;  // 0 when a tile is whole rows
  const unsigned pr = blockIdx.y;
  const T *__restrict__ in = pairs.in[pr];
  T *__restrict__ out = pairs.out[pr];
  const unsigned k = pairs.k[pr], kinv = pairs.kinv[pr];
  const bool add = c0 != nullptr && ((pairs.add >> pr) & 1u);
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
    const unsigned cm0 = (unsigned)(row0 % L);
    // stage: coalesced 16-byte loads; c0's words are added on the way in (a vector never straddles a row: n is a multiple of V)
    if (VEC) {
      const uint4 *src = reinterpret_cast<const uint4 *>(in + base);
      const unsigned nv = words / V;
      if (add) {
        const uint4 *src0 = reinterpret_cast<const uint4 *>(c0 + base);
        for (unsigned v = threadIdx.x; v < nv; v += blockDim.x) {
          union { uint4 u; T w[V]; } x, y;
          x.u = src[v];
          y.u = src0[v];
          const T p = mc[(cm0 + ((v * V) >> logn)) % L].p;
#pragma unroll
          for (unsigned e = 0; e < V; ++e) x.w[e] = rot_add<T>(x.w[e], y.w[e], p);
          rot_lds_raw[v] = x.u;
        }
      } else {
        unsigned v = threadIdx.x;
        for (; v + 3u * blockDim.x < nv; v += 4u * blockDim.x) {
          const uint4 a = src[v], b = src[v + blockDim.x], c = src[v + 2u * blockDim.x], d = src[v + 3u * blockDim.x];
          rot_lds_raw[v] = a;
          rot_lds_raw[v + blockDim.x] = b;
          rot_lds_raw[v + 2u * blockDim.x] = c;
          rot_lds_raw[v + 3u * blockDim.x] = d;
        }
        for (; v < nv; v += blockDim.x) rot_lds_raw[v] = src[v];
      }
    } else {
      for (unsigned w = threadIdx.x; w < words; w += blockDim.x) {
        T x = in[base + w];
        if (add) x = rot_add<T>(x, c0[base + w], mc[(cm0 + (w >> logn)) % L].p);
        lds[w] = x;
      }
    }
    __syncthreads();
    unsigned dst_chunk = 0;
    size_t obase = base;
    if (chunks_log) {  // the output chunk this input chunk fills: the forward image of its first slot, by k^-1
      dst_chunk = aut_ntt_src(src_chunk << chunk_log, kinv, logn, mask2n) >> chunk_log;
      obase = (row0 << logn) + ((size_t)dst_chunk << chunk_log);
    }
    T *o = out + obase;
    const unsigned jbase = dst_chunk << chunk_log, sbase = src_chunk << chunk_log;
    if (VEC) {
      for (unsigned v = threadIdx.x; v < words / V; v += blockDim.x) {
        union { uint4 u; T w[V]; } pk;
#pragma unroll
        for (unsigned e = 0; e < V; ++e) {
          const unsigned local = v * V + e;
          pk.w[e] = chunks_log ? lds[aut_ntt_src(jbase + local, k, logn, mask2n) - sbase]
                               : lds[(local & ~(n - 1u)) + aut_ntt_src(local & (n - 1u), k, logn, mask2n)];
        }
        reinterpret_cast<uint4 *>(o)[v] = pk.u;
      }
    } else {
      for (unsigned w = threadIdx.x; w < words; w += blockDim.x)
        o[w] = chunks_log ? lds[aut_ntt_src(jbase + w, k, logn, mask2n) - sbase] : lds[(w & ~(n - 1u)) + aut_ntt_src(w & (n - 1u), k, logn, mask2n)];
    }
    __syncthreads();  // (the next tile overwrites the staging area)
  }
}

template <typename T>
hipError_t launch_permute_add_ntt(const Shape &s, const DevTables &t, T *const *outs, const T *const *ins, const uint64_t *ks, unsigned add_mask,
                                  int pairs, const T *c0, size_t L, size_t batch, hipStream_t st) {
  if (pairs < 1 || pairs > kRotateMaxPairs || L == 0 || L > s.nm) return hipErrorInvalidValue;
  const size_t rows = batch * L;
  if (rows == 0) return hipSuccess;
  const unsigned logn = (unsigned)s.logn, mask2n = (unsigned)(2 * s.n - 1);
  RotPairs<T> a{};
  a.add = c0 ? add_mask : 0u;
  uintptr_t align = a.add ? (uintptr_t)c0 : 0;
  for (int m = 0; m < kRotateMaxPairs; ++m) {
    const int q = m < pairs ? m : 0;
    if ((ks[q] & 1) == 0) return hipErrorInvalidValue;
    a.in[m] = ins[q];
    a.out[m] = outs[q];
    a.k[m] = (unsigned)(ks[q] & mask2n);
    a.kinv[m] = aut_inverse_mod_2n(a.k[m], mask2n);
    align |= (uintptr_t)ins[q] | (uintptr_t)outs[q];
  }
  const size_t row_bytes = s.n * sizeof(T);
  const bool vec = align % 16 == 0 && row_bytes % 16 == 0;
  unsigned chunk_log = logn, rows_per_tile = 1;
  while (chunk_log > 0 && ((size_t)sizeof(T) << chunk_log) > kNttChunkBytes) --chunk_log;
  if (chunk_log == logn && row_bytes < kNttChunkBytes) rows_per_tile = (unsigned)(kNttChunkBytes / row_bytes);
  const size_t tile_words = (size_t)rows_per_tile << chunk_log;
  const size_t ntiles = chunk_log < logn ? rows << (logn - chunk_log) : (rows + rows_per_tile - 1) / rows_per_tile;
  const size_t lds = tile_words * sizeof(T);  // at most kNttChunkBytes
  const size_t cap = (size_t)1 << 16;         // grid-stride beyond 65536 tiles per pair
  const dim3 g((unsigned)(ntiles < cap ? ntiles : cap), (unsigned)pairs), b(256);
  const ModConst<T> *mc = (const ModConst<T> *)t.mc;
  if (vec) hipLaunchKernelGGL((k_permute_add_ntt<T, true>), g, b, lds, st, a, c0, mc, logn, (unsigned)L, chunk_log, rows_per_tile, rows, ntiles);
  else hipLaunchKernelGGL((k_permute_add_ntt<T, false>), g, b, lds, st, a, c0, mc, logn, (unsigned)L, chunk_log, rows_per_tile, rows, ntiles);
  return hipGetLastError();
}

#define NFLHIP_ROTATE_INSTANCES(T)                                                                                                     \
  template hipError_t launch_permute_add_ntt<T>(const Shape &, const DevTables &, T *const *, const T *const *, const uint64_t *, unsigned, \
                                                int, const T *, size_t, size_t, hipStream_t);
NFLHIP_ROTATE_INSTANCES(uint16_t)
NFLHIP_ROTATE_INSTANCES(uint32_t)
NFLHIP_ROTATE_INSTANCES(uint64_t)
#undef NFLHIP_ROTATE_INSTANCES

__global__ void k_warm_rotate() {}
hipError_t warm_rotate(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_rotate, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
