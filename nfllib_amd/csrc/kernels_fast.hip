// kernels_fast.hip -- 64-bit limbs, rows of 4096 words and longer: the compiled register-tiled kernels for 4096-word blocks
// (BASELINE.json configs[1], the metric shape: nfl::poly<uint64_t, 4096, 4>) -- the NFLHIP_VARIANT=hipcc cross-check and the
// general-modulus family -- and, at the end, the dispatch that serves a call from the generated assembly kernels (asm_launch.hip)
// where they take the shape and from the compiled ones where they decline.  The compiled kernels:
//
// One 256-thread workgroup (4 wavefronts) owns one RNS row = one (polynomial,
// modulus) slab of 4096 x 8 B = 32 KiB.  Each thread keeps 16 coefficients in
// VGPRs and the 12 butterfly stages run as three radix-16 register passes:
//
//   forward (Cooley-Tukey, natural -> bit-reversed; merged psi twiddles)
//     F1 stages 0-3   thread t holds x[t + 256k]      twiddles wave-uniform (SGPR)
//     -- exchange E1 through LDS (all-to-all inside the workgroup, 1 barrier)
//     F2 stages 4-7   thread (B,r) holds x[256B + r + 16k]
//     -- exchange E2 through LDS (16-lane groups: wave-local, no barrier)
//     F3 stages 8-11  thread q holds x[16q + k]
//   inverse (Gentleman-Sande) is the mirror image I1 (no exchange needed after
//   F3: same layout), E2', I2, E1', I3 with n^-1 folded into the last stage.
//
// The fused polymul kernel therefore touches HBM exactly once per operand word:
// read a, read b, write c = 3 x 32 KiB per row (the algorithmic minimum of
// SURVEY.md 8(d)); everything else stays in VGPRs/LDS.  LDS words are stored at
// index e + (e >> 4) (one pad word per 16) which makes every ds_read_b64 /
// ds_write_b64 of both exchange patterns bank-conflict free.
//
// Reference behaviour replaced: core::ntt_pow_phi (core.hpp:594-600), the
// point-wise mulmod loop (core.hpp:24-37 with ops.hpp:201-219) and
// core::invntt_pow_invphi (core.hpp:608-614).
#include "asm_launch.h"
#include "modarith64.h"

namespace nflhip {

static constexpr int kN = 1 << kLogN;   // (kLogN, kThreads: asm_launch.h)
static constexpr int kLdsWords = kN + (kN >> 4);  // padded slab

__device__ __forceinline__ int pad(int e) { return e + (e >> 4); }

// (the lazy butterflies ct_bfly / gs_bfly, canon and mul_lazy live in modarith64.h: kernels_wave.hip uses them too)

// radix-16 register passes; TW(s, g) yields the twiddle of sub-stage s (0..3), group g
template <int ARITH, class TW> __device__ __forceinline__ void ct16(u64 (&v)[16], TW tw, const Mod &k) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int half = 8 >> s;
#pragma unroll
    for (int g = 0; g < (1 << s); ++g) {
      const Tw64 w = tw(s, g);
#pragma unroll
      for (int h = 0; h < half; ++h) ct_bfly<ARITH>(v[g * 2 * half + h], v[g * 2 * half + h + half], w, k);
    }
  }
}
template <int ARITH, class TW> __device__ __forceinline__ void gs16(u64 (&v)[16], TW tw, const Mod &k) {
#pragma unroll
  for (int s = 3; s >= 0; --s) {
    const int half = 8 >> s;
#pragma unroll
    for (int g = 0; g < (1 << s); ++g) {
      const Tw64 w = tw(s, g);
#pragma unroll
      for (int h = 0; h < half; ++h) gs_bfly<ARITH>(v[g * 2 * half + h], v[g * 2 * half + h + half], w, k);
    }
  }
}

// Position of the 4096-word block this workgroup transforms inside a longer row of
// n = 4096 * 2^r words (r = 0: the row itself).  The streaming outer passes of
// kernels_generic.hip handle global stages [0, r); the passes below then cover global
// stages r .. r+11 with block index offsets folded into the twiddle indices.
struct Blk {
  int r;
  unsigned blk;
};

// ---- forward transform of the 16 words a thread loaded as x[t + 256k] ---------------
// On return thread q = t holds X[16q + k] (bit-reversed order positions), lazy in [0,4p).
template <int ARITH>
__device__ __forceinline__ void fwd_head(u64 (&v)[16], u64 *sm, const Tw64 *__restrict__ tw, const Mod &k, const int t,
                                         const bool war_barrier, const Blk bk) {
  // F1: stages r..r+3, block index of sub-stage s is blk*2^s + g: psi[2^(r+s) + ...] (wave-uniform)
  ct16<ARITH>(v, [&](int s, int g) { return tw[(1u << (bk.r + s)) + (bk.blk << s) + g]; }, k);
  if (war_barrier) __syncthreads();  // the slab may still be read by slower waves (previous transform)
  {
    const int base = t + (t >> 4);
#pragma unroll
    for (int k = 0; k < 16; ++k) sm[base + 272 * k] = v[k];
  }
  __syncthreads();
  const int B = t >> 4, r = t & 15;
  {
    const int base = 272 * B + r;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = sm[base + 17 * k];
  }
  // F2: stages 4-7 inside 256-word block B: psi[2^(4+s) + B*2^s + g]
  ct16<ARITH>(v, [&](int s, int g) { return tw[(16u << (bk.r + s)) + ((bk.blk * 16u + B) << s) + g]; }, k);
  // E2: 16-lane transpose through this wave's own LDS region (LDS is in-order per wave)
  {
    const int base = 272 * B + r;
#pragma unroll
    for (int k = 0; k < 16; ++k) sm[base + 17 * k] = v[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    const int base = 17 * t;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = sm[base + k];
  }
}
// F3: stages 8-11 inside 16-word block q = t: psi[2^(8+s) + q*2^s + g]
template <int ARITH>
__device__ __forceinline__ void fwd_tail(u64 (&v)[16], const Tw64 *__restrict__ tw, const Mod &k, const int t,
                                         const Blk bk) {
  ct16<ARITH>(v, [&](int s, int g) { return tw[(256u << (bk.r + s)) + ((bk.blk * 256u + t) << s) + g]; }, k);
}
template <int ARITH>
__device__ __forceinline__ void fwd_core(u64 (&v)[16], u64 *sm, const Tw64 *__restrict__ tw, const Mod &k, const int t,
                                         const bool war_barrier, const Blk bk) {
  fwd_head<ARITH>(v, sm, tw, k, t, war_barrier, bk);
  fwd_tail<ARITH>(v, tw, k, t, bk);
}

// ---- inverse transform of the 16 words a thread holds as X[16q + k], in [0,2p) -------
// On return thread t holds x[t + 256k]: canonical in [0,p) when r == 0 (n^-1 folded into
// global stage 0), lazy in [0,2p) when outer inverse passes follow (r > 0).
template <int ARITH>
__device__ __forceinline__ void inv_core(u64 (&v)[16], u64 *sm, const Tw64 *__restrict__ tw, const MC64 &c, const Mod &k,
                                         const int t, const Blk bk) {
  const u64 p = c.p, p2 = c.p2;
  // I1: stages 11..8; mirrored index 2m-1-j with m = 2^(8+s), j = q*2^s + g
  gs16<ARITH>(v, [&](int s, int g) { return tw[(512u << (bk.r + s)) - 1u - (((bk.blk * 256u + t) << s) + g)]; }, k);
  const int B = t >> 4, r = t & 15;
  {
    const int base = 17 * t;
#pragma unroll
    for (int k = 0; k < 16; ++k) sm[base + k] = v[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    const int base = 272 * B + r;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = sm[base + 17 * k];
  }
  // I2: stages 7..4; m = 2^(4+s), j = B*2^s + g
  gs16<ARITH>(v, [&](int s, int g) { return tw[(32u << (bk.r + s)) - 1u - (((bk.blk * 16u + B) << s) + g)]; }, k);
  {
    const int base = 272 * B + r;
#pragma unroll
    for (int k = 0; k < 16; ++k) sm[base + 17 * k] = v[k];
  }
  __syncthreads();
  {
    const int base = t + (t >> 4);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = sm[base + 272 * k];
  }
  // I3: stages r+3..r+1 (uniform twiddles), then stage r (with n^-1 folded in when r == 0)
#pragma unroll
  for (int s = 3; s >= 1; --s) {
    const int half = 8 >> s;
#pragma unroll
    for (int g = 0; g < (1 << s); ++g) {
      const Tw64 w = tw[(2u << (bk.r + s)) - 1u - ((bk.blk << s) + g)];
#pragma unroll
      for (int h = 0; h < half; ++h) gs_bfly<ARITH>(v[g * 2 * half + h], v[g * 2 * half + h + half], w, k);
    }
  }
  if (bk.r > 0) {  // plain last stage: the merged scale happens in the outer pass that owns global stage 0
    const Tw64 w = tw[(2u << bk.r) - 1u - bk.blk];
#pragma unroll
    for (int h = 0; h < 8; ++h) gs_bfly<ARITH>(v[h], v[h + 8], w, k);
    return;
  }
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    const u64 x = v[h], y = v[h + 8];
    if (ARITH == 0) {
      v[h] = mul_shoup<u64>(x + y, c.ninv, c.ninv_sh, p);
      v[h + 8] = mul_shoup<u64>(y - x + p2, c.w1ninv, c.w1ninv_sh, p);
    } else {
      v[h] = csub<u64>(shoup_acc(x + y, Tw64{c.ninv, c.ninv_sh}, 0, k), p);
      v[h + 8] = csub<u64>(shoup_acc(y - x + p2, Tw64{c.w1ninv, c.w1ninv_sh}, 0, k), p);
    }
  }
}

// ---- the metric kernel: c = INTT( NTT(a) (.) NTT(b) ), one row per workgroup ---------

template <bool B_IS_NTT, int ARITH>
__device__ __forceinline__ void polymul_body(u64 *sm, u64 *c, const u64 *a, const u64 *b, const Tw64 *__restrict__ psi,
                                             const MC64 *__restrict__ mc, int nm, size_t row) {
  const int t = threadIdx.x;
  const int cm = (int)(row % (size_t)nm);
  const MC64 mcc = mc[cm];
  const Mod k = make_mod(mcc);
  const Tw64 *tw = psi + ((size_t)cm << kLogN);
  const size_t off = row << kLogN;

  u64 va[16], vb[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) va[i] = a[off + t + 256 * i];
  const Blk bk{0, 0u};
  fwd_head<ARITH>(va, sm, tw, k, t, false, bk);
  // b's HBM loads are issued here so their latency hides under F3(a) without
  // holding 32 more VGPRs through the first two passes
  asm volatile("" ::: "memory");
  if (!B_IS_NTT) {
#pragma unroll
    for (int i = 0; i < 16; ++i) vb[i] = b[off + t + 256 * i];
  } else {
    // b already in NTT form: thread q needs B[16q + k]
    const ulonglong2 *b2 = reinterpret_cast<const ulonglong2 *>(b + off + 16 * t);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const ulonglong2 x = b2[i];
      vb[2 * i] = x.x;
      vb[2 * i + 1] = x.y;
    }
  }
  asm volatile("" ::: "memory");
  fwd_tail<ARITH>(va, tw, k, t, bk);
  if (!B_IS_NTT) fwd_core<ARITH>(vb, sm, tw, k, t, true, bk);
  // point-wise product on canonical representatives (operator*, ops.hpp:201-219)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (ARITH >= 2) {
      va[i] = mul_lazy(fold2(va[i], k), B_IS_NTT ? vb[i] : fold2(vb[i], k), mcc.mu2, k);
    } else {
      const u64 x = canon<ARITH>(va[i], k);
      const u64 y = B_IS_NTT ? vb[i] : canon<ARITH>(vb[i], k);
      va[i] = barrett<u64>::mul(x, y, k.p, mcc.mu);
    }
  }
  inv_core<ARITH>(va, sm, tw, mcc, k, t, bk);
#pragma unroll
  for (int i = 0; i < 16; ++i) c[off + t + 256 * i] = va[i];
}

// a launch over the moduli [cm0, cm0 + cmcnt) of every polynomial only (cmcnt > 0): logical block L -> block index in the batch.
// Contexts whose moduli beyond a prefix need the general arithmetic send the prefix to the generated kernels and the rest here.
__device__ __forceinline__ size_t block_of(unsigned L, int nm, int r, int cm0, int cmcnt) {
  if (cmcnt <= 0) return L;
  const unsigned rs = L >> r, bl = L & ((1u << r) - 1u);
  const size_t row = (size_t)(rs / (unsigned)cmcnt) * (size_t)nm + (size_t)cm0 + rs % (unsigned)cmcnt;
  return (row << r) | bl;
}

template <bool B_IS_NTT, int ARITH, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void k_polymul4096(u64 *c, const u64 *a, const u64 *b,
                                                                const Tw64 *__restrict__ psi,
                                                                const MC64 *__restrict__ mc, int nm, int cm0, int cmcnt) {
  __shared__ u64 sm[kLdsWords];
  polymul_body<B_IS_NTT, ARITH>(sm, c, a, b, psi, mc, nm, block_of(blockIdx.x, nm, 0, cm0, cmcnt));
}

// ---- stand-alone transforms (in place or out of place) --------------------------------
// One workgroup per 4096-word block of a row of n = 2^logn words (logn >= 12); for
// logn > 12 the streaming outer passes run before (forward) / after (inverse) these.
template <int ARITH>
__global__ __launch_bounds__(kThreads) void k_ntt_fwd4096(const u64 *src, u64 *dst, const Tw64 *__restrict__ psi,
                                                          const MC64 *__restrict__ mc, int nm, int logn, int cm0, int cmcnt) {
  __shared__ u64 sm[kLdsWords];
  const int t = threadIdx.x;
  const int r = logn - kLogN;
  const size_t blk = block_of(blockIdx.x, nm, r, cm0, cmcnt);
  const size_t row = blk >> r;
  const Blk bk{r, (unsigned)(blk & ((1u << r) - 1u))};
  const int cm = (int)(row % (size_t)nm);
  const Mod k = make_mod(mc[cm]);
  const Tw64 *tw = psi + ((size_t)cm << logn);
  const size_t off = blk << kLogN;
  u64 v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = src[off + t + 256 * i];
  fwd_core<ARITH>(v, sm, tw, k, t, false, bk);
  // thread q holds X[16q+k]: transpose inside the wave's LDS region for coalesced stores
  {
    const int base = 17 * t;
#pragma unroll
    for (int i = 0; i < 16; ++i) sm[base + i] = canon<ARITH>(v[i], k);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int w = t >> 6, l = t & 63;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int e = 1024 * w + 64 * j + l;
    dst[off + e] = sm[pad(e)];
  }
}

// MUL: the point-wise product src (.) mul (both canonical, NTT order) is fused into the load.
template <int ARITH, bool MUL>
__global__ __launch_bounds__(kThreads) void k_ntt_inv4096(const u64 *src, const u64 *mul, u64 *dst,
                                                          const Tw64 *__restrict__ psi, const MC64 *__restrict__ mc,
                                                          int nm, int logn, int cm0, int cmcnt) {
  __shared__ u64 sm[kLdsWords];
  const int t = threadIdx.x;
  const int r = logn - kLogN;
  const size_t blk = block_of(blockIdx.x, nm, r, cm0, cmcnt);
  const size_t row = blk >> r;
  const Blk bk{r, (unsigned)(blk & ((1u << r) - 1u))};
  const int cm = (int)(row % (size_t)nm);
  const MC64 mcc = mc[cm];
  const Mod k = make_mod(mcc);
  const Tw64 *tw = psi + ((size_t)cm << logn);
  const size_t off = blk << kLogN;
  const int w = t >> 6, l = t & 63;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int e = 1024 * w + 64 * j + l;
    u64 x = src[off + e];
    if (MUL) x = ARITH >= 2 ? mul_lazy(x, mul[off + e], mcc.mu2, k) : barrett<u64>::mul(x, mul[off + e], k.p, mcc.mu);
    sm[pad(e)] = x;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  u64 v[16];
  {
    const int base = 17 * t;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = sm[base + i];
  }
  inv_core<ARITH>(v, sm, tw, mcc, k, t, bk);
#pragma unroll
  for (int i = 0; i < 16; ++i) dst[off + t + 256 * i] = v[i];
}

// ---- launchers --------------------------------------------------------------------------
// The delta-form arithmetic needs delta < 2^32 (c < 2048 in params.hpp:94-97's c*2^21 - 1); every
// prime of the mirrored table qualifies, Shape::small_delta records it per context.
static inline bool fast_shape(const Shape &s) { return s.limb_bits == 64 && s.logn == kLogN; }

// ---- dispatch: the generated assembly kernels (asm_launch.hip) first, the compiled kernels above where those decline ----
hipError_t launch_polymul_blocks_asm_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a_in,
                                         const uint64_t *b_in, size_t batch, hipStream_t st, bool b_is_ntt) {
  if (s.limb_bits != 64 || s.logn < kLogN) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  return launch_asm(b_is_ntt ? kAsmPolymulNtt : kAsmPolymul, s, t, c, a_in, b_in, batch, st);
}

template <bool B_IS_NTT>
static hipError_t launch_polymul_v(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                                   unsigned rows, hipStream_t st, int cm0 = 0, int cmcnt = 0) {
  const Tw64 *psi = (const Tw64 *)t.psi;
  const MC64 *mc = (const MC64 *)t.mc;
  const int nm = (int)s.nm;
  // delta-form arithmetic (two-bit fold, one-off quotient: the assembly kernel's formulation) needs delta < 2^32; any other
  // modulus takes the Harvey ranges with the generic Shoup product.  cmcnt > 0: `rows` counts only the moduli [cm0, cm0 + cmcnt)
  if (s.small_delta) hipLaunchKernelGGL((k_polymul4096<B_IS_NTT, 3, 2>), dim3(rows), dim3(kThreads), 0, st, c, a, b, psi, mc, nm, cm0, cmcnt);
  else hipLaunchKernelGGL((k_polymul4096<B_IS_NTT, 0, 2>), dim3(rows), dim3(kThreads), 0, st, c, a, b, psi, mc, nm, cm0, cmcnt);
  return hipGetLastError();
}

// A context whose moduli beyond a prefix have delta >= 2^32 (the reference's table from its 93rd 62-bit prime on, params.hpp:82-119):
// at degree 4096 the prefix rows keep the generated delta-form kernels (grid restricted to those moduli), the others take the
// general-modulus kernels -- two launches on the stream, disjoint rows.
static inline bool split_families(const Shape &s, size_t batch) {
  return s.limb_bits == 64 && s.logn == kLogN && !s.small_delta && s.nm_small > 0 && !s.compiled_only && batch > 0 &&
         batch * (s.nm - (size_t)s.nm_small) <= 0x7fffffffull;
}

static inline bool row16k_shape(const Shape &s) { return s.limb_bits == 64 && s.logn == kLogN + 2; }
static inline bool row8k_shape(const Shape &s) { return s.limb_bits == 64 && s.logn == kLogN + 1; }
// 32768-word rows: one operand register-resident in a 1024-thread workgroup (tools/gen_polymul_asm.py build_row32k).
static inline bool row32k_shape(const Shape &s) { return s.limb_bits == 64 && s.logn == kLogN + 3 && !s.compiled_only; }
hipError_t launch_row32k_u64(const Shape &s, const DevTables &t, int mode, uint64_t *c, const uint64_t *a, const uint64_t *b,
                             size_t batch, hipStream_t st) {
  if (!row32k_shape(s)) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  // modes 4 / 5: the two halves of the composed product -- b' goes through the context's scratch in a layout only these two share;
  // 6 / 7: the same pair on incomplete transforms (b' two stages short and unreduced; BOTH launches of a product take the same pair)
  const AsmKind k = mode == 1 ? kAsmPolymulNtt32k : mode == 2 ? kAsmFwd32k : mode == 3 ? kAsmInv32k : mode == 4 ? kAsmFwd32kS :
                    mode == 6 ? kAsmFwd32kSI2 : mode == 7 ? kAsmPolymulNtt32kSI2 : kAsmPolymulNtt32kS;
  return launch_asm(k, s, t, c, a, b, batch, st);
}

hipError_t launch_polymul_fast_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                                   int b_is_ntt, size_t batch, hipStream_t st) {
  const bool inc2 = !b_is_ntt && polymul_level() == 2 && t.mc_inc[1];   // coefficient form in and out: incomplete transforms
  if (row16k_shape(s))  // a 16384-word row fits one CU: the whole product is a single launch
    return batch == 0 ? hipSuccess : launch_asm(b_is_ntt ? kAsmPolymulNtt16k : inc2 ? kAsmPolymul16kI2 : kAsmPolymul16k, s, t, c, a, b, batch, st);
  if (row8k_shape(s))   // 8192-word rows: 512 threads, two rows per CU
    return batch == 0 ? hipSuccess : launch_asm(b_is_ntt ? kAsmPolymulNtt8k : inc2 ? kAsmPolymul8kI2 : kAsmPolymul8k, s, t, c, a, b, batch, st);
  if (row32k_shape(s) && b_is_ntt) return launch_row32k_u64(s, t, 1, c, a, b, batch, st);
  if (!fast_shape(s)) return hipErrorNotSupported;
  const size_t rows = batch * s.nm;
  if (rows == 0) return hipSuccess;
  if (rows > 0x7fffffffull) return hipErrorInvalidValue;
  if (split_families(s, batch)) {
    const int ns = s.nm_small, level = b_is_ntt ? 0 : polymul_level();
    hipError_t e = hipErrorNotSupported;
    if (level == 1 || level == 2) e = launch_asm(level == 1 ? kAsmPolymulI1 : kAsmPolymulI2, s, t, c, a, b, batch, st, ns);
    if (e == hipErrorNotSupported) e = launch_asm(b_is_ntt ? kAsmPolymulNtt : kAsmPolymul, s, t, c, a, b, batch, st, ns);
    if (e == hipSuccess) {
      const unsigned rest = (unsigned)(batch * (s.nm - (size_t)ns));
      return b_is_ntt ? launch_polymul_v<true>(s, t, c, a, b, rest, st, ns, (int)s.nm - ns)
                      : launch_polymul_v<false>(s, t, c, a, b, rest, st, ns, (int)s.nm - ns);
    }
    if (e != hipErrorNotSupported) return e;
  }
  if (!b_is_ntt && s.logn == kLogN) {
    // coefficient form in AND out: the transforms may stay incomplete (tools/asmgen/incomplete.py) -- same words out
    const int level = polymul_level();
    if (level == 1 || level == 2) {
      const hipError_t e = launch_asm(level == 1 ? kAsmPolymulI1 : kAsmPolymulI2, s, t, c, a, b, batch, st);
      if (e != hipErrorNotSupported) return e;
    }
  }
  {
    const hipError_t e = launch_asm(b_is_ntt ? kAsmPolymulNtt : kAsmPolymul, s, t, c, a, b, batch, st);
    if (e != hipErrorNotSupported) return e;
  }
  return b_is_ntt ? launch_polymul_v<true>(s, t, c, a, b, (unsigned)rows, st)
                  : launch_polymul_v<false>(s, t, c, a, b, (unsigned)rows, st);
}

// inner 4096-word blocks of rows with logn >= 12 (used directly for n = 4096 and by the
// generic launch plans of kernels_generic.hip after / before their streaming outer passes)
hipError_t launch_inner_fwd_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t rows,
                                     hipStream_t st) {
  if (s.limb_bits != 64 || s.logn < kLogN) return hipErrorNotSupported;
  const size_t blocks = rows << (s.logn - kLogN);
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (rows % s.nm == 0) {  // the generated kernels index rows as (poly, modulus)
    hipError_t e = launch_asm_x2(kAsmFwd2, s, t, dst, src, rows / s.nm, st);
    if (e == hipErrorNotSupported) e = launch_asm(kAsmFwd, s, t, dst, src, nullptr, rows / s.nm, st);
    if (e != hipErrorNotSupported) return e;
  }
  const Tw64 *psi = (const Tw64 *)t.psi;
  const MC64 *mc = (const MC64 *)t.mc;
  if (rows % s.nm == 0 && split_families(s, rows / s.nm)) {
    const int ns = s.nm_small;
    hipError_t e = launch_asm_x2(kAsmFwd2, s, t, dst, src, rows / s.nm, st, ns);
    if (e == hipErrorNotSupported) e = launch_asm(kAsmFwd, s, t, dst, src, nullptr, rows / s.nm, st, ns);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_ntt_fwd4096<0>, dim3((unsigned)(rows / s.nm * (s.nm - (size_t)ns))), dim3(kThreads), 0, st, src, dst, psi, mc,
                         (int)s.nm, s.logn, ns, (int)s.nm - ns);
      return hipGetLastError();
    }
    if (e != hipErrorNotSupported) return e;
  }
  const dim3 g((unsigned)blocks), b(kThreads);
  if (s.small_delta) hipLaunchKernelGGL(k_ntt_fwd4096<3>, g, b, 0, st, src, dst, psi, mc, (int)s.nm, s.logn, 0, 0);
  else hipLaunchKernelGGL(k_ntt_fwd4096<0>, g, b, 0, st, src, dst, psi, mc, (int)s.nm, s.logn, 0, 0);
  return hipGetLastError();
}

hipError_t launch_inner_inv_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, const uint64_t *mul,
                                     uint64_t *dst, size_t rows, hipStream_t st) {
  if (s.limb_bits != 64 || s.logn < kLogN) return hipErrorNotSupported;
  const size_t blocks = rows << (s.logn - kLogN);
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (rows % s.nm == 0) {
    hipError_t e = mul ? hipErrorNotSupported : launch_asm_x2(kAsmInv2, s, t, dst, src, rows / s.nm, st);
    if (e == hipErrorNotSupported) e = launch_asm(mul ? kAsmInvMul : kAsmInv, s, t, dst, src, mul, rows / s.nm, st);
    if (e != hipErrorNotSupported) return e;
  }
  const Tw64 *psi = (const Tw64 *)t.psi;
  const MC64 *mc = (const MC64 *)t.mc;
  dim3 g((unsigned)blocks), b(kThreads);
  int cm0 = 0, cmcnt = 0;
  if (rows % s.nm == 0 && split_families(s, rows / s.nm)) {
    const int ns = s.nm_small;
    hipError_t e = mul ? hipErrorNotSupported : launch_asm_x2(kAsmInv2, s, t, dst, src, rows / s.nm, st, ns);
    if (e == hipErrorNotSupported) e = launch_asm(mul ? kAsmInvMul : kAsmInv, s, t, dst, src, mul, rows / s.nm, st, ns);
    if (e == hipSuccess) {
      cm0 = ns, cmcnt = (int)s.nm - ns;
      g = dim3((unsigned)(rows / s.nm * (size_t)cmcnt));
    } else if (e != hipErrorNotSupported) {
      return e;
    }
  }
#define NFLHIP_INV(A)                                                                                                  \
  if (mul) hipLaunchKernelGGL((k_ntt_inv4096<A, true>), g, b, 0, st, src, mul, dst, psi, mc, (int)s.nm, s.logn, cm0, cmcnt);      \
  else hipLaunchKernelGGL((k_ntt_inv4096<A, false>), g, b, 0, st, src, mul, dst, psi, mc, (int)s.nm, s.logn, cm0, cmcnt);
  if (s.small_delta) { NFLHIP_INV(2) }
  else { NFLHIP_INV(0) }
#undef NFLHIP_INV
  return hipGetLastError();
}

hipError_t launch_ntt_fwd_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t batch,
                                   hipStream_t st) {
  if (row16k_shape(s) || row8k_shape(s)) {
    if (batch == 0) return hipSuccess;
    const hipError_t e = launch_asm_x2(row16k_shape(s) ? kAsmFwd16kX2 : kAsmFwd8kX2, s, t, dst, src, batch, st);   // (batch >= 2)
    if (e != hipErrorNotSupported) return e;
    return launch_asm(row16k_shape(s) ? kAsmFwd16k : kAsmFwd8k, s, t, dst, src, nullptr, batch, st);
  }
  if (row32k_shape(s)) return launch_row32k_u64(s, t, 2, dst, src, nullptr, batch, st);
  if (!fast_shape(s)) return hipErrorNotSupported;
  return launch_inner_fwd_fast_u64(s, t, src, dst, batch * s.nm, st);
}

hipError_t launch_ntt_inv_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t batch,
                                   hipStream_t st) {
  if (row16k_shape(s)) return batch == 0 ? hipSuccess : launch_asm(kAsmInv16k, s, t, dst, src, nullptr, batch, st);
  if (row8k_shape(s)) return batch == 0 ? hipSuccess : launch_asm(kAsmInv8k, s, t, dst, src, nullptr, batch, st);
  if (row32k_shape(s)) return launch_row32k_u64(s, t, 3, dst, src, nullptr, batch, st);
  if (!fast_shape(s)) return hipErrorNotSupported;
  return launch_inner_inv_fast_u64(s, t, src, nullptr, dst, batch * s.nm, st);
}

// first-use warm-up (api.hip warm_up_device): the runtime loads a translation unit's code object at the first launch of ANY of its kernels
__global__ void k_warm_fast() {}
hipError_t warm_fast(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_fast, dim3(1), dim3(64), 0, st);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : warm_asm(st);   // ... and the generated kernels' module and launchers
}

}  // namespace nflhip
