// asm_launch.hip -- host side of the generated assembly kernels (tools/gen_polymul_asm.py, tools/asmgen/, tools/gen_row*_asm.py):
// the embedded code object, the table of its kernels (asm_kernels.def) and one launcher per kernarg layout, for every limb
// width and every row length from 8 to 65536 words.  A launcher returns hipErrorNotSupported for what its kernels do not take
// and callers chain on that value to the compiled kernels, so the ORDER of a launcher's checks is part of its contract.
#include <atomic>
#include <mutex>

#include "asm_launch.h"

namespace nflhip {

static const unsigned char kPolymulHsaco[] = {
#include "polymul4096_hsaco.inc"
};
struct AsmInfo {
  const char *name;
  unsigned char row, level, whole;  // (asm_kernels.def; 0 where the column is empty)
};
static const AsmInfo kAsmInfo[kAsmCount] = {
#define X(kind, name, row, level, whole) {name, row + 0, level + 0, whole + 0},
#include "asm_kernels.def"
#undef X
};
struct AsmKernel {
  hipModule_t mod = nullptr;
  hipFunction_t fn[kAsmCount] = {};
  std::once_flag once;
};
static AsmKernel g_asm[16];  // per device

static hipFunction_t asm_fn(AsmKind kind) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  AsmKernel &k = g_asm[dev];
  std::call_once(k.once, [&k] {  // contexts may be used from several host threads
    if (hipModuleLoadData(&k.mod, kPolymulHsaco) != hipSuccess) {
      k.mod = nullptr;
      (void)hipGetLastError();
      return;
    }
    for (int i = 0; i < kAsmCount; ++i)
      if (hipModuleGetFunction(&k.fn[i], k.mod, kAsmInfo[i].name) != hipSuccess) {
        k.fn[i] = nullptr;
        (void)hipGetLastError();
      }
  });
  return k.fn[kind];
}

// every generated kernel reads its arguments as one packed block; `bytes` is the kernarg segment the kernel declares
static hipError_t launch_packed(hipFunction_t fn, unsigned gx, unsigned gy, unsigned threads, void *args, size_t bytes, hipStream_t st) {
  void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  return hipModuleLaunchKernel(fn, gx, gy, 1, threads, 1, 1, 0, st, nullptr, extra);
}

// The ring-mode kernels (rows of 8192 / 16384 / 32768 words) read the twiddle table with its last four stages lane-major
// (DevTables::psi_lm, tools/gen_polymul_asm.py tw_base_lm); the 4096-word kernels read the natural table.
// Building with EXTRA=-DNFLHIP_NATURAL_TWIDDLES and NFL_GEN_NATURAL_TWIDDLES=1 in the generators' environment gives the
// natural-order variant of the former for same-box comparisons (profiles/r03_lane_major_twiddles.txt).
#ifdef NFLHIP_NATURAL_TWIDDLES
#define PSI_LM(t) ((t).psi)
#else
#define PSI_LM(t) ((t).psi_lm)
#endif

// which n = 4096 product serves coefficient-form operands: 0 = complete transforms (nflhip_polymul4096nt_asm), 1 / 2 = that many
// stages dropped each way.  Default chosen by measurement (profiles/r06_incomplete_ab.txt); the test hook switches it per process.
#ifndef NFLHIP_POLYMUL_LEVEL
#define NFLHIP_POLYMUL_LEVEL 2
#endif
static std::atomic<int> g_polymul_level{NFLHIP_POLYMUL_LEVEL};
int polymul_level() { return g_polymul_level.load(); }   // (api.hip reads it ONCE per product: the launches of a chunked plan must agree)
extern "C" int nflhip_debug_polymul_level(int level) {   // include/nflhip_debug.h; returns the previous setting; level < 0 only reads
  const int old = g_polymul_level.load();
  if (level >= 0 && level <= 2) g_polymul_level.store(level);
  return old;
}

// ---- the standard arguments (dst, src_a, src_b, psi, mc, nm, logn) -------------------------------------------------------
struct StdArgs {
  void *c;
  const void *a, *b, *psi, *mc;
  int nm, logn;
};
static_assert(sizeof(StdArgs) == 48, "kernarg layout of the standard-argument kernels (ARGS_STD)");
static inline unsigned std_threads(int row) { return row >= kLogN + 2 ? 1024u : (unsigned)kThreads << (row - kLogN); }
static inline bool std_context(const Shape &s, int ny) {
  return !s.compiled_only && (s.small_delta || (ny > 0 && ny <= s.nm_small)) && s.nm <= 65535;
}

hipError_t launch_asm(AsmKind kind, const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                      size_t batch, hipStream_t st, int ny) {
  if (!std_context(s, ny)) return hipErrorNotSupported;
  hipFunction_t fn = asm_fn(kind);
  if (!fn) return hipErrorNotSupported;
  const AsmInfo &k = kAsmInfo[kind];
  // (level 1 / 2: their own ModConst records -- scale of the shorter inverse, 2^127 Barrett constant -- where the context has them)
  const void *mc = k.level ? t.mc_inc[k.level - 1] : t.mc;
  if (!k.row || !mc || s.logn < k.row || (k.whole && s.logn != k.row)) return hipErrorNotSupported;
  StdArgs args = {c, a, b, k.row > kLogN ? PSI_LM(t) : t.psi, mc, (int)s.nm, s.logn};
  const size_t gx = batch << (s.logn - k.row);
  if (gx > 0x7fffffffull) return hipErrorInvalidValue;
  return launch_packed(fn, (unsigned)gx, (unsigned)(ny > 0 ? ny : s.nm), std_threads(k.row), &args, sizeof(args), st);
}

// n = 4096 stand-alone transforms of a batch: two polynomials (same modulus) per workgroup, like the a / b operands of the
// fused product -- twice the bytes in flight per workgroup and one set of twiddle loads for both rows.
// (the same for rows of 16384 / 8192 words: the forward half of their fused products without the product)
hipError_t launch_asm_x2(AsmKind kind, const Shape &s, const DevTables &t, uint64_t *dst, const uint64_t *src, size_t batch,
                         hipStream_t st, int ny) {
  const AsmInfo &k = kAsmInfo[kind];
  if (!std_context(s, ny) || !k.row || s.logn != k.row) return hipErrorNotSupported;
  if (batch < 2 || batch > 0x7fffffffull) return hipErrorNotSupported;
  hipFunction_t fn = asm_fn(kind);
  if (!fn) return hipErrorNotSupported;
  struct {
    StdArgs std;
    int count;
  } args = {{dst, src, nullptr, k.row > kLogN ? PSI_LM(t) : t.psi, t.mc, (int)s.nm, s.logn}, (int)batch};
  static_assert(sizeof(args) == 56, "kernarg layout of the two-row kernels (ARGS_STD + count)");
  // 52 < sizeof: the struct's trailing padding is not part of the kernel's declared kernarg segment
  return launch_packed(fn, (unsigned)((batch + 1) / 2), (unsigned)(ny > 0 ? ny : s.nm), std_threads(k.row), &args, 52, st);
}

// transform-fused pipelines (tools/gen_polymul_asm.py build_fused, kernarg ARGS_FUSED): one 256-thread workgroup per
// (batch element, modulus); the intermediate polynomials of `x.ntt_pow_phi(); r = x * k + e` / `(b - a * s).invntt_pow_invphi()`
// (tests/nfllib_demo_main_op.cpp:26-58) never reach HBM
static std::atomic<int> g_fused_grid{0};
extern "C" void nflhip_debug_fused_grid(int mode) { g_fused_grid.store(mode); }  // include/nflhip_debug.h
hipError_t launch_fused_asm_u64(const Shape &s, const DevTables &t, int kind, uint64_t *out0, uint64_t *out1,
                                const void *const *x, const unsigned *xstride, const int *xfmt, const void *const *k,
                                const unsigned *kstride, size_t batch, hipStream_t st) {
  if (s.limb_bits != 64 || s.logn < kLogN || s.logn > kLogN + 3 || s.compiled_only || !s.small_delta || s.nm > 65535 || kind < 0 || kind > 3)
    return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  if (batch > 0x7fffffffull) return hipErrorInvalidValue;
  if (s.logn == kLogN + 3) {
    // rows of 32768 words: the inverse pipelines only (one operand register-resident, b and the key streamed through the idle
    // twiddle ring: build_row32k), dense a / b, the key one polynomial for the batch or one per element
    if (kind < 2 || xstride[0] != 1 || xstride[1] != 1 || kstride[0] > 1 || xfmt[0] || xfmt[1]) return hipErrorNotSupported;
    hipFunction_t fn32 = asm_fn(kind == 2 ? kAsmFused32kFmsInv : kAsmFused32kFmaInv);
    if (!fn32) return hipErrorNotSupported;
    struct {
      StdArgs std;
      const void *k;
      int kstride, pad;
    } a32 = {{out0, x[0], x[1], PSI_LM(t), t.mc, (int)s.nm, s.logn}, k[0], (int)kstride[0], 0};
    static_assert(sizeof(a32) == 64, "kernarg layout of nflhip_fused_*_inv32768_asm (ARGS_STD + key pointer + stride flag)");
    // 60 < sizeof: `pad` is the struct's trailing padding, not part of the kernel's declared kernarg segment
    return launch_packed(fn32, (unsigned)batch, (unsigned)s.nm, 1024, &a32, 60, st);
  }
  // rows of 4096 words: 256 threads on the pair-mode map; 8192 / 16384: the row-resident ring-mode map, 512 / 1024 threads,
  // lane-major twiddle copy
  const int rows_log = s.logn - kLogN;
  const int forced = g_fused_grid.load(std::memory_order_relaxed);
  // rows of 4096 words have two register maps: pair mode (168 VGPRs, two interleaved butterflies, three workgroups per CU)
  // and ring mode (128 VGPRs, one butterfly at a time, four per CU).  Measured same-box (profiles/r04_ring_vs_pair_4096.txt):
  // the inverse pipelines -- 70 % VALU, the rest exposed operand latency -- gain 4 % from the fourth workgroup; the forward
  // ones are VALU-bound and keep pair mode.  Mode 3 of the debug hook swaps the choice (A/B runs).
  const bool ring4k = rows_log == 0 && ((kind >= 2) != (forced == 3));
  // the four kinds (0 enc2, 1 fma_fwd, 2 fms_inv, 3 fma_inv) of a row length lie in that order
  static_assert(kAsmFusedFmaFwd == kAsmFusedEnc2 + 1 && kAsmFusedFmsInv == kAsmFusedEnc2 + 2 && kAsmFusedFmaInv == kAsmFusedEnc2 + 3, "fused kinds, 4096");
  static_assert(kAsmFused8kFmaFwd == kAsmFused8kEnc2 + 1 && kAsmFused8kFmsInv == kAsmFused8kEnc2 + 2 && kAsmFused8kFmaInv == kAsmFused8kEnc2 + 3, "fused kinds, 8192");
  static_assert(kAsmFused16kFmaFwd == kAsmFused16kEnc2 + 1 && kAsmFused16kFmsInv == kAsmFused16kEnc2 + 2 && kAsmFused16kFmaInv == kAsmFused16kEnc2 + 3, "fused kinds, 16384");
  static_assert(kAsmFusedFmaFwdR == kAsmFusedEnc2R + 1 && kAsmFusedFmsInvR == kAsmFusedEnc2R + 2 && kAsmFusedFmaInvR == kAsmFusedEnc2R + 3, "fused kinds, 4096 ring mode");
  hipFunction_t fn = ring4k ? asm_fn((AsmKind)(kAsmFusedEnc2R + kind))
                            : asm_fn((AsmKind)((rows_log == 0 ? kAsmFusedEnc2 : rows_log == 1 ? kAsmFused8kEnc2 : kAsmFused16kEnc2) + kind));
  if (!fn) return hipErrorNotSupported;
  const int nx = kind == 0 ? 3 : 2, nk = kind == 0 ? 2 : 1;
  struct {
    void *out0, *out1;
    const void *x[3], *k[2], *psi, *mc;
    int nm, logn, fmt;
    unsigned sx[3], sk[2], count, magic;
  } args = {};
  static_assert(sizeof(args) == 112, "kernarg layout of nflhip_fused_*_asm (ARGS_FUSED)");
  args.out0 = out0;
  args.out1 = out1;
  for (int i = 0; i < nx; ++i) {
    // (the stride multiplies the batch index in 32 bits inside the kernel)
    if ((uint64_t)xstride[i] * (batch - 1) > 0xffffffffull || xfmt[i] < 0 || xfmt[i] > 3 || (kind >= 2 && xfmt[i])) return hipErrorInvalidValue;
    args.x[i] = x[i];
    args.sx[i] = xstride[i];
    args.fmt |= xfmt[i] << (4 * i);
  }
  for (int i = 0; i < nk; ++i) {
    if ((uint64_t)kstride[i] * (batch - 1) > 0xffffffffull) return hipErrorInvalidValue;
    args.k[i] = k[i];
    args.sk[i] = kstride[i];
  }
  args.psi = rows_log || ring4k ? PSI_LM(t) : t.psi;
  args.mc = t.mc;
  args.nm = (int)s.nm;
  args.logn = s.logn;
  args.count = (unsigned)batch;
  // forward kinds with more than one modulus: the nm rows of a batch element back to back on one XCD (1-D grid, the kernel
  // deals the workgroups itself), so that compact inputs -- one copy for all moduli -- come from HBM once
  const size_t groups = (batch + 7) / 8, wgs = groups * 8 * s.nm;
  const bool fits = wgs <= 0x7fffffffull && groups * s.nm < (0xffffffffull / s.nm);
  // (rows of 8192 / 16384 words keep the 2-D grid by default: with the nm rows of an element on one XCD that L2 holds nm
  // twiddle tables and the key rows of nm moduli at once -- measured at 16384 x 8: encrypt traffic 1.24x -> 1.32x)
  const bool remap = fits && forced != 1 && (forced == 2 || (rows_log == 0 && kind < 2 && s.nm > 1 && args.fmt != 0));
  args.magic = remap ? (unsigned)(0x100000000ull / s.nm + 1) : 0u;
  const unsigned threads = (unsigned)(kThreads << rows_log);
  if (remap) return launch_packed(fn, (unsigned)wgs, 1, threads, &args, sizeof(args), st);
  return launch_packed(fn, (unsigned)batch, (unsigned)s.nm, threads, &args, sizeof(args), st);
}

// rows of 32768 words, forward side (tools/gen_polymul_asm.py build_row32k fwd_i8 / fma_fwd_i8 / enc2_i8): a compact Gaussian
// polynomial (one signed byte per coefficient) -> the NTT words of every modulus; and out0 = NTT(x) k0 + e0' [, out1 = NTT(x) k1 +
// e1'] with x compact, the keys one polynomial each (NTT form) and e' ALREADY transformed words (what the first kernel wrote)
hipError_t launch_row32k_fwd_i8_u64(const Shape &s, const DevTables &t, uint64_t *dst, const void *x8, size_t batch, hipStream_t st) {
  if (s.limb_bits != 64 || s.logn != kLogN + 3 || s.compiled_only || !s.small_delta || s.nm > 65535) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  if (batch > 0x7fffffffull) return hipErrorInvalidValue;
  return launch_asm(kAsmFwd32kI8, s, t, dst, (const uint64_t *)x8, nullptr, batch, st);   // (standard arguments, a = the bytes)
}
hipError_t launch_row32k_fwd_fma_i8_u64(const Shape &s, const DevTables &t, uint64_t *out0, uint64_t *out1, const void *x8,
                                        const uint64_t *k0, const uint64_t *e0p, const uint64_t *k1, const uint64_t *e1p, size_t batch,
                                        hipStream_t st) {
  if (s.limb_bits != 64 || s.logn != kLogN + 3 || s.compiled_only || !s.small_delta || s.nm > 65535) return hipErrorNotSupported;
  if (batch == 0) return hipSuccess;
  if (batch > 0x7fffffffull) return hipErrorInvalidValue;
  hipFunction_t fn = asm_fn(out1 ? kAsmFused32kEnc2I8 : kAsmFused32kFmaFwdI8);
  if (!fn) return hipErrorNotSupported;
  struct {
    StdArgs std;
    const void *k0, *k1, *e1p;
    void *out1;
  } args = {{out0, x8, e0p, PSI_LM(t), t.mc, (int)s.nm, s.logn}, k0, out1 ? k1 : k0, out1 ? e1p : e0p, out1 ? out1 : out0};
  static_assert(sizeof(args) == 80, "kernarg layout of nflhip_fused_{fma_fwd,enc2_}32768i8_asm");
  return launch_packed(fn, (unsigned)batch, (unsigned)s.nm, 1024, &args, sizeof(args), st);
}

// n = 65536: one launch of the three-role kernel (tools/gen_polymul_asm.py build_pipe): fused block products of `cnt_v`
// polynomials whose operands already went through the forward streaming pass (a_v, b_v -> c_v), the forward streaming
// pass of `cnt_f` polynomials (fa_src -> fa_dst, fb_src -> fb_dst) and the inverse streaming pass of `cnt_i`
// polynomials in place (inv).  Counts may be zero.
hipError_t launch_polymul_pipe64k_u64(const Shape &s, const DevTables &t, uint64_t *c_v, const uint64_t *a_v,
                                      const uint64_t *b_v, int cnt_v, const uint64_t *fa_src, uint64_t *fa_dst,
                                      const uint64_t *fb_src, uint64_t *fb_dst, int cnt_f, uint64_t *inv, int cnt_i,
                                      hipStream_t st, bool b_is_ntt, int level) {
  if (s.limb_bits != 64 || s.logn != 16 || s.compiled_only || !s.small_delta || s.nm > 65535) return hipErrorNotSupported;
  // (coefficient loads / stores carry `nt`: they pass through the L2 once, the twiddle tables stay resident: measured +3 %)
  // b_is_ntt: b_v is the caller's transformed operand (canonical words), read block-wise as it lies; no forward role for it
  // level 2 (coefficient-form operands only): the block products run on incomplete transforms, and the streaming inverse role
  // folds in (n / 4)^-1 from the level-2 records -- every launch of one product takes the same level
  const bool inc = level == 2 && !b_is_ntt && t.mc_inc[1];
  hipFunction_t fn = asm_fn(b_is_ntt ? kAsmPipe64kB : inc ? kAsmPipe64kI2 : kAsmPipe64k);
  if (!fn) return hipErrorNotSupported;
  const int mx = cnt_v > cnt_f ? (cnt_v > cnt_i ? cnt_v : cnt_i) : (cnt_f > cnt_i ? cnt_f : cnt_i);
  if (mx <= 0) return hipSuccess;
  struct {
    StdArgs std;
    int cnt_v, cnt_f, cnt_i, remap_gx;
    const void *fa_src;
    void *fa_dst;
    const void *fb_src;
    void *fb_dst, *inv;
    unsigned remap_per, remap_magic;
  } args = {{c_v, a_v, b_v, t.psi, inc ? t.mc_inc[1] : t.mc, (int)s.nm, s.logn}, cnt_v, cnt_f, cnt_i, 0, fa_src, fa_dst, fb_src, fb_dst, inv, 0u, 0u};
  static_assert(sizeof(args) == 112, "kernarg layout of nflhip_polymul_pipe65536_asm");
  // per polynomial row: 16 block products + 3 x 4 streaming workgroups (2 x 4 when b needs no forward pass)
  const size_t gx = (size_t)mx * (b_is_ntt ? 24 : 28);
  if (gx > 0x7fffffffull) return hipErrorInvalidValue;
#ifndef NFLHIP_NO_PIPE_REMAP
  // modulus-major units in contiguous ranges per XCD slot (see build_pipe): every twiddle table is then fetched by ~1.3 of
  // the 8 private L2s instead of all 8.  Needs units divisible by 8 and the kernel's one-multiply division by gx exact.
  const unsigned long long units = (unsigned long long)gx * s.nm;
  if (units % 8 == 0 && units * gx < (1ull << 32)) {
    args.remap_gx = (int)gx;
    args.remap_per = (unsigned)(units / 8);
    args.remap_magic = (unsigned)((1ull << 32) / gx + 1);
  }
#endif
  return launch_packed(fn, (unsigned)gx, (unsigned)s.nm, kThreads, &args, sizeof(args), st);
}

// n = 65536 / 32768, whole batch in ONE launch of persistent workgroups (tools/gen_polymul_asm.py fused_header): the three
// roles of a row run on one XCD and hand the intermediates over through that XCD's L2.  `work` is device memory of at
// least xcd_plan_bytes(); it is (re)initialised here, on `st`.
static std::atomic<unsigned long long> g_xcd_launches{0};
extern "C" unsigned long long nflhip_debug_xcd_launches(void) { return g_xcd_launches.load(); }  // include/nflhip_debug.h
// test / profiling hook: a device buffer (32 domains x 65536 records x 16 bytes) into which every role of the NEXT one-launch
// products writes {ticket | kind << 28, t0 = workgroup free, t1 = inputs ready, t2 = done} (low words of s_memtime); nullptr = off
static std::atomic<void *> g_xcd_trace{nullptr};
extern "C" void nflhip_debug_xcd_trace(void *device_buffer) { g_xcd_trace.store(device_buffer); }
__global__ void k_xcd_reset(uint4 *ctl) {   // block 0: the header; block d + 1: record d at byte 4096 + 69632 d (2 KiB each)
  uint4 *p = blockIdx.x == 0 ? ctl : ctl + (4096 + (size_t)(blockIdx.x - 1) * 0x11000) / 16;
  p[threadIdx.x] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && (threadIdx.x == 8 || threadIdx.x == 9)) p[threadIdx.x] = make_uint4(~0u, ~0u, ~0u, ~0u);
  // (bytes 128 .. 159: one free mask of 32 scratch slots per XCD -- the pooled plan)
}
struct XcdPlan {
  int rlog, wgs, dlog;
  unsigned magic;
  size_t ctl_bytes, slot_bytes, total;
};
static bool xcd_plan(const Shape &s, size_t batch, XcdPlan *p) {
  if (s.limb_bits != 64 || (s.logn != 16 && s.logn != 15) || s.compiled_only || !s.small_delta || s.nm > 65535) return false;
  // the kernel derives a row's XCD from the hardware XCC id: it needs the whole 8-XCD device (no compute partition)
  static int cus[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  if (cus[dev] != 256) return false;
  const unsigned long long rows = (unsigned long long)batch * s.nm;
  if (batch < 2 || rows < 8 || rows > 0x0fffffffull) return false;  // every XCD serves rows xcd, xcd + 8, ...
  const bool pow2 = (batch & (batch - 1)) == 0;
  if (!pow2 && rows * batch >= (1ull << 32)) return false;  // the kernel divides row numbers by the batch with one multiply
  p->magic = (unsigned)(pow2 ? (1ull << 32) / batch : (1ull << 32) / batch + 1);
  p->rlog = 3;   // 2^rlog rows in flight per scheduling domain
  p->dlog = 2;   // 2^dlog scheduling domains per XCD (measured: 1 domain 13.8 k, 2: 23.7 k, 4: 26.1 k products/s at n = 65536)
  p->wgs = 768;  // persistent workgroups: three per CU
  if (rows < (8ull << p->dlog)) return false;
  p->ctl_bytes = 4096 + ((size_t)8 << p->dlog) * 0x11000;  // word 0: next row; one 256 B scheduler record per domain, 68 KiB apart, from byte 4096
  p->slot_bytes = (size_t)rows * (s.n * 8);                 // per operand: the scratch mirrors the batch (every row its own scratch rows)
  p->total = p->ctl_bytes + 2 * p->slot_bytes;
  return true;
}
size_t xcd_plan_bytes(const Shape &s, size_t batch) {
  XcdPlan p;
  return xcd_plan(s, batch, &p) ? p.total : 0;
}
hipError_t launch_polymul_xcd_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                                  size_t batch, void *work, hipStream_t st, int level) {
  XcdPlan p;
  if (!xcd_plan(s, batch, &p)) return hipErrorNotSupported;
  const bool inc = level == 2 && t.mc_inc[1];
  hipFunction_t fn = asm_fn(s.logn == 16 ? (inc ? kAsmXcd64kI2 : kAsmXcd64k) : (inc ? kAsmXcd32kI2 : kAsmXcd32k));
  if (!fn) return hipErrorNotSupported;
  // fresh counters: word block 0 (workgroups that joined, per XCD) and the first KiB of every domain's record
  hipLaunchKernelGGL(k_xcd_reset, dim3((8u << p.dlog) + 1), dim3(128), 0, st, (uint4 *)work);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  char *w = (char *)work;
  struct {
    StdArgs std;
    int rows, batch;
    unsigned magic;
    int d, rlog, jmax, spin, inv;
    void *scr_a, *scr_b, *ctl, *trace;
  } args = {{c, a, b, t.psi, inc ? t.mc_inc[1] : t.mc, (int)s.nm, s.logn}, (int)(batch * s.nm), (int)batch, p.magic, p.dlog, p.rlog, 0,
            1 << 22, 0, w + p.ctl_bytes, w + p.ctl_bytes + p.slot_bytes, w, g_xcd_trace.load()};
  static_assert(sizeof(args) == 112, "kernarg layout of nflhip_polymul_xcd*_asm");
  g_xcd_launches.fetch_add(1);
  return launch_packed(fn, (unsigned)p.wgs, 1, kThreads, &args, sizeof(args), st);
}

// ---- one row per wave (or two / four waves): n = 1024 / 2048 [/ 4096], 32- and 64-bit limbs -------------------------------
// (tools/gen_row1024_u32_asm.py, tools/asmgen/rows1k.py)  The two limb widths share every launcher; what they differ in:
struct RowLimb {
  int bits, max_logn;     // rows of 2^10 .. 2^max_logn words: the kinds below are indexed [logn - 10]
  bool small_delta;       // 64-bit limbs: delta-form arithmetic, every modulus needs delta < 2^32
  bool fwd_fma_level2;    // 32-bit limbs: the forward pipelines reduce x k + e (lazily reduced x, e) with the base multiplication's
                          // Barrett step -- they need and read the level-2 records
  AsmKind mul[3], mul_inc[3], fwd[3], inv[3], fms_inv[3], fma_inv[3];   // product on complete / incomplete transforms, ...
  AsmKind enc2[2][3], fma_fwd[2][3];                                    // [format]: words / int8 inputs
};
static const RowLimb kRow32 = {32, 12, false, true,
    {kAsmRow1024U32, kAsmRow2048U32, kAsmRow4096U32}, {kAsmRow1024I2U32, kAsmRow2048I2U32, kAsmRow4096I2U32},
    {kAsmRowFwd1024U32, kAsmRowFwd2048U32, kAsmRowFwd4096U32}, {kAsmRowInv1024U32, kAsmRowInv2048U32, kAsmRowInv4096U32},
    {kAsmRowFmsInv1024U32, kAsmRowFmsInv2048U32, kAsmRowFmsInv4096U32}, {kAsmRowFmaInv1024U32, kAsmRowFmaInv2048U32, kAsmRowFmaInv4096U32},
    {{kAsmRowEnc2W1024U32, kAsmRowEnc2W2048U32, kAsmRowEnc2W4096U32}, {kAsmRowEnc2I81024U32, kAsmRowEnc2I82048U32, kAsmRowEnc2I84096U32}},
    {{kAsmRowFmaFwdW1024U32, kAsmRowFmaFwdW2048U32, kAsmRowFmaFwdW4096U32}, {kAsmRowFmaFwdI81024U32, kAsmRowFmaFwdI82048U32, kAsmRowFmaFwdI84096U32}}};
static const RowLimb kRow64 = {64, 11, true, false,   // (no n = 4096 members: max_logn keeps the third slots unread)
    {kAsmRow1024L0U64, kAsmRow2048L0U64}, {kAsmRow1024U64, kAsmRow2048U64}, {kAsmRowFwd1024U64, kAsmRowFwd2048U64}, {kAsmRowInv1024U64, kAsmRowInv2048U64},
    {kAsmRowFmsInv1024U64, kAsmRowFmsInv2048U64}, {kAsmRowFmaInv1024U64, kAsmRowFmaInv2048U64},
    {{kAsmRowEnc2W1024U64, kAsmRowEnc2W2048U64}, {kAsmRowEnc2I81024U64, kAsmRowEnc2I82048U64}},
    {{kAsmRowFmaFwdW1024U64, kAsmRowFmaFwdW2048U64}, {kAsmRowFmaFwdI81024U64, kAsmRowFmaFwdI82048U64}}};
static inline bool row_shape(const RowLimb &w, const Shape &s) {
  return s.limb_bits == w.bits && s.logn >= 10 && s.logn <= w.max_logn && !s.compiled_only && (s.small_delta || !w.small_delta);
}
static inline unsigned row_magic(const Shape &s) { return s.nm == 1 ? 0u : (unsigned)((1ull << 32) / s.nm + 1); }  // row mod nm: one multiply in the kernel
static inline unsigned row_grid(unsigned long long rows, unsigned rpb) { return (unsigned)((rows + rpb - 1) / rpb); }   // rpb rows per 256-thread workgroup
// the product / transform kernels of every row length below 4096 take (dst, a, b, psi, mc, nm, magic, rows)
struct RowArgs {
  void *c;
  const void *a, *b, *psi, *mc;
  unsigned nm, magic;
  unsigned long long rows;
};
static_assert(sizeof(RowArgs) == 56, "kernarg layout of nflhip_row{8,1024,2048,4096}_u{32,64}_asm and nflhip_row128_u16_asm");
static hipError_t launch_rows(hipFunction_t fn, unsigned rpb, RowArgs args, hipStream_t st) {
  return launch_packed(fn, row_grid(args.rows, rpb), 1, 256, &args, sizeof(args), st);
}

// the fused product (on incomplete transforms unless nflhip_debug_polymul_level says 0) and the stand-alone transforms.
// mode: 0 fused product, 2 forward (canonical NTT-form words out), 3 inverse
static hipError_t launch_row1024(const RowLimb &w, const Shape &s, const DevTables &t, int mode, void *c, const void *a, const void *b,
                                 size_t batch, hipStream_t st) {
  if (!row_shape(w, s) || (mode != 0 && mode != 2 && mode != 3)) return hipErrorNotSupported;
  const unsigned long long rows = (unsigned long long)batch * s.nm;
  if (rows == 0) return hipSuccess;
  if (rows * s.nm >= (1ull << 32)) return hipErrorNotSupported;  // (row mod nm is one multiply in the kernel)
  const bool inc = mode == 0 && g_polymul_level.load() == 2 && t.mc_inc[1];   // coefficient form in and out: incomplete transforms
  hipFunction_t fn = asm_fn((mode == 0 ? (inc ? w.mul_inc : w.mul) : (mode == 2 ? w.fwd : w.inv))[s.logn - 10]);
  if (!fn) return hipErrorNotSupported;
  return launch_rows(fn, 4u >> (s.logn - 10), {c, a, b, t.psi, inc ? t.mc_inc[1] : t.mc, (unsigned)s.nm, row_magic(s), rows}, st);
}

// 32-bit limbs, n = 1024 / 2048 / 4096: one / two / four waves per row; hipErrorNotSupported: the compiled launch_row1024_u32
hipError_t launch_row1024_u32_asm(const Shape &s, const DevTables &t, int mode, uint32_t *c, const uint32_t *a,
                                  const uint32_t *b, size_t batch, hipStream_t st) {
  // mode (as launch_row1024_u32): 0 fused product, 1 product with b already transformed (n = 8 only), 2 forward
  // (canonical NTT-form words out), 3 inverse
  if (s.limb_bits == 32 && s.logn == 3 && mode >= 0 && mode <= 3 && !s.compiled_only) {
    // n = 8 (the reference's (8, 60, uint32_t) config): one LANE per row, 256 rows per workgroup (tools/gen_row8_u32_asm.py)
    const unsigned long long rows8 = (unsigned long long)batch * s.nm;
    if (rows8 == 0) return hipSuccess;
    if (rows8 * s.nm >= (1ull << 32)) return hipErrorNotSupported;
    static_assert(kAsmRowNtt8U32 == kAsmRow8U32 + 1 && kAsmRowFwd8U32 == kAsmRow8U32 + 2 && kAsmRowInv8U32 == kAsmRow8U32 + 3, "row-8 kernels in mode order");
    hipFunction_t f8 = asm_fn((AsmKind)(kAsmRow8U32 + mode));
    if (!f8) return hipErrorNotSupported;
    return launch_rows(f8, 256, {c, a, b, t.psi, t.mc, (unsigned)s.nm, row_magic(s), rows8}, st);
  }
  return launch_row1024(kRow32, s, t, mode, c, a, b, batch, st);
}
// 64-bit limbs, n = 1024 / 2048: one wave / two waves per row; hipErrorNotSupported: the compiled k_row<Pol64, ...>
hipError_t launch_row1024_u64_asm(const Shape &s, const DevTables &t, int mode, uint64_t *c, const uint64_t *a,
                                  const uint64_t *b, size_t batch, hipStream_t st) {
  return launch_row1024(kRow64, s, t, mode, c, a, b, batch, st);
}

// ... and the transform-fused pipelines on those rows (rows1k.py build_row1k_fwd_fma / build_row1k_fma_inv, gen_row1024_u32_asm.py
// build_fwd_fma / build_fma_inv): operands of format words or int8, strides 0 / 1; hipErrorNotSupported: the compiled k_row_fwd_fma /
// k_row_fma_inv (kernels_wave.hip)
static hipError_t launch_row_fwd_fma(const RowLimb &w, const Shape &s, const DevTables &t, int format, void *out0, void *out1, const void *x,
                                     unsigned xs, const void *k0, unsigned k0s, const void *e0, unsigned e0s, const void *k1, unsigned k1s,
                                     const void *e1, unsigned e1s, size_t batch, hipStream_t st) {
  if (g_fused_grid.load(std::memory_order_relaxed) == 4) return hipErrorNotSupported;   // (nflhip_debug_fused_grid: the compiled one-pass template instead)
  if (!row_shape(w, s) || (w.fwd_fma_level2 && !t.mc_inc[1]) || (format != 0 && format != 1)) return hipErrorNotSupported;
  if (xs > 1 || k0s > 1 || e0s > 1 || (out1 && (k1s > 1 || e1s > 1))) return hipErrorNotSupported;
  const unsigned long long rows = (unsigned long long)batch * s.nm;
  if (rows == 0) return hipSuccess;
  if (rows * s.nm >= (1ull << 32)) return hipErrorNotSupported;
  hipFunction_t fn = asm_fn((out1 ? w.enc2 : w.fma_fwd)[format][s.logn - 10]);
  if (!fn) return hipErrorNotSupported;
  struct {
    void *out0, *out1;
    const void *x, *psi, *mc;
    unsigned nm, magic;
    const void *k0, *e0, *k1, *e1;
    unsigned long long rows;
    unsigned xs, k0s, e0s, k1s, e1s, pad;
  } args = {out0, out1, x, t.psi, w.fwd_fma_level2 ? t.mc_inc[1] : t.mc, (unsigned)s.nm, row_magic(s), k0, e0, out1 ? k1 : k0, out1 ? e1 : e0,
            rows, xs, k0s, e0s, out1 ? k1s : 0u, out1 ? e1s : 0u, 0u};
  static_assert(sizeof(args) == 112, "kernarg layout of nflhip_row*_enc2*_u{32,64}_asm");
  return launch_packed(fn, row_grid(rows, 4u >> (s.logn - 10)), 1, 256, &args, sizeof(args), st);
}
hipError_t launch_row_fwd_fma_u64_asm(const Shape &s, const DevTables &t, int format, uint64_t *out0, uint64_t *out1, const void *x, unsigned xs,
                                      const uint64_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint64_t *k1, unsigned k1s,
                                      const void *e1, unsigned e1s, size_t batch, hipStream_t st) {
  return launch_row_fwd_fma(kRow64, s, t, format, out0, out1, x, xs, k0, k0s, e0, e0s, k1, k1s, e1, e1s, batch, st);
}
hipError_t launch_row_fwd_fma_u32_asm(const Shape &s, const DevTables &t, int format, uint32_t *out0, uint32_t *out1, const void *x, unsigned xs,
                                      const uint32_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint32_t *k1, unsigned k1s,
                                      const void *e1, unsigned e1s, size_t batch, hipStream_t st) {
  return launch_row_fwd_fma(kRow32, s, t, format, out0, out1, x, xs, k0, k0s, e0, e0s, k1, k1s, e1, e1s, batch, st);
}

static hipError_t launch_row_fma_inv(const RowLimb &w, const Shape &s, const DevTables &t, int subtract, void *c, const void *a, const void *key,
                                     int kstride, const void *b, size_t batch, hipStream_t st) {
  if (g_fused_grid.load(std::memory_order_relaxed) == 4) return hipErrorNotSupported;   // (nflhip_debug_fused_grid: the compiled one-pass template instead)
  if (!row_shape(w, s) || kstride < 0 || kstride > 1) return hipErrorNotSupported;
  const unsigned long long rows = (unsigned long long)batch * s.nm;
  if (rows == 0) return hipSuccess;
  if (rows * s.nm >= (1ull << 32)) return hipErrorNotSupported;
  hipFunction_t fn = asm_fn((subtract ? w.fms_inv : w.fma_inv)[s.logn - 10]);
  if (!fn) return hipErrorNotSupported;
  struct {
    RowArgs row;
    const void *key;
    unsigned kstride, pad;
  } args = {{c, a, b, t.psi, t.mc, (unsigned)s.nm, row_magic(s), rows}, key, (unsigned)kstride, 0u};
  static_assert(sizeof(args) == 72, "kernarg layout of nflhip_row*_fm?inv_u{32,64}_asm");
  return launch_packed(fn, row_grid(rows, 4u >> (s.logn - 10)), 1, 256, &args, sizeof(args), st);
}
hipError_t launch_row_fma_inv_u64_asm(const Shape &s, const DevTables &t, int subtract, uint64_t *c, const uint64_t *a, const uint64_t *key,
                                      int kstride, const uint64_t *b, size_t batch, hipStream_t st) {
  return launch_row_fma_inv(kRow64, s, t, subtract, c, a, key, kstride, b, batch, st);
}
hipError_t launch_row_fma_inv_u32_asm(const Shape &s, const DevTables &t, int subtract, uint32_t *c, const uint32_t *a, const uint32_t *key,
                                      int kstride, const uint32_t *b, size_t batch, hipStream_t st) {
  return launch_row_fma_inv(kRow32, s, t, subtract, c, a, key, kstride, b, batch, st);
}

// 16-bit limbs, n = 128 (the reference's (128, 14, uint16_t) config): the fused product, eight rows per wave
// (tools/gen_row128_u16_asm.py)
hipError_t launch_row128_u16_asm(const Shape &s, const DevTables &t, int mode, uint16_t *c, const uint16_t *a,
                                 const uint16_t *b, size_t batch, hipStream_t st) {
  // mode: 0 fused product, 1 product with b already transformed, 2 forward (canonical NTT-form words out), 3 inverse
  if (s.limb_bits != 16 || s.logn != 7 || s.compiled_only || (s.nm & (s.nm - 1)) != 0 || mode < 0 || mode > 3)
    return hipErrorNotSupported;
  const unsigned long long rows = (unsigned long long)batch * s.nm;
  if (rows == 0) return hipSuccess;
  if (rows > 0x7fffffffull) return hipErrorNotSupported;
  static_assert(kAsmRowNtt128U16 == kAsmRow128U16 + 1 && kAsmRowFwd128U16 == kAsmRow128U16 + 2 && kAsmRowInv128U16 == kAsmRow128U16 + 3, "row-128 kernels in mode order");
  hipFunction_t fn = asm_fn((AsmKind)(kAsmRow128U16 + mode));
  if (!fn) return hipErrorNotSupported;
  return launch_rows(fn, 32, {c, a, b, t.psi, t.mc, (unsigned)s.nm, 0u, rows}, st);   // (nm is a power of two: no magic)
}

// first-use warm-up (kernels_fast.hip warm_fast): the runtime loads a translation unit's code object at the first launch of ANY of its kernels
__global__ void k_warm_asm() {}
hipError_t warm_asm(hipStream_t st) {
  (void)asm_fn(kAsmPolymul);   // (hipModuleLoadData + the function table)
  hipLaunchKernelGGL(k_warm_asm, dim3(1), dim3(64), 0, st);
  return hipGetLastError();
}

}  // namespace nflhip
