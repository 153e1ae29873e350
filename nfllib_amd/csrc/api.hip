// api.hip -- the C ABI of include/nflhip.h: context + device-table provisioning
// and the device-pointer entry points (the host-pointer ones stage through them: api_host.hip).  No CPU compute path exists
// here: every operation is a launch of a gfx950 kernel (kernels_generic.hip / kernels_fast.hip).
#include "../../include/nflhip.h"
#include "../../include/nflhip_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "ctx.h"
#include "gauss_table.h"
#include "host_tables.h"
#include "kernels.h"

using namespace nflhip;

// errno-style: one message per calling thread, so concurrent callers of one context never race on it
static thread_local std::string g_last_error = "";

namespace nflhip {
int set_error(int code, const std::string &msg) {  // (ctx.h fail, comm.hip)
  g_last_error = msg;
  return code;
}
}  // namespace nflhip

// ---------------------------------------------------------------------------
// the context's device tables: host_tables.cpp computes them, this uploads and frees them
// ---------------------------------------------------------------------------
struct TableSlot {
  void **dev;
  const HostTables::Bytes *host;
};
// THE list of device tables: upload_tables and free_tables both walk it (h == nullptr: only the device side is read)
static std::array<TableSlot, 16> table_slots(DevTables &t, const HostTables *h) {
  static const HostTables none;
  if (!h) h = &none;
  return {{{&t.psi, &h->psi}, {&t.psi_lm, &h->psi_lm}, {&t.mc, &h->mc}, {&t.mc_inc[0], &h->mc_inc[0]}, {&t.mc_inc[1], &h->mc_inc[1]},
           {&t.resc, &h->resc}, {(void **)&t.qhat, &h->qhat}, {(void **)&t.qsh, &h->qsh}, {(void **)&t.qparts, &h->qparts},
           {(void **)&t.bparts, &h->bparts}, {(void **)&t.qhat_w, &h->qhat_w}, {(void **)&t.qsh_w, &h->qsh_w},
           {&t.crt_bfrag, &h->crt_bfrag}, {&t.crt_bproj, &h->crt_bproj}, {(void **)&t.crt_coff, &h->crt_coff},
           {(void **)&t.crt_c2048, &h->crt_c2048}}};
}

// an empty host table leaves its pointer null; a failure leaves every pointer null or owned (nflhip_ctx_destroy frees them)
static int upload_tables(nflhip_ctx *c, const HostTables &h) {
  for (const TableSlot &s : table_slots(c->tabs, &h)) {
    *s.dev = nullptr;
    if (s.host->empty()) continue;
    HIPCHK(nullptr, hipMalloc(s.dev, s.host->size()));
    HIPCHK(nullptr, hipMemcpy(*s.dev, s.host->data(), s.host->size(), hipMemcpyHostToDevice));
  }
  c->tabs.proj_K = h.proj_K;
  c->tabs.inv_qtop = h.inv_qtop;
  c->tabs.crt_Lw = h.crt_Lw;
  c->tabs.crt_nsh = h.crt_nsh;
  c->shape.crt_L = h.crt_L;
  c->shape.crt_Lacc = h.crt_Lacc;
  c->shape.crt_Q0 = h.crt_Q0;
  c->shape.small_delta = h.small_delta;
  c->shape.nm_small = h.nm_small;
  c->h_Q = h.Q;
  c->h_lifting = h.lifting;
  c->h_P = h.P;
  c->h_roots = h.roots;
  c->h_invk = h.invk;
  c->h_phi = h.phi;
  return NFLHIP_OK;
}

static void free_tables(nflhip_ctx *c) {
  for (const TableSlot &s : table_slots(c->tabs, nullptr)) {
    if (*s.dev) (void)hipFree(*s.dev);
    *s.dev = nullptr;
  }
}

// the comparison flags: pinned host memory the kernels store into and the caller reads once the stream has drained (device memory +
// a copy when the pinned allocation is refused); a hit stores the call's TOKEN, so nothing has to be cleared in front of a launch
static int alloc_cmp_flags(nflhip_ctx *c) {
  if (hipHostMalloc((void **)&c->tabs.flag, nflhip_ctx::kCmpSlots * sizeof(int), hipHostMallocDefault) == hipSuccess) {
    c->flag_host = true;
    std::memset(c->tabs.flag, 0, nflhip_ctx::kCmpSlots * sizeof(int));
  } else {
    (void)hipGetLastError();
    c->tabs.flag = nullptr;
    HIPCHK(nullptr, hipMalloc((void **)&c->tabs.flag, nflhip_ctx::kCmpSlots * sizeof(int)));
    HIPCHK(nullptr, hipMemset(c->tabs.flag, 0, nflhip_ctx::kCmpSlots * sizeof(int)));
  }
  return NFLHIP_OK;
}

// ---------------------------------------------------------------------------
// dispatch on the limb type: f(T()) for the context's T = uint16_t / uint32_t / uint64_t
// ---------------------------------------------------------------------------
template <typename F>
static auto with_limb(const nflhip_ctx *ctx, F f) {
  if (ctx->shape.limb_bits == 16) return f(uint16_t());
  if (ctx->shape.limb_bits == 32) return f(uint32_t());
  return f(uint64_t());
}

static int ensure_scratch(nflhip_ctx *ctx, size_t bytes) {
  if (ctx->scratch_bytes >= bytes) return NFLHIP_OK;
  if (ctx->scratch) HIPCHK(ctx, hipFree(ctx->scratch));
  ctx->scratch = nullptr;
  ctx->scratch_bytes = 0;
  HIPCHK(ctx, hipMalloc(&ctx->scratch, bytes));
  ctx->scratch_bytes = bytes;
  return NFLHIP_OK;
}

// chunks of a batch in the n = 65536 pipeline (fill + drain cost ~0.7 chunk; small grids lose efficiency: 4 measured best)
#ifndef NFLHIP_PIPE_CHUNKS
#define NFLHIP_PIPE_CHUNKS 4
#endif
static constexpr int kPipeChunks = NFLHIP_PIPE_CHUNKS;


// Rows of 65536 / 32768 words in ONE launch of persistent workgroups (asm_launch.hip launch_polymul_xcd_u64) instead
// of the chunked pipeline / the register-resident row kernels: by default for SMALL batches, where the other plans'
// fill and drain launches (n = 65536) or the one-workgroup-per-row grid (n = 32768) leave CUs idle.  Measured (MI355X):
// n = 65536 / 30 moduli +5 % at batch 4, +11 % at 8, +-0 at 16, -2 % at 64; n = 32768 / 2 moduli against the row
// kernels 68 vs 58 k products/s at batch 8, 302 vs 223 k at 32, 622 vs 716 k at 128.  Shape::plan (NFLHIP_XCD at context
// creation) forces either.
static bool xcd_on(const nflhip_ctx *ctx, size_t batch) {
  if (ctx->shape.plan >= 0) return ctx->shape.plan != 0;
  return batch * ctx->shape.nm <= (ctx->shape.logn == 15 ? 255u : 256u);
}

// hipGraph capture: the entry points only enqueue work on the caller's stream, so they can be captured.  The
// multi-launch plans additionally order successive calls on the shared scratch with events recorded OUTSIDE any
// capture; inside a capture those waits are illegal (and meaningless: a graph orders its own nodes), so they are
// skipped -- a graph that replays a multi-launch plan must not run concurrently with other work on the same context.
static bool is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs == hipStreamCaptureStatusActive;
}

// A context's workspaces (ctx.h Workspace), each under its owner's mutex.  ws_grow: the buffer holds `need` bytes afterwards, or the
// call is refused while capturing -- `what`: the caller and its article, "keyswitch: the".  ws_begin: that, and the stream waits for
// the call that used the workspace last; ws_end: the next call waits for this one.  A capturing call neither waits nor records.
static int ws_grow(nflhip_ctx *ctx, Workspace &w, size_t need, bool cap, const char *what) {
  if (w.bytes >= need) return NFLHIP_OK;
  if (cap) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, std::string(what) + " scratch has to grow, which a stream capture cannot do");
  if (w.buf) HIPCHK(ctx, hipFree(w.buf));  // (synchronises: nothing still reads it)
  w.buf = nullptr;
  w.bytes = 0;
  HIPCHK(ctx, hipMalloc(&w.buf, need));
  w.bytes = need;
  return NFLHIP_OK;
}
static int ws_begin(nflhip_ctx *ctx, Workspace &w, size_t need, bool cap, hipStream_t st, const char *what) {
  int rc = ws_grow(ctx, w, need, cap, what);
  if (rc) return rc;
  if (!w.ev) HIPCHK(ctx, hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  if (!cap && w.ev_valid) HIPCHK(ctx, hipStreamWaitEvent(st, w.ev, 0));  // a previous call on another stream
  return NFLHIP_OK;
}
static int ws_end(nflhip_ctx *ctx, Workspace &w, bool cap, hipStream_t st) {
  if (cap) return NFLHIP_OK;
  HIPCHK(ctx, hipEventRecord(w.ev, st));
  w.ev_valid = true;
  return NFLHIP_OK;
}
static void ws_free(Workspace &w) {
  if (w.ev) (void)hipEventDestroy(w.ev);
  if (w.buf) (void)hipFree(w.buf);
  w = Workspace();
}

// The warm maps (ctx.h WarmMap), each under its owner's mutex: a call while capturing may repeat what warm_covers finds -- an entry
// for its key with every size at least the call's -- and a call outside a capture raises the entry to its sizes afterwards (an
// entry that cannot be stored only costs a later capture its refusal).
static bool warm_covers(const WarmMap &m, const std::array<size_t, 3> &key, const std::array<size_t, 3> &sizes) {
  const auto it = m.find(key);
  return it != m.end() && it->second[0] >= sizes[0] && it->second[1] >= sizes[1] && it->second[2] >= sizes[2];
}
static void warm_note(WarmMap &m, const std::array<size_t, 3> &key, const std::array<size_t, 3> &sizes) {
  try {
    std::array<size_t, 3> &w = m[key];  // (a new entry is zeros)
    for (int i = 0; i < 3; ++i) w[i] = std::max(w[i], sizes[i]);
  } catch (const std::bad_alloc &) {
  }
}

// composed path: NTT(a)->c, NTT(b)->scratch, inverse with the product fused into its load
template <typename T>
static int polymul_composed(nflhip_ctx *ctx, T *c, const T *a, const T *b, int b_is_ntt, size_t batch, hipStream_t st) {
  hipError_t e;
  const T *bn = b;
  std::unique_lock<std::mutex> lk(ctx->scratch_mu, std::defer_lock);
  T *acopy = nullptr;
  // c may alias a or b: transform a into c first only when that does not clobber b
  const size_t bytes = poly_bytes(ctx, batch);
  lk.lock();
  const bool cap = is_capturing(st);
  // (from 256 rows on; below that the one-launch plan further down spreads a row over more CUs -- measured, same box:
  // batch 8 / 32 / 128 / 512 of two moduli 58 / 223 / 716 / 785 k products/s here against 68 / 302 / 622 / 779 k)
  if (sizeof(T) == 8 && !b_is_ntt && ctx->shape.logn == 15 && !(xcd_on(ctx, batch) && xcd_plan_bytes(ctx->shape, batch) != 0)) {
    // rows of 32768 words: b' = NTT(b) into the scratch (one read, one write), then c = INTT(NTT(a) (.) b') with the row
    // of a register-resident and b' streamed through the point-wise step (two reads, one write): 5 operand passes
    int rcs = ensure_scratch(ctx, bytes);
    if (rcs) return rcs;
    if (!cap && ctx->ev_scratch_valid) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));
    if (!cap && ctx->ev_prev_valid)
      for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[k], 0));
    // (the level is read ONCE per product: both launches must agree on what b' is)
    const int pair = polymul_level() == 2 && ctx->tabs.mc_inc[1] ? 6 : 4;
    e = launch_row32k_u64(ctx->shape, ctx->tabs, pair, (uint64_t *)ctx->scratch, (const uint64_t *)b, nullptr, batch, st);
    if (e == hipSuccess)
      e = launch_row32k_u64(ctx->shape, ctx->tabs, pair + 1, (uint64_t *)c, (const uint64_t *)a, (const uint64_t *)ctx->scratch, batch, st);
    if (e == hipSuccess) {
      if (!cap) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_scratch, st));
        ctx->ev_scratch_valid = true;
        for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[k], ctx->ev_scratch, 0));
      }
      return NFLHIP_OK;
    }
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "polymul: 32768-word row kernels");
  }
  if (sizeof(T) == 8 && !b_is_ntt && xcd_on(ctx, batch)) {
    // rows of 65536 / 32768 words: ONE launch of persistent workgroups, every row's three roles on one XCD and the
    // intermediates through that XCD's L2 (asm_launch.hip launch_polymul_xcd_u64); needs only a ring of row slots
    const size_t need = xcd_plan_bytes(ctx->shape, batch);
    if (need) {
      int rcx = ensure_scratch(ctx, need);
      if (rcx) return rcx;
      if (!cap && ctx->ev_scratch_valid) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));
      if (!cap && ctx->ev_prev_valid)
        for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[k], 0));
      e = launch_polymul_xcd_u64(ctx->shape, ctx->tabs, (uint64_t *)c, (const uint64_t *)a, (const uint64_t *)b, batch,
                                 ctx->scratch, st, polymul_level());
      if (e == hipSuccess) {
        if (!cap) {
          HIPCHK(ctx, hipEventRecord(ctx->ev_scratch, st));
          ctx->ev_scratch_valid = true;
          for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[k], ctx->ev_scratch, 0));
        }
        return NFLHIP_OK;
      }
      if (e != hipErrorNotSupported) return hipfail(ctx, e, "polymul: one-launch kernel");
    }
  }
  int rc = ensure_scratch(ctx, 2 * bytes);
  if (rc) return rc;
  T *s0 = (T *)ctx->scratch, *s1 = (T *)((char *)ctx->scratch + bytes);
  (void)acopy;
  if (sizeof(T) == 8 && ctx->shape.logn == 16) {
    // n = 65536: the streaming passes (HBM-bound) and the fused block kernel (VALU-bound) of neighbouring chunks share
    // every CU inside ONE kernel whose workgroups take three roles; consecutive launches on the caller's stream form the
    // pipeline: launch L = forward pass of chunk L, block products of chunk L-1, inverse pass of chunk L-2.
    const size_t pw = ctx->shape.nm * ctx->shape.n;
    size_t nchunk = (size_t)kPipeChunks;
    size_t edge = 0;   // polynomials in the first and in the last chunk when they are shorter than the others (experiment knob only)
#ifdef NFLHIP_ABLATION_KNOBS   // experiment builds only (tools/sessions/gpu_round5_a.sh, gpu_round6_g.sh): chunk count / edge chunks at run time, chunk aliasing
#include "ablation_knobs.inc"
#endif
    if (nchunk * 2 > batch) nchunk = batch >= 2 ? batch / 2 : 1;
    // chunk boundaries: uniform.  (Round 6 tried SHORT first / last chunks -- the first launch runs the forward role alone and the last
    // the inverse role alone, the pipeline's fill and drain -- through the experiment knob below: nothing beyond noise at batch 128,
    // +0.8 % for eight chunks at batch 256: profiles/r06_E_edge_chunks.txt.)
    if (nchunk < 3 || 2 * edge + (nchunk - 2) > batch) edge = 0;
    auto lo_of = [&](size_t ch) -> size_t {
      if (!edge) return batch * ch / nchunk;
      if (ch == 0) return 0;
      if (ch >= nchunk) return batch;
      return edge + (batch - 2 * edge) * (ch - 1) / (nchunk - 2);
    };
#ifdef NFLHIP_ABLATION_KNOBS   // ... and every chunk laid over chunk 0's memory (WRONG results by construction: the roles of
    // neighbouring launches then share one window of a, b, c and the scratch that fits the 256 MiB Infinity Cache -- what
    // the plan would run at if none of its passes reached HBM)
    auto at_of = [&](size_t ch) { return alias_chunks ? (size_t)0 : lo_of(ch); };
#else
    auto at_of = lo_of;
#endif
    bool supported = true;
    const int level = b_is_ntt ? 0 : polymul_level();   // read once: the three roles of a chunk run in different launches
    if (!cap && ctx->ev_scratch_valid) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));  // a previous call on another stream
    if (!cap && ctx->ev_prev_valid)  // ... or a helper-stream plan (polymul_ntt_dev at this shape) still reading s0
      for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[k], 0));
    for (size_t L = 0; L < nchunk + 2 && supported; ++L) {
      const bool hf = L < nchunk, hv = L >= 1 && L - 1 < nchunk, hi = L >= 2 && L - 2 < nchunk;
      const size_t f0 = hf ? at_of(L) : 0, v0 = hv ? at_of(L - 1) : 0, i0 = hi ? at_of(L - 2) : 0;
      const int cf = hf ? (int)(lo_of(L + 1) - lo_of(L)) : 0, cv = hv ? (int)(lo_of(L) - lo_of(L - 1)) : 0, ci = hi ? (int)(lo_of(L - 1) - lo_of(L - 2)) : 0;
      // (b already transformed: its blocks are read from the caller's array by the block products, no forward pass, no scratch)
      e = launch_polymul_pipe64k_u64(ctx->shape, ctx->tabs, (uint64_t *)c + v0 * pw, (const uint64_t *)s0 + v0 * pw,
                                     (b_is_ntt ? (const uint64_t *)b : (const uint64_t *)s1) + v0 * pw, cv, (const uint64_t *)a + f0 * pw,
                                     (uint64_t *)s0 + f0 * pw, b_is_ntt ? nullptr : (const uint64_t *)b + f0 * pw,
                                     b_is_ntt ? nullptr : (uint64_t *)s1 + f0 * pw, cf, (uint64_t *)c + i0 * pw, ci, st, b_is_ntt != 0, level);
      if (e == hipErrorNotSupported && L == 0) { supported = false; break; }
      if (e != hipSuccess) return hipfail(ctx, e, "polymul: pipeline kernel");
    }
    if (supported) {
      if (!cap) {  // the scratch is reused by the next call on any stream: order it after this one
        HIPCHK(ctx, hipEventRecord(ctx->ev_scratch, st));
        ctx->ev_scratch_valid = true;
        for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[k], ctx->ev_scratch, 0));
      }
      return NFLHIP_OK;
    }
  }
  if (sizeof(T) == 8 && ctx->shape.logn > 12 && ctx->aux[0]) {
    // large rows: streaming outer passes, then the fused assembly kernel over the 4096-word blocks,
    // then the outer inverse passes (9 operand streams of HBM traffic instead of 13; 7 when b is already transformed:
    // its 4096-word blocks are exactly what the fused kernel would have computed for it).  The batch is cut
    // into chunks that alternate between two helper streams: one chunk's HBM-bound streaming passes
    // overlap another chunk's VALU-bound fused kernel.  Fully asynchronous w.r.t. the host.
    const size_t nm = ctx->shape.nm, pw = nm * ctx->shape.n;  // words per poly
    const size_t nchunk = batch >= 8 ? 8 : batch;
    HIPCHK(ctx, hipEventRecord(ctx->ev_start, st));
    for (int k = 0; k < 2; ++k) {
      HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[k], ctx->ev_start, 0));
      if (!cap && ctx->ev_prev_valid) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[k], ctx->ev_done[1 - k], 0));  // previous call's scratch use
    }
    bool unsupported = false;
    const int logi = 12;  // words (log2) per block of the fused kernel
    for (size_t ch = 0; ch < nchunk && !unsupported; ++ch) {
      const size_t lo = batch * ch / nchunk, hi = batch * (ch + 1) / nchunk, cnt = hi - lo;
      if (cnt == 0) continue;
      hipStream_t s = ctx->aux[ch & 1];
      const uint64_t *ak = (const uint64_t *)a + lo * pw, *bk = (const uint64_t *)b + lo * pw;
      uint64_t *ck = (uint64_t *)c + lo * pw, *s0k = (uint64_t *)s0 + lo * pw, *s1k = (uint64_t *)s1 + lo * pw;
      e = launch_outer_fwd_u64(ctx->shape, ctx->tabs, ak, s0k, cnt * nm, s, logi);
      if (e == hipSuccess && !b_is_ntt) e = launch_outer_fwd_u64(ctx->shape, ctx->tabs, bk, s1k, cnt * nm, s, logi);
      if (e != hipSuccess) return hipfail(ctx, e, "polymul: outer forward");
      const uint64_t *bblk = b_is_ntt ? bk : s1k;
      e = launch_polymul_blocks_asm_u64(ctx->shape, ctx->tabs, ck, s0k, bblk, cnt, s, b_is_ntt != 0);
      if (e == hipErrorNotSupported) { unsupported = true; break; }
      if (e != hipSuccess) return hipfail(ctx, e, "polymul: fused blocks");
      e = launch_outer_inv_u64(ctx->shape, ctx->tabs, ck, cnt * nm, s, logi);
      if (e != hipSuccess) return hipfail(ctx, e, "polymul: outer inverse");
    }
    for (int k = 0; k < 2; ++k) {
      HIPCHK(ctx, hipEventRecord(ctx->ev_done[k], ctx->aux[k]));
      HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[k], 0));
    }
    if (!cap) ctx->ev_prev_valid = true;  // (inside a capture the helper streams forked from and joined back into st)
    if (!unsupported) return NFLHIP_OK;
    // (assembly kernel unavailable: fall through to the composed plan, ordered after the helper streams)
  }
  // an earlier asynchronous plan (issued on any stream) may still be using the scratch
  if (!cap && ctx->ev_scratch_valid) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));
  if (!cap && ctx->ev_prev_valid)
    for (int k = 0; k < 2; ++k) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[k], 0));
  e = launch_ntt_fwd<T>(ctx->shape, ctx->tabs, a, s0, batch, st);
  if (e != hipSuccess) return hipfail(ctx, e, "polymul: ntt(a)");
  if (!b_is_ntt) {
    e = launch_ntt_fwd<T>(ctx->shape, ctx->tabs, b, s1, batch, st);
    if (e != hipSuccess) return hipfail(ctx, e, "polymul: ntt(b)");
    bn = s1;
  }
  e = launch_ntt_inv<T>(ctx->shape, ctx->tabs, s0, bn, c, batch, st);
  if (e != hipSuccess) return hipfail(ctx, e, "polymul: intt");
  // the scratch is reused by the next call on any stream: make that safe
  if (!cap) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hipfail(ctx, e, "polymul: sync");
  }
  return NFLHIP_OK;
}

// A comparison that ends in one flag: launch(z, flag, token) -- z the limb type's zero -- on a result slot of its own, then the
// flag read back.  A hit stores the call's token, 1, 2, ... per slot: never the value the flag holds from an earlier call.
template <typename F>
static int flag_call(nflhip_ctx *ctx, hipStream_t st, const char *where, int *hit, F launch) {
  const unsigned slot = ctx->cmp_next.fetch_add(1, std::memory_order_relaxed) % nflhip_ctx::kCmpSlots;
  std::lock_guard<std::mutex> lk(ctx->cmp_mu[slot]);  // held until the readback below has completed
  int *dflag = ctx->tabs.flag + slot, &last = ctx->cmp_token[slot];
  if (last == 0x7fffffff) {   // wrap: clear the flag once, start over
    last = 0;
    if (ctx->flag_host) *dflag = 0;
    else (void)hipMemsetAsync(dflag, 0, sizeof(int), st);
  }
  const int token = ++last;
  hipError_t e = with_limb(ctx, [&](auto z) { return launch(z, dflag, token); });
  if (e != hipSuccess) return hipfail(ctx, e, where);
  int flag = 0;
  if (!ctx->flag_host) HIPCHK(ctx, hipMemcpyAsync(&flag, ctx->tabs.flag + slot, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (ctx->flag_host) flag = *(volatile int *)dflag;
  *hit = flag == token ? 1 : 0;
  return NFLHIP_OK;
}

extern "C" {

int nflhip_abi_version(void) { return NFLHIP_ABI_VERSION; }

// include/nflhip_debug.h: test hooks, not part of the product boundary
void nflhip_debug_gauss_tie_shift(int shift) { set_gauss_tie_shift(shift); }

const char *nflhip_last_error(const nflhip_ctx *ctx) {
  (void)ctx;
  return g_last_error.c_str();
}

int nflhip_device_count(int *count) {
  if (!count) return fail(nullptr, NFLHIP_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return hipfail(nullptr, e, "hipGetDeviceCount");
  }
  *count = n;
  return NFLHIP_OK;
}

// First-use costs paid ONCE per device when its first context is created instead of inside whichever call comes first (measured,
// profiles/r06_first_use.txt: the first element-wise call 3.2 ms, the first transform 5.4 - 6.6 ms, the first CRT call 1.3 ms against
// 35 - 60 us afterwards -- the runtime loads a translation unit's code object at the first launch of any of its kernels, the generated
// kernels' module at its first use): one empty launch per translation unit, the module, and -- per context -- the three device staging
// buffers of the host-pointer entry points at one polynomial's size: + 20 ms on the first context of a process, nothing afterwards.
static int warm_up_device(nflhip_ctx *c) {
  static std::once_flag once[16];
  if (c->device >= 0 && c->device < 16) {
    hipError_t e = hipSuccess;
    std::call_once(once[c->device], [&] {
      hipStream_t st = c->hstream;
      hipError_t (*const tus[])(hipStream_t) = {nflhip::warm_generic, nflhip::warm_fast, nflhip::warm_crt, nflhip::warm_crt_mfma,
                                                nflhip::warm_sample, nflhip::warm_wave, nflhip::warm_automorph, nflhip::warm_rescale, nflhip::warm_dot, nflhip::warm_decompose, nflhip::warm_baseconv, nflhip::warm_baseconv_ntt, nflhip::warm_keyswitch, nflhip::warm_dot_multi, nflhip::warm_rotate, nflhip::warm_lintrans, nflhip::warm_mulrelin, nflhip::warm_scale_round, nflhip::warm_tensor_dot};
      for (auto f : tus)
        if (e == hipSuccess) e = f(st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    });
    if (e != hipSuccess) return hipfail(nullptr, e, "first-use warm-up");
  }
  for (int slot = 0; slot < 3; ++slot) {
    int rc = ensure_stage(c, slot, c->shape.n * c->shape.nm * c->word);
    if (rc) return rc;
  }
  return NFLHIP_OK;
}

// `parent`: a child context takes the parent's configuration instead of reading the environment again
static int ctx_create_mode(nflhip_ctx **out, int device, int limb_bits, size_t degree, size_t nmoduli, const void *P,
                           const void *primitive_roots, const void *invkmax, int kmax_log2, int cyclic,
                           const nflhip_ctx *parent = nullptr) {
  if (!out) return fail(nullptr, NFLHIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (limb_bits != 16 && limb_bits != 32 && limb_bits != 64)
    return fail(nullptr, NFLHIP_ERR_INVALID, "limb_bits must be 16, 32 or 64");
  if (!P || !primitive_roots || !invkmax) return fail(nullptr, NFLHIP_ERR_INVALID, "NULL parameter table");
  if (degree == 0 || (degree & (degree - 1)) != 0) return fail(nullptr, NFLHIP_ERR_INVALID, "degree must be a power of two");
  if (kmax_log2 < 1 || kmax_log2 > 30 || degree > (((size_t)1) << kmax_log2))
    return fail(nullptr, NFLHIP_ERR_INVALID, "degree exceeds kMaxPolyDegree (core.hpp:59-60)");
  if (degree < 4) return fail(nullptr, NFLHIP_ERR_UNSUPPORTED, "degree < 4 is not supported by the device engine");
  if (nmoduli == 0 || nmoduli > 1024) return fail(nullptr, NFLHIP_ERR_INVALID, "nmoduli out of range");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, NFLHIP_ERR_NO_DEVICE, "no HIP device available (this engine has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, NFLHIP_ERR_INVALID, "device index out of range");
  HIPCHK(nullptr, hipSetDevice(device));
  nflhip_ctx *c = new (std::nothrow) nflhip_ctx();
  if (!c) return fail(nullptr, NFLHIP_ERR_NOMEM, "out of host memory");
  c->device = device;
  c->cyclic = cyclic;
  c->word = (size_t)limb_bits / 8;
  c->shape.limb_bits = limb_bits;
  c->shape.n = degree;
  c->shape.nm = nmoduli;
  c->kmax_log2 = kmax_log2;
  // the environment is read HERE, once per context (include/nflhip.h "environment")
  if (parent) {
    c->shape.compiled_only = parent->shape.compiled_only;
    c->shape.plan = parent->shape.plan;
  } else {
    const char *v = getenv("NFLHIP_VARIANT");
    c->shape.compiled_only = v && (!strcmp(v, "hipcc") || !strcmp(v, "compiled")) ? 1 : 0;
    const char *x = getenv("NFLHIP_XCD");
    c->shape.plan = x && *x ? (atoi(x) != 0 ? 1 : 0) : -1;
  }
  c->shape.logn = 0;
  while ((((size_t)1) << c->shape.logn) < degree) c->shape.logn++;
  int rc;
  try {  // (host containers: no exception may cross the C boundary)
    HostTables h;
    std::string err;
    rc = build_host_tables(limb_bits, degree, nmoduli, cyclic, kmax_log2, P, primitive_roots, invkmax, &h, &err);
    rc = rc != NFLHIP_OK ? fail(nullptr, rc, err) : upload_tables(c, h);
  } catch (const std::bad_alloc &) {
    rc = fail(nullptr, NFLHIP_ERR_NOMEM, "out of host memory while building the tables");
  } catch (const std::exception &ex) {
    rc = fail(nullptr, NFLHIP_ERR_INVALID, std::string("table construction failed: ") + ex.what());
  }
  if (rc == NFLHIP_OK) rc = alloc_cmp_flags(c);
  if (rc == NFLHIP_OK) {
    hipError_t se = hipStreamCreateWithFlags(&c->hstream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && se == hipSuccess; ++k) {
      se = hipStreamCreateWithFlags(&c->aux[k], hipStreamNonBlocking);
      if (se == hipSuccess) se = hipEventCreateWithFlags(&c->ev_done[k], hipEventDisableTiming);
    }
    if (se == hipSuccess) se = hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming);
    if (se == hipSuccess) se = hipEventCreateWithFlags(&c->ev_scratch, hipEventDisableTiming);
    if (se != hipSuccess) rc = hipfail(nullptr, se, "hipStreamCreate");
  }
  if (rc == NFLHIP_OK) rc = warm_up_device(c);
  if (rc != NFLHIP_OK) {
    nflhip_ctx_destroy(c);
    return rc;
  }
  *out = c;
  return NFLHIP_OK;
}

int nflhip_ctx_create(nflhip_ctx **out, int device, int limb_bits, size_t degree, size_t nmoduli, const void *P,
                      const void *primitive_roots, const void *invkmax, int kmax_log2) {
  return ctx_create_mode(out, device, limb_bits, degree, nmoduli, P, primitive_roots, invkmax, kmax_log2, 0);
}

int nflhip_ctx_destroy(nflhip_ctx *ctx) {
  if (!ctx) return NFLHIP_OK;
  for (nflhip_ctx *child : ctx->row_ctx) nflhip_ctx_destroy(child);
  ctx->row_ctx.clear();
  nflhip_ctx_destroy(ctx->resc_last);
  nflhip_ctx_destroy(ctx->resc_kept);
  ctx->resc_last = ctx->resc_kept = nullptr;
  for (auto &kv : ctx->bcn_child) nflhip_ctx_destroy(kv.second);
  ctx->bcn_child.clear();
  for (auto &kv : ctx->lvl_child) nflhip_ctx_destroy(kv.second);
  ctx->lvl_child.clear();
  (void)hipSetDevice(ctx->device);
  // (the buffers go in the order they always went: where a LATER context's scratch lands follows the order of these frees, and a
  // table measured with another order moved by up to 2 % at its largest scratch -- profiles/r19_keyswitch_host.txt)
  for (Workspace *w : {&ctx->resc_ws, &ctx->bcn_ws[0], &ctx->bcn_ws[1]}) ws_free(*w);
  for (auto &kv : ctx->bconv) (void)hipFree(kv.second);
  ctx->bconv.clear();
  for (Workspace *w : {&ctx->rot_ws, &ctx->lt_ws, &ctx->bsgs_ws, &ctx->mr_ws}) ws_free(*w);
  for (auto &kv : ctx->mr_pi) (void)hipFree(kv.second);
  ctx->mr_pi.clear();
  ws_free(ctx->ks_ws);
  for (auto &kv : ctx->ks_recs) (void)hipFree(kv.second);
  ctx->ks_recs.clear();
  for (Workspace *w : {&ctx->sr_ws[0], &ctx->sr_ws[1], &ctx->bfv_ws}) ws_free(*w);
  for (auto &kv : ctx->srec) (void)hipFree(kv.second);
  ctx->srec.clear();
  if (ctx->hstream) (void)hipStreamDestroy(ctx->hstream);
  for (int k = 0; k < 2; ++k) {
    if (ctx->aux[k]) { (void)hipStreamSynchronize(ctx->aux[k]); (void)hipStreamDestroy(ctx->aux[k]); }
    if (ctx->ev_done[k]) (void)hipEventDestroy(ctx->ev_done[k]);
  }
  if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
  if (ctx->ev_scratch) (void)hipEventDestroy(ctx->ev_scratch);
  pipe_destroy(ctx);
  for (int i = 0; i < 4; ++i) free_stage(ctx, i);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  free_tables(ctx);
  if (ctx->tabs.flag) (void)(ctx->flag_host ? hipHostFree(ctx->tabs.flag) : hipFree(ctx->tabs.flag));
  delete ctx;
  return NFLHIP_OK;
}

// A child context over `count` rows of this one -- row i of the child is row phys(i) here, in order -- with the tables mode
// `cyclic`; never while capturing (`refusal`: the caller's message).  The child takes this context's configuration; a cyclic row
// child reads the environment itself.  bcn_child, level_child, rescale_children and row_child keep what this creates.
extern "C++" {
template <typename Phys>
static int child_create(nflhip_ctx *ctx, size_t count, Phys phys, int cyclic, bool cap, const char *refusal, nflhip_ctx **out) {
  if (cap) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, refusal);
  try {
    return with_limb(ctx, [&](auto z) {  // the parameter tables in the limb type's own width
      typedef decltype(z) T;
      std::vector<T> P(count), roots(count), invk(count);
      for (size_t i = 0; i < count; ++i) {
        const size_t j = phys(i);
        P[i] = (T)ctx->h_P[j];
        roots[i] = (T)ctx->h_roots[j];
        invk[i] = (T)ctx->h_invk[j];
      }
      return ctx_create_mode(out, ctx->device, ctx->shape.limb_bits, ctx->shape.n, count, P.data(), roots.data(), invk.data(), ctx->kmax_log2,
                             cyclic, cyclic ? nullptr : ctx);
    });
  } catch (const std::bad_alloc &) {
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  }
}
// ... kept in a map under `key`: looked up, or created and entered
template <typename Phys>
static int child_in_map(nflhip_ctx *ctx, ChildMap &m, const std::array<size_t, 2> &key, size_t count, Phys phys, bool cap, const char *refusal,
                        nflhip_ctx **out) {
  const auto it = m.find(key);
  if (it != m.end()) {
    *out = it->second;
    return NFLHIP_OK;
  }
  nflhip_ctx *child = nullptr;
  int rc = child_create(ctx, count, phys, 0, cap, refusal, &child);
  if (rc) return rc;
  try {
    m[key] = child;
  } catch (const std::bad_alloc &) {
    nflhip_ctx_destroy(child);
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  }
  *out = child;
  return NFLHIP_OK;
}
}  // extern "C++"

int nflhip_ctx_device(const nflhip_ctx *ctx) { return ctx ? ctx->device : -1; }
size_t nflhip_degree(const nflhip_ctx *ctx) { return ctx ? ctx->shape.n : 0; }
size_t nflhip_nmoduli(const nflhip_ctx *ctx) { return ctx ? ctx->shape.nm : 0; }
int nflhip_limb_bits(const nflhip_ctx *ctx) { return ctx ? ctx->shape.limb_bits : 0; }
size_t nflhip_crt_limbs(const nflhip_ctx *ctx) { return ctx ? ctx->shape.crt_L : 0; }

int nflhip_get_table(const nflhip_ctx *ctx, int which, size_t cm, void *host_out, size_t host_bytes) {
  if (!ctx || !host_out) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (cm >= ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "modulus index out of range");
  const size_t w = ctx->word;
  int rc = which >= NFLHIP_TAB_PHIS ? NFLHIP_OK : set_device(ctx);
  if (rc) return rc;
  const size_t mcsz = sizeof(ModConst<uint64_t>) / 8 * w;  // sizeof(ModConst<T>)
  switch (which) {
    case NFLHIP_TAB_PSI: {
      const size_t bytes = ctx->shape.n * 2 * w;
      if (host_bytes < bytes) return fail(ctx, NFLHIP_ERR_INVALID, "output buffer too small");
      HIPCHK(ctx, hipMemcpy(host_out, (const char *)ctx->tabs.psi + cm * bytes, bytes, hipMemcpyDeviceToHost));
      return NFLHIP_OK;
    }
    case NFLHIP_TAB_MODULUS:
    case NFLHIP_TAB_INVDEGREE: {
      if (host_bytes < w) return fail(ctx, NFLHIP_ERR_INVALID, "output buffer too small");
      const size_t off = cm * mcsz + (which == NFLHIP_TAB_MODULUS ? 0 : 3 * w);
      HIPCHK(ctx, hipMemcpy(host_out, (const char *)ctx->tabs.mc + off, w, hipMemcpyDeviceToHost));
      return NFLHIP_OK;
    }
    case NFLHIP_TAB_PHIS:
    case NFLHIP_TAB_SHOUPPHIS:
    case NFLHIP_TAB_INVPOLY_INVPHIS:
    case NFLHIP_TAB_SHOUPINVPOLY_INVPHIS:
    case NFLHIP_TAB_OMEGAS:
    case NFLHIP_TAB_INVOMEGAS: {
      const size_t n = ctx->shape.n, words = (which == NFLHIP_TAB_OMEGAS || which == NFLHIP_TAB_INVOMEGAS) ? 2 * n : n;
      if (host_bytes < words * w) return fail(ctx, NFLHIP_ERR_INVALID, "output buffer too small");
      const std::vector<uint64_t> v = reference_table(ctx->h_P[cm], ctx->h_phi[cm], ctx->h_invk[cm], ctx->kmax_log2, n, ctx->shape.limb_bits, which);
      for (size_t i = 0; i < words; ++i) {
        if (w == 8) ((uint64_t *)host_out)[i] = v[i];
        else if (w == 4) ((uint32_t *)host_out)[i] = (uint32_t)v[i];
        else ((uint16_t *)host_out)[i] = (uint16_t)v[i];
      }
      return NFLHIP_OK;
    }
    default: return fail(ctx, NFLHIP_ERR_INVALID, "unknown table id");
  }
}

int nflhip_get_crt_constant(const nflhip_ctx *ctx, int what, size_t cm, uint64_t *host_out, size_t cap, size_t *nlimbs) {
  if (!ctx || !host_out || !nlimbs) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  const std::vector<uint64_t> *src = nullptr;
  if (what == 0) src = &ctx->h_Q;
  else if (what == 1 && cm < ctx->shape.nm) src = &ctx->h_lifting[cm];
  else return fail(ctx, NFLHIP_ERR_INVALID, "unknown CRT constant");
  size_t n = src->size();
  while (n > 0 && (*src)[n - 1] == 0) --n;
  *nlimbs = n;
  if (cap < n) return fail(ctx, NFLHIP_ERR_INVALID, "output buffer too small");
  memset(host_out, 0, cap * sizeof(uint64_t));
  memcpy(host_out, src->data(), n * sizeof(uint64_t));
  return NFLHIP_OK;
}

// ---------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------
// The generated fast kernels of a row family -- for 64-bit limbs the fast plans, then the 1024 / 2048-word rows; the rows of
// 32-bit and of 16-bit limbs -- in mode 0: c = a b, 1: c = a b with b in NTT form, 2: c = NTT(a), 3: c = INTT(a).
// NFLHIP_ERR_UNSUPPORTED: none serves the shape, the caller takes the generic path.
static int fast_family(nflhip_ctx *ctx, int mode, void *c, const void *a, const void *b, size_t batch, hipStream_t st) {
  const Shape &s = ctx->shape;
  const DevTables &t = ctx->tabs;
  hipError_t e;
  if (s.limb_bits == 64) {
    e = mode == 2 ? launch_ntt_fwd_fast_u64(s, t, (const uint64_t *)a, (uint64_t *)c, batch, st)
      : mode == 3 ? launch_ntt_inv_fast_u64(s, t, (const uint64_t *)a, (uint64_t *)c, batch, st)
                  : launch_polymul_fast_u64(s, t, (uint64_t *)c, (const uint64_t *)a, (const uint64_t *)b, mode, batch, st);
    if (e == hipErrorNotSupported) e = launch_row1024_u64(s, t, mode, (uint64_t *)c, (const uint64_t *)a, (const uint64_t *)b, batch, st);
  } else if (s.limb_bits == 32) {
    e = launch_row1024_u32(s, t, mode, (uint32_t *)c, (const uint32_t *)a, (const uint32_t *)b, batch, st);
  } else {
    e = launch_row128_u16_asm(s, t, mode, (uint16_t *)c, (const uint16_t *)a, (const uint16_t *)b, batch, st);
  }
  if (e == hipSuccess) return NFLHIP_OK;
  if (e == hipErrorNotSupported) return NFLHIP_ERR_UNSUPPORTED;
  static const char *const op[4] = {"polymul", "polymul", "ntt_fwd", "ntt_inv"};
  return hipfail(ctx, e, (std::string(op[mode]) + (s.limb_bits == 64 ? "(fast)" : s.limb_bits == 32 ? "(u32)" : "(u16)")).c_str());
}

static int ntt_dev(nflhip_ctx *ctx, int inverse, void *d, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (!d && batch) return fail(ctx, NFLHIP_ERR_INVALID, "NULL data pointer");
  hipStream_t st = (hipStream_t)stream;
  const int rc = fast_family(ctx, inverse ? 3 : 2, d, d, nullptr, batch, st);
  if (rc != NFLHIP_ERR_UNSUPPORTED) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return inverse ? launch_ntt_inv<T>(ctx->shape, ctx->tabs, (const T *)d, nullptr, (T *)d, batch, st)
                   : launch_ntt_fwd<T>(ctx->shape, ctx->tabs, (const T *)d, (T *)d, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, inverse ? "ntt_inv" : "ntt_fwd");
  return NFLHIP_OK;
}
int nflhip_ntt_fwd_dev(nflhip_ctx *ctx, void *d, size_t batch, void *stream) { return ntt_dev(ctx, 0, d, batch, stream); }
int nflhip_ntt_inv_dev(nflhip_ctx *ctx, void *d, size_t batch, void *stream) { return ntt_dev(ctx, 1, d, batch, stream); }

// Galois automorphisms (kernels_automorph.hip).  The arguments are checked in full before anything is enqueued.
static int automorphism_multi(nflhip_ctx *ctx, void *const *outs, const uint64_t *ks, size_t count, const void *in, size_t batch,
                              int form, hipStream_t st) {
  if (form != NFLHIP_FORM_COEFF && form != NFLHIP_FORM_NTT) return fail(ctx, NFLHIP_ERR_INVALID, "unknown polynomial form");
  if (count == 0 || count > NFLHIP_AUTOMORPHISM_MAX_OUTPUTS) return fail(ctx, NFLHIP_ERR_INVALID, "output count out of range (1 to 16)");
  if (!outs || !ks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL output or multiplier array");
  for (size_t m = 0; m < count; ++m)
    if ((ks[m] & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism exponent k must be odd");
  if (batch == 0) return NFLHIP_OK;
  if (!in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL input");
  const size_t bytes = poly_bytes(ctx, batch);
  for (size_t m = 0; m < count; ++m) {
    if (!outs[m]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL output");
    if (bytes_overlap(outs[m], in, bytes)) return fail(ctx, NFLHIP_ERR_INVALID, "an output overlaps the input");
    for (size_t l = 0; l < m; ++l)
      if (bytes_overlap(outs[m], outs[l], bytes)) return fail(ctx, NFLHIP_ERR_INVALID, "two outputs overlap");
  }
  const int ntt = form == NFLHIP_FORM_NTT, c = (int)count;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_automorphism<T>(ctx->shape, ctx->tabs, (T *const *)outs, ks, c, (const T *)in, ntt, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "automorphism");
  return NFLHIP_OK;
}
int nflhip_automorphism_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, uint64_t k, int form, void *stream) {
  CHECK_CTX(ctx);
  void *outs[1] = {d_out};
  return automorphism_multi(ctx, outs, &k, 1, d_in, batch, form, (hipStream_t)stream);
}
int nflhip_automorphism_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const uint64_t *ks, size_t count, const void *d_in,
                                  size_t batch, int form, void *stream) {
  CHECK_CTX(ctx);
  return automorphism_multi(ctx, d_outs, ks, count, d_in, batch, form, (hipStream_t)stream);
}

// RNS rescale by the last modulus (kernels_rescale.hip).  The composed NTT-form plan: the dropped rows go to context-owned scratch
// and through the inverse transform of a one-modulus child context (the last modulus); d_i = (h - r) mod p_i is expanded into the
// output, which the child context over the first nm - 1 moduli forward-transforms in place; one pass combines it with the kept
// input rows.  Every transform launcher of the project therefore serves it, the compiled ones under NFLHIP_VARIANT=hipcc.
static int rescale_children(nflhip_ctx *ctx, bool cap) {  // under resc_mu
  const size_t nm = ctx->shape.nm;
  const char *refusal = "rescale: the composed plan's child contexts have to be created, which a stream capture cannot do";
  int rc = NFLHIP_OK;
  if (!ctx->resc_last) rc = child_create(ctx, 1, [nm](size_t) { return nm - 1; }, 0, cap, refusal, &ctx->resc_last);
  if (!rc && !ctx->resc_kept) rc = child_create(ctx, nm - 1, [](size_t i) { return i; }, 0, cap, refusal, &ctx->resc_kept);
  return rc;
}
static int rescale_composed(nflhip_ctx *ctx, void *out, const void *in, size_t batch, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->resc_mu);
  const size_t row = ctx->shape.n * ctx->word, nm = ctx->shape.nm;
  const bool cap = is_capturing(st);
  int rc = rescale_children(ctx, cap);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Workspace &ws = ctx->resc_ws;
  if ((rc = ws_begin(ctx, ws, batch * row, cap, st, "rescale: the composed plan's"))) return rc;
  HIPCHK(ctx, hipMemcpy2DAsync(ws.buf, row, (const char *)in + (nm - 1) * row, nm * row, row, batch, hipMemcpyDeviceToDevice, st));
  rc = nflhip_ntt_inv_dev(ctx->resc_last, ws.buf, batch, st);
  if (rc) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_rescale_expand<T>(ctx->shape, ctx->tabs, (T *)out, (const T *)ws.buf, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "rescale: expand");
  if ((rc = ws_end(ctx, ws, cap, st))) return rc;  // (here: the expand was the workspace's last reader)
  rc = nflhip_ntt_fwd_dev(ctx->resc_kept, out, batch, st);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_rescale_combine<T>(ctx->shape, ctx->tabs, (T *)out, (const T *)in, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "rescale: combine");
  return NFLHIP_OK;
}
// Where the one-launch kernel serves the NTT form by default: rows below 32 KiB.  Measured against the composed plan in one run
// (profiles/r08_rescale.txt): 1.45x faster at u64/1024/2, 1.03x at u32/1024/2, but 0.95x at u64/4096/4 (rows of 32 KiB), where the
// generated register-tiled transforms of the composed plan outrun the radix-4 LDS transforms by more than the traffic they add.
static bool rescale_fused_on(const nflhip_ctx *ctx) {
  return !ctx->shape.compiled_only && ctx->shape.n * ctx->word < 32768;
}

int nflhip_rescale_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, int form, void *stream) {
  int rc = rescale_check(ctx, d_out, d_in, batch, form, false);  // in full, before any device use
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (form == NFLHIP_FORM_COEFF) {
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_rescale_coeff<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, batch, st);
    });
    return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "rescale");
  }
  const bool forced = (form & NFLHIP_RESCALE_FUSED) != 0;
  if (forced || (form == NFLHIP_FORM_NTT && rescale_fused_on(ctx))) {
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_rescale_ntt_fused<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, batch, st);
    });
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "rescale (fused)");
    if (forced) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "rescale: two rows of this shape do not fit the one-launch kernel's LDS");
  }
  return rescale_composed(ctx, d_out, d_in, batch, st);
}

// Sums of products across polynomials (kernels_dot.hip).  A shared operand takes the tiled plan by default: it is read once per four
// groups.  Measured against the untiled plan at 4 / 16 / 64 terms (profiles/r09_dot.txt): 7 % faster at 16, level
// at 4 and 64, nowhere slower by more than two runs differ, so the rule has no threshold.
static bool dot_tiled_on(const nflhip_dot_operand *a, const nflhip_dot_operand *b, size_t groups, int flags) {
  return !(flags & NFLHIP_DOT_UNTILED) && groups > 1 && (a->group_stride == 0 || b->group_stride == 0);
}
int nflhip_dot_dev(nflhip_ctx *ctx, void *d_out, const nflhip_dot_operand *a, const nflhip_dot_operand *b, const void *d_addend,
                   size_t groups, size_t terms, int flags, void *stream) {
  int rc = dot_check(ctx, d_out, a, b, d_addend, groups, terms, flags);  // in full, before any device use
  if (rc || groups == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const int tiled = dot_tiled_on(a, b, groups, flags);
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_dot<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)a->ptr, a->group_stride, a->term_stride, (const T *)b->ptr,
                         b->group_stride, b->term_stride, (const T *)d_addend, groups, terms, tiled, (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "dot");
}
int nflhip_dot_ptrs_dev(nflhip_ctx *ctx, void *d_out, const void *const *d_a, const void *const *d_b, size_t terms, const void *d_addend,
                        void *stream) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "dot: not on a cyclic row context");
  if (terms == 0 || terms > NFLHIP_DOT_MAX_POINTERS) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the pointer form takes 1 to 16 terms");
  if (!d_out || !d_a || !d_b) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t pb = poly_bytes(ctx, 1);
  for (size_t j = 0; j < terms; ++j) {
    if (!d_a[j] || !d_b[j]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    if (bytes_overlap(d_out, d_a[j], pb) || bytes_overlap(d_out, d_b[j], pb)) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the output overlaps an operand");
  }
  int rc = dot_check_out(ctx, d_out, pb, d_addend);
  if (rc || (rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_dot_ptrs<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *const *)d_a, (const T *const *)d_b, terms, (const T *)d_addend,
                              (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "dot (pointer form)");
}

// Several outputs against one first operand (kernels_dot_multi.hip).  Two groups per load of b's words unless NFLHIP_DOT_UNTILED.
int nflhip_dot_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const nflhip_dot_operand *a, const void *const *d_bs, size_t b_term_stride,
                         size_t outputs, size_t groups, size_t terms, int flags, void *stream) {
  int rc = dot_multi_check(ctx, d_outs, a, d_bs, b_term_stride, outputs, groups, terms, flags);  // in full, before any device use
  if (rc || groups == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_dot_multi<T>(ctx->shape, ctx->tabs, (T *const *)d_outs, (const T *)a->ptr, a->group_stride, a->term_stride,
                               (const T *const *)d_bs, b_term_stride, outputs, groups, terms, !(flags & NFLHIP_DOT_UNTILED), (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "dot_multi");
}

// Gadget decomposition (kernels_decompose.hip).  The coefficient form is one streaming pass.  The NTT form has two plans with the
// same words: composed -- the streaming pass into the output, then the context's own forward launcher in place over batch * terms
// polynomials (every shape, the compiled kernels under NFLHIP_VARIANT=hipcc, no scratch of its own) -- and the one-launch kernel
// (rows up to 32 KiB).  Default: the one-launch kernel for rows of up to 2048 words.  Measured against the composed plan in one run
// (profiles/r11_decompose.txt), composed / fused: x1.17 at u64/1024/2, x1.08 at u64/2048/2, x1.02 at u32/1024/2, but
// x0.70 at u64/4096/4 and x0.62 at u32/4096/3 -- at 4096 words the generated register-tiled transforms of the composed plan outrun
// the radix-4 LDS transform by more than the two extra passes over the output cost, for 16 KiB and 32 KiB rows alike, so the rule
// is in words, not bytes.
static bool decompose_fused_on(const nflhip_ctx *ctx) {
  return !ctx->shape.compiled_only && ctx->shape.n <= 2048;
}
size_t nflhip_decompose_terms(const nflhip_ctx *ctx, int w) { return decompose_terms(ctx, w); }
int nflhip_decompose_dev(nflhip_ctx *ctx, void *d_out, int out_format, const void *d_in, size_t batch, int w, int flags, void *stream) {
  if (out_format < 0) return fail(ctx, NFLHIP_ERR_INVALID, "decompose: unknown output format");
  int rc = decompose_check(ctx, d_out, out_format, d_in, batch, w, flags, nullptr);  // in full, before any device use
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int sgn = (flags & NFLHIP_DECOMP_SIGNED) != 0;
  const bool ntt = (flags & NFLHIP_FORM_NTT) != 0, forced = (flags & NFLHIP_DECOMP_FUSED) != 0;
  hipError_t e;
  if (out_format != NFLHIP_FMT_WORDS) {
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_decompose_compact<T>(ctx->shape, ctx->tabs, d_out, out_format, (const T *)d_in, batch, w, sgn, st);
    });
    return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "decompose (compact)");
  }
  if (ntt && (forced || (!(flags & NFLHIP_DECOMP_COMPOSED) && decompose_fused_on(ctx)))) {
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_decompose_ntt_fused<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, batch, w, sgn, st);
    });
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "decompose (fused)");
    if (forced) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "decompose: a row of this shape does not fit the one-launch kernel's LDS");
  }
  e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_decompose_words<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, batch, w, sgn, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "decompose");
  return ntt ? nflhip_ntt_fwd_dev(ctx, d_out, batch * decompose_terms(ctx, w), stream) : NFLHIP_OK;
}
int nflhip_gadget_mul_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, int w, void *stream) {
  int rc = decompose_check(ctx, d_out, -1, d_in, batch, w, 0, nullptr);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_gadget_mul<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, batch, w, (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "gadget_mul");
}

// RNS base conversion and mod-down (kernels_baseconv.hip).  The record of a pair of row ranges (host_tables.cpp
// build_baseconv_record) is built and uploaded by the first call that names the pair and kept until the context goes: that call
// allocates and copies synchronously, later calls only look the pointer up.  The record is complete before it enters the map, and the
// kernels of any stream read it only after this function returned it.
static int baseconv_record(nflhip_ctx *ctx, size_t s0, size_t ks, size_t d0, size_t kd, bool moddown, hipStream_t st, const uint64_t **rec) {
  std::lock_guard<std::mutex> lk(ctx->bconv_mu);
  const std::array<size_t, 5> key = {s0, ks, d0, kd, moddown ? (size_t)1 : (size_t)0};
  auto it = ctx->bconv.find(key);
  if (it != ctx->bconv.end()) {
    *rec = (const uint64_t *)it->second;
    return NFLHIP_OK;
  }
  std::vector<uint64_t> h;
  std::string err;
  int rc;
  try {
    rc = build_baseconv_record(ctx->shape.limb_bits, ctx->h_P, s0, ks, d0, kd, moddown, &h, &err);
  } catch (const std::bad_alloc &) {
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory while building the base conversion tables");
  }
  if (rc) return fail(ctx, rc, err);  // (host arithmetic only: a repeated modulus is refused before any device use)
  if (is_capturing(st))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "baseconv: the first call for a pair of row ranges uploads its tables, which a stream capture cannot do");
  if ((rc = set_device(ctx))) return rc;
  void *d = nullptr;
  HIPCHK(ctx, hipMalloc(&d, h.size() * sizeof(uint64_t)));
  hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hipfail(ctx, e, "baseconv: table upload");
  }
  try {
    ctx->bconv[key] = d;
  } catch (const std::bad_alloc &) {
    (void)hipFree(d);
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  }
  *rec = (const uint64_t *)d;
  return NFLHIP_OK;
}
static int baseconv_run(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, bool centred,
                        bool moddown, hipStream_t st) {
  if (batch == 0) return NFLHIP_OK;  // (touches nothing: no record is built for an empty batch)
  const uint64_t *rec = nullptr;
  int rc = baseconv_record(ctx, s0, ks, d0, kd, moddown, st, &rec);
  if (rc || (rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_baseconv<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, rec, batch, s0, ks, d0, kd, centred, moddown, st);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, moddown ? "moddown" : "baseconv");
}
int nflhip_baseconv_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags,
                        void *stream) {
  int rc = baseconv_check(ctx, d_out, d_in, batch, s0, ks, d0, kd, flags, false);  // in full, before any device use
  if (rc) return rc;
  return baseconv_run(ctx, d_out, d_in, batch, s0, ks, d0, kd, (flags & NFLHIP_BASECONV_CENTERED) != 0, false, (hipStream_t)stream);
}
int nflhip_moddown_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t k, int flags, void *stream) {
  const size_t nm = ctx ? ctx->shape.nm : 0, kept = k < nm ? nm - k : 0;
  int rc = baseconv_check(ctx, d_out, d_in, batch, kept, k, 0, kept, flags, true);  // in full, before any device use
  if (rc) return rc;
  return baseconv_run(ctx, d_out, d_in, batch, kept, k, 0, kept, !(flags & NFLHIP_MODDOWN_FLOOR), true, (hipStream_t)stream);
}

// The same on NTT-form data (kernels_baseconv_ntt.hip).  Two plans with the same words, each the other's cross-check:
//   fused     one launch, the source rows in LDS (launch_baseconv_ntt_fused); needs (ks + 1 + centred) rows within 64 KiB
//   composed  the source rows gathered into context-owned scratch and inverse-transformed by a child context over the moduli of S;
//             k_baseconv converts from the scratch (launch_baseconv_rows); the result is forward-transformed -- by the context
//             itself when D is every row, else in a second scratch by a child context over the moduli of D and scattered to rows
//             D; the mod-down converts into the dense output, transforms it with the child over the first nm - k moduli and
//             combines it with the input's kept rows in one streaming pass.  Every transform launcher of the project serves it.
// The child context over (first row, count): created on first use, never while capturing.  (0, nm) is the context itself.
static int bcn_child(nflhip_ctx *ctx, size_t first, size_t count, bool cap, nflhip_ctx **out) {  // under bcn_mu
  if (first == 0 && count == ctx->shape.nm) {
    *out = ctx;
    return NFLHIP_OK;
  }
  return child_in_map(ctx, ctx->bcn_child, {first, count}, count, [first](size_t i) { return first + i; }, cap,
                      "baseconv_ntt: the composed plan's child context has to be created, which a stream capture cannot do", out);
}
// ... the same for a caller that does not hold bcn_mu: the child over the rows [0, L)
static int kept_rows_child(nflhip_ctx *ctx, size_t L, bool cap, nflhip_ctx **out) {
  std::lock_guard<std::mutex> lk(ctx->bcn_mu);
  int rc = bcn_child(ctx, 0, L, cap, out);
  return rc ? rc : set_device(ctx);
}
static int baseconv_ntt_composed(nflhip_ctx *ctx, void *out, const void *in, const uint64_t *rec, size_t batch, size_t s0, size_t ks, size_t d0,
                                 size_t kd, bool centred, bool moddown, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->bcn_mu);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t row = ctx->shape.n * ctx->word, nm = ctx->shape.nm;
  const bool cap = is_capturing(st), whole = !moddown && d0 == 0 && kd == nm;
  nflhip_ctx *cs = nullptr, *cd = nullptr;
  int rc = bcn_child(ctx, s0, ks, cap, &cs);
  if (!rc) rc = bcn_child(ctx, d0, kd, cap, &cd);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const char *what = "baseconv_ntt: the composed plan's";
  // (the second workspace starts d0 rows early: k_baseconv writes row d0 + j of a polynomial of kd rows, so the dense rows begin at
  // row d0 of the buffer)
  if (!moddown && !whole && (rc = ws_grow(ctx, ctx->bcn_ws[1], (d0 + batch * kd) * row, cap, what))) return rc;
  if ((rc = ws_begin(ctx, ctx->bcn_ws[0], batch * ks * row, cap, st, what))) return rc;
  void *src = ctx->bcn_ws[0].buf;
  HIPCHK(ctx, hipMemcpy2DAsync(src, ks * row, (const char *)in + s0 * row, nm * row, ks * row, batch, hipMemcpyDeviceToDevice, st));
  rc = nflhip_ntt_inv_dev(cs, src, batch, st);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  void *conv = moddown || whole ? out : ctx->bcn_ws[1].buf;  // where k_baseconv's polynomial 0, row 0 would be
  const size_t onm = moddown || !whole ? kd : nm;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_baseconv_rows<T>(ctx->shape, ctx->tabs, (T *)conv, onm, (const T *)src, ks, rec, batch, ks, d0, kd, centred, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "baseconv_ntt: conversion");
  void *dense = moddown || whole ? out : (void *)((char *)conv + d0 * row);
  rc = nflhip_ntt_fwd_dev(cd, dense, batch, st);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (moddown) {
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_moddown_ntt_combine<T>(ctx->shape, (T *)out, (const T *)in, rec, batch, ks, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, "moddown_ntt: combine");
  } else if (!whole) {
    HIPCHK(ctx, hipMemcpy2DAsync((char *)out + d0 * row, nm * row, dense, kd * row, kd * row, batch, hipMemcpyDeviceToDevice, st));
  }
  return ws_end(ctx, ctx->bcn_ws[0], cap, st);
}
// Where the one-launch kernel serves by default: when its rows fit the LDS and a row has up to 2048 words.  Measured against the
// composed plan in one run, alternated (profiles/r13_baseconv_ntt.txt), composed / fused: x1.43 - x1.78 for the mod-ups
// 1 -> 4 and 2 -> 4 and x1.09 - x1.45 for the mod-downs k = 1, 2 at u64/1024/4 and u64/2048/4, but x0.82 / x0.73 at u32/4096/3 (rows of
// 16 KiB) and x0.88 at u64/4096/4 (32 KiB) -- at 4096 words the generated register-tiled transforms of the composed plan outrun the
// radix-4 LDS transforms by more than the gather and the extra passes cost, whatever the row's bytes: the rule is in words, as
// decompose_fused_on.  Contexts created under NFLHIP_VARIANT=hipcc compose.
static bool rows_take_lds_conversions(const nflhip_ctx *ctx) {  // THE rule in words; the plans built on the conversions ask it too
  return ctx->shape.n <= 2048;
}
static bool baseconv_ntt_fused_on(const nflhip_ctx *ctx) {
  return !ctx->shape.compiled_only && rows_take_lds_conversions(ctx);
}
static int baseconv_ntt_run(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags,
                            bool centred, bool moddown, hipStream_t st) {
  if (batch == 0) return NFLHIP_OK;  // (touches nothing: no record is built for an empty batch)
  const uint64_t *rec = nullptr;
  int rc = baseconv_record(ctx, s0, ks, d0, kd, moddown, st, &rec);
  if (rc || (rc = set_device(ctx))) return rc;
  const bool forced = (flags & NFLHIP_BASECONV_NTT_FUSED) != 0;
  if (forced || (!(flags & NFLHIP_BASECONV_NTT_COMPOSED) && baseconv_ntt_fused_on(ctx))) {
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_baseconv_ntt_fused<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_in, rec, batch, s0, ks, d0, kd, centred, moddown, st);
    });
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, moddown ? "moddown_ntt (fused)" : "baseconv_ntt (fused)");
    if (forced) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "baseconv_ntt: the source rows of this call do not fit the one-launch kernel's LDS");
  }
  return baseconv_ntt_composed(ctx, d_out, d_in, rec, batch, s0, ks, d0, kd, centred, moddown, st);
}
int nflhip_baseconv_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags,
                            void *stream) {
  int rc = baseconv_ntt_check(ctx, d_out, d_in, batch, s0, ks, d0, kd, flags, false);  // in full, before any device use
  if (rc) return rc;
  return baseconv_ntt_run(ctx, d_out, d_in, batch, s0, ks, d0, kd, flags, (flags & NFLHIP_BASECONV_CENTERED) != 0, false, (hipStream_t)stream);
}
int nflhip_moddown_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t k, int flags, void *stream) {
  const size_t nm = ctx ? ctx->shape.nm : 0, kept = k < nm ? nm - k : 0;
  int rc = baseconv_ntt_check(ctx, d_out, d_in, batch, kept, k, 0, kept, flags, true);  // in full, before any device use
  if (rc) return rc;
  return baseconv_ntt_run(ctx, d_out, d_in, batch, kept, k, 0, kept, flags, !(flags & NFLHIP_MODDOWN_FLOOR), true, (hipStream_t)stream);
}

// Calls below the top level (kernels_level.hip; include/nflhip.h "leveled key switching").  The level context C_l over the rows
// [0, level) and [nm - K, nm) of this one -- a subsequence of the moduli, in their order: created on first use, never while
// capturing, destroyed with this context.  keyswitch_run and mulrelin_run then run on it as they are, with its own records, scratch,
// events and warm maps; the key alone stays in this context's layout, described by a KeyLevel that travels to the three launchers
// which read it (dot_key and the two one-launch kernels).  rotate_run and lintrans_run run on it likewise (kernels_level_rotate.hip).
static int level_child(nflhip_ctx *ctx, size_t K, size_t level, bool cap, nflhip_ctx **out) {
  std::lock_guard<std::mutex> lk(ctx->bcn_mu);
  const size_t count = level + K, hole = ctx->shape.nm - count;
  return child_in_map(ctx, ctx->lvl_child, {K, level}, count, [level, hole](size_t i) { return i < level ? i : hole + i; }, cap,
                      "level: the first call at a (k_special, level) creates its context, which a stream capture cannot do", out);
}
// acc = [addend +] sum_d a(., d) (.) key[d][c]: nflhip_dot_dev with the key as the shared second operand, a term every two polynomials;
// kl: the key lies in the parent's layout (ctx is a level context)
static int dot_key(nflhip_ctx *ctx, void *out, const nflhip_dot_operand *a, const void *key, size_t c, const void *addend, size_t groups,
                   size_t terms, const KeyLevel *kl, hipStream_t st) {
  if (!kl) {
    const nflhip_dot_operand b = {(const char *)key + c * poly_bytes(ctx, 1), 0, 2};
    return nflhip_dot_dev(ctx, out, a, &b, addend, groups, terms, 0, st);
  }
  if (terms == 0 || terms > nflhip::kDotMaxTerms) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the number of terms is out of range (1 to 2^31)");  // (as dot_check)
  int rc = set_device(ctx);
  if (rc) return rc;
  const char *kc = (const char *)key + c * kl->knm * ctx->shape.n * ctx->word;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_dot_key_level<T>(ctx->shape, ctx->tabs, (T *)out, (const T *)a->ptr, a->group_stride, a->term_stride, (const T *)kc,
                                   (const T *)addend, groups, terms, groups > 1, *kl, st);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "dot (level key)");
}

// Hybrid key switching in NTT form (kernels_keyswitch.hip; include/nflhip.h "hybrid key switching"): the mod-up of every digit, the
// two inner products against the key and the mod-down of both sums, defined as the composition of nflhip_baseconv_ntt_dev,
// nflhip_dot_dev and nflhip_moddown_ntt_dev.  Three plans with the same words:
//   sequence  that composition itself over context-owned scratch: X = the input embedded in nm rows, U = [dnum][batch][nm][n]
//   composed  one inverse transform of the child context over rows [0, L), k_modup_digits into U = [batch][dnum][nm][n], one forward
//             transform of the context over batch dnum polynomials
//   fused     k_modup_dot_fused straight to the sums
// then (sequence, composed) nflhip_dot_dev twice into acc = [2][batch][nm][n] and, for all, nflhip_moddown_ntt_dev -- one call of
// 2 batch polynomials when out1 follows out0 in memory (Engine.key_switch_ntt allocates them so), else one per output.
// The records are those of baseconv_record: every digit's and the mod-down's are built BEFORE anything is enqueued, so a repeated
// modulus is refused with the builder's message and nothing written.
// UNDER ks_mu, which is not recursive and which this function therefore never takes: keyswitch_run holds it for its whole call, the
// other three callers take it around this fetch alone (after their own mutex, before bcn_mu).
static int keyswitch_records(nflhip_ctx *ctx, size_t K, size_t alpha, hipStream_t st, const uint64_t *const **recs) try {
  const size_t nm = ctx->shape.nm, L = nm - K, dnum = (L + alpha - 1) / alpha;
  std::vector<const uint64_t *> h(dnum);
  const uint64_t *down = nullptr;
  int rc = NFLHIP_OK;
  for (size_t d = 0; d < dnum && !rc; ++d) rc = baseconv_record(ctx, d * alpha, std::min(alpha, L - d * alpha), 0, nm, false, st, &h[d]);
  if (!rc) rc = baseconv_record(ctx, L, K, 0, L, true, st, &down);
  if (rc) return rc;
  const std::array<size_t, 2> key = {K, alpha};
  auto it = ctx->ks_recs.find(key);
  if (it == ctx->ks_recs.end()) {
    if (is_capturing(st))
      return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "keyswitch: the first call for a (k_special, alpha) uploads its tables, which a stream capture cannot do");
    if ((rc = set_device(ctx))) return rc;
    void *d = nullptr;
    HIPCHK(ctx, hipMalloc(&d, dnum * sizeof(uint64_t *)));
    hipError_t e = hipMemcpy(d, h.data(), dnum * sizeof(uint64_t *), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hipfail(ctx, e, "keyswitch: table upload");
    }
    it = ctx->ks_recs.emplace(key, d).first;
  }
  *recs = (const uint64_t *const *)it->second;
  return NFLHIP_OK;
} catch (const std::bad_alloc &) {
  return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
}
// Which plan serves by default.  Measured against the sequence in one run, alternated (profiles/r14_keyswitch.txt),
// sequence / plan: the one-launch kernel x1.11 / x1.10 at u64/1024/4 (alpha 1 / 3) and x1.05 at u64/2048/4; the composed plan x0.84 /
// x0.93 / x0.88 at those points -- the LDS transforms of the sequence's one-launch conversions beat its separate passes -- but x1.02 /
// x1.04 / x1.02 at u64/4096/4 (K 1 / 2) and u32/4096/3, where the sequence composes as well and the composed plan saves dnum - 1
// inverse transforms; every block of the run within 1.1 % of its median.  So: the one-launch kernel where it fits; past it the
// composed plan for rows above 2048 words and the sequence for shorter ones, where the composed plan measured slower.
static int keyswitch_default_plan(const nflhip_ctx *ctx, size_t L, size_t dnum, bool centred) {
  if (!ctx->shape.compiled_only && keyswitch_fused_fits(L, dnum, ctx->shape.n, ctx->word, centred)) return NFLHIP_KEYSWITCH_FUSED;
  return rows_take_lds_conversions(ctx) ? NFLHIP_KEYSWITCH_SEQUENCE : NFLHIP_KEYSWITCH_COMPOSED;
}
// The mod-up of every digit of `batch` polynomials on L rows, by one of two routes with the same words:
//   per digit   X = the input embedded in nm rows; nflhip_baseconv_ntt_dev per digit: U = [dnum][batch][nm][n], the operand {U, 1, batch}
//   all digits  X = the input, L rows dense; one inverse transform by the child over rows [0, L), k_modup_digits, one forward transform
//               of this context over batch dnum polynomials: U = [batch][dnum][nm][n], the operand {U, dnum, 1}
// The route is the CALLER's: the key switch takes it from its plan (the sequence is per digit, the composed plan all digits), the
// entries built on the mod-up from modup_default_route -- so a context created under NFLHIP_VARIANT=hipcc with rows up to 2048 words
// goes per digit in the key switch's default plan and all digits in theirs.
enum ModupRoute { kModupPerDigit, kModupAllDigits };
static ModupRoute modup_default_route(const nflhip_ctx *ctx) { return baseconv_ntt_fused_on(ctx) ? kModupPerDigit : kModupAllDigits; }
static size_t modup_x_bytes(const nflhip_ctx *ctx, ModupRoute route, size_t batch, size_t L) {
  return batch * (route == kModupPerDigit ? ctx->shape.nm : L) * ctx->shape.n * ctx->word;
}
// X from an input that lies elsewhere (the merged multiplication has none: its tensor kernel writes X)
static int modup_copy_in(nflhip_ctx *ctx, ModupRoute route, void *X, const void *in, size_t batch, size_t L, hipStream_t st) {
  const size_t row = ctx->shape.n * ctx->word, pb = ctx->shape.nm * row, qb = L * row;
  if (route == kModupPerDigit) HIPCHK(ctx, hipMemcpy2DAsync(X, pb, in, qb, qb, batch, hipMemcpyDeviceToDevice, st));
  else HIPCHK(ctx, hipMemcpyAsync(X, in, batch * qb, hipMemcpyDeviceToDevice, st));
  return NFLHIP_OK;
}
// U and its operand *u from X; `child`: the context over rows [0, L) (all digits); `what`: the entry, for an error's text
static int modup_run(nflhip_ctx *ctx, nflhip_ctx *child, ModupRoute route, void *U, void *X, const uint64_t *const *recs, size_t batch, size_t L,
                     size_t alpha, bool centred, const char *what, hipStream_t st, nflhip_dot_operand *u) {
  const size_t nm = ctx->shape.nm, dnum = (L + alpha - 1) / alpha, pb = nm * ctx->shape.n * ctx->word;
  int rc;
  if (route == kModupPerDigit) {
    for (size_t d = 0; d < dnum; ++d)
      if ((rc = nflhip_baseconv_ntt_dev(ctx, (char *)U + d * batch * pb, X, batch, d * alpha, std::min(alpha, L - d * alpha), 0, nm,
                                        centred ? NFLHIP_BASECONV_CENTERED : 0, st)))
        return rc;
    *u = {U, 1, batch};
  } else {
    if ((rc = nflhip_ntt_inv_dev(child, X, batch, st)) || (rc = set_device(ctx))) return rc;
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_modup_digits<T>(ctx->shape, ctx->tabs, (T *)U, (const T *)X, recs, batch, L, alpha, centred, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, (std::string(what) + ": mod-up").c_str());
    if ((rc = nflhip_ntt_fwd_dev(ctx, U, batch * dnum, st))) return rc;
    *u = {U, dnum, 1};
  }
  return set_device(ctx);
}
// The mod-down of the two sums acc = [2][batch][nm][n] by the last `drop` rows: one call of 2 batch polynomials when out1 follows out0
// in memory (the Engine allocates them so), else one per output
static bool moddown_pair_adjacent(const nflhip_ctx *ctx, const void *out0, const void *out1, size_t batch, size_t drop) {
  return (const char *)out1 == (const char *)out0 + batch * (ctx->shape.nm - drop) * ctx->shape.n * ctx->word;
}
static int moddown_pair(nflhip_ctx *ctx, void *out0, void *out1, const void *acc, size_t batch, size_t drop, bool floor, hipStream_t st) {
  const int mdflags = floor ? NFLHIP_MODDOWN_FLOOR : 0;
  int rc;
  if (moddown_pair_adjacent(ctx, out0, out1, batch, drop)) {
    rc = nflhip_moddown_ntt_dev(ctx, out0, acc, 2 * batch, drop, mdflags, st);
  } else {
    rc = nflhip_moddown_ntt_dev(ctx, out0, acc, batch, drop, mdflags, st);
    if (!rc) rc = nflhip_moddown_ntt_dev(ctx, out1, (const char *)acc + poly_bytes(ctx, batch), batch, drop, mdflags, st);
  }
  return rc ? rc : set_device(ctx);
}
static int keyswitch_run(nflhip_ctx *ctx, void *out0, void *out1, const void *in, const void *key, size_t batch, size_t K, size_t alpha, int flags,
                         hipStream_t st, const KeyLevel *kl = nullptr) {
  std::lock_guard<std::mutex> lk(ctx->ks_mu);
  const size_t nm = ctx->shape.nm, L = nm - K, dnum = (L + alpha - 1) / alpha, pb = nm * ctx->shape.n * ctx->word;
  const bool centred = (flags & NFLHIP_KEYSWITCH_CENTERED) != 0, floor = (flags & NFLHIP_KEYSWITCH_FLOOR) != 0, cap = is_capturing(st);
  const uint64_t *const *recs = nullptr;
  int rc = keyswitch_records(ctx, K, alpha, st, &recs);
  if (rc) return rc;
  int plan = flags & (NFLHIP_KEYSWITCH_COMPOSED | NFLHIP_KEYSWITCH_FUSED | NFLHIP_KEYSWITCH_SEQUENCE);
  if (plan == NFLHIP_KEYSWITCH_FUSED && !keyswitch_fused_fits(L, dnum, ctx->shape.n, ctx->word, centred))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "keyswitch: the rows of this call do not fit the one-launch kernel's LDS");
  if (!plan) plan = keyswitch_default_plan(ctx, L, dnum, centred);
  // what a call while capturing may do: repeat a (k_special, alpha, plan, modes) already served at this batch or a larger one
  const std::array<size_t, 3> wkey = {K, alpha, (size_t)(plan | (flags & (NFLHIP_KEYSWITCH_CENTERED | NFLHIP_KEYSWITCH_FLOOR)))}, wsizes = {batch, 0, 0};
  if (cap && !warm_covers(ctx->ks_warm, wkey, wsizes))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "keyswitch: the first call for a (k_special, alpha, plan), or for a larger batch, allocates, which a stream capture cannot do");
  const bool fused = plan == NFLHIP_KEYSWITCH_FUSED;
  const ModupRoute route = plan == NFLHIP_KEYSWITCH_SEQUENCE ? kModupPerDigit : kModupAllDigits;
  const size_t xb = fused ? 0 : modup_x_bytes(ctx, route, batch, L), ub = fused ? 0 : batch * dnum * pb, ab = 2 * batch * pb;
  if ((rc = set_device(ctx))) return rc;
  nflhip_ctx *child = nullptr;
  if (plan == NFLHIP_KEYSWITCH_COMPOSED && (rc = kept_rows_child(ctx, L, cap, &child))) return rc;
  if ((rc = ws_begin(ctx, ctx->ks_ws, xb + ub + ab, cap, st, "keyswitch: the"))) return rc;
  char *X = (char *)ctx->ks_ws.buf, *U = X + xb, *acc = U + ub;
  if (fused) {
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      if (kl) return launch_modup_dot_fused_level<T>(ctx->shape, ctx->tabs, (T *)acc, (const T *)in, (const T *)key, recs, batch, L, alpha, centred, *kl, st);
      return launch_modup_dot_fused<T>(ctx->shape, ctx->tabs, (T *)acc, (const T *)in, (const T *)key, recs, batch, L, alpha, centred, st);
    });
    if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "keyswitch: the rows of this call do not fit the one-launch kernel's LDS");
    if (e != hipSuccess) return hipfail(ctx, e, "keyswitch (fused)");
  } else {
    nflhip_dot_operand a;
    if ((rc = modup_copy_in(ctx, route, X, in, batch, L, st))) return rc;
    if ((rc = modup_run(ctx, child, route, U, X, recs, batch, L, alpha, centred, "keyswitch", st, &a))) return rc;
    for (size_t c = 0; c < 2; ++c)
      if ((rc = dot_key(ctx, acc + c * batch * pb, &a, key, c, nullptr, batch, dnum, kl, st))) return rc;
  }
  if ((rc = moddown_pair(ctx, out0, out1, acc, batch, K, floor, st)) || (rc = ws_end(ctx, ctx->ks_ws, cap, st))) return rc;
  if (!cap) warm_note(ctx->ks_warm, wkey, wsizes);
  return NFLHIP_OK;
}
size_t nflhip_keyswitch_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha) { return keyswitch_digits(ctx, k_special, alpha); }
int nflhip_keyswitch_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch, size_t k_special,
                             size_t alpha, int flags, void *stream) {
  int rc = keyswitch_check(ctx, d_out0, d_out1, d_in, d_key, batch, k_special, alpha, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  return keyswitch_run(ctx, d_out0, d_out1, d_in, d_key, batch, k_special, alpha, flags, (hipStream_t)stream);
}

// Hoisted rotations (kernels_rotate.hip, kernels_dot_multi.hip; include/nflhip.h "hoisted rotations"): count key switches of one c1, each
// followed by the addition of c0 and the NTT-form automorphism -- the permutation LAST, so that the mod-up is shared.  Two plans with
// the same words:
//   sequence  per rotation nflhip_keyswitch_ntt_dev (its default plan) into T0, T1 = [batch][L][n], c0 added by nflhip_pointwise_dev on
//             the child context over rows [0, L) -- or, where that entry cannot serve (a pointer off 16 bytes, a batch that is no whole
//             number of 16-byte groups), by nflhip_dot_dev as c0 + T0 (.) 1 into T2 --, then nflhip_automorphism_dev twice
//   hoisted   the mod-up of c1 once into U (modup_run, the route modup_default_route's); k_dot_multi into S = [2 count][batch][nm][n];
//             one mod-down into Y = [2 count][batch][L][n]; k_permute_add_ntt
// Default: hoisted for count >= 2, the sequence for count == 1 (a single rotation has no mod-up to share and the key switch's own
// default plan is the measured best there).
// kl: ctx is a level context and the keys lie in its parent's layout (nflhip_rotate_hoisted_level_ntt_dev): the sequence calls
// keyswitch_run with it -- the public entry would read the key in this context's layout --, the hoisted plan the k_dot_multi instances
// of kernels_level_rotate.hip, the component pointers keys[m] + c knm n words.  Everything else is this context's own.
// Lock order: rot_mu, then ks_mu, then bcn_mu.
static int rotate_run(nflhip_ctx *ctx, void *const *out0s, void *const *out1s, const void *c0, const void *c1, const void *const *keys,
                      const uint64_t *ks, size_t count, size_t batch, size_t K, size_t alpha, int flags, hipStream_t st,
                      const KeyLevel *kl = nullptr) {
  std::lock_guard<std::mutex> lk(ctx->rot_mu);
  const size_t nm = ctx->shape.nm, L = nm - K, dnum = (L + alpha - 1) / alpha, row = ctx->shape.n * ctx->word, pb = nm * row, qb = L * row;
  const bool centred = (flags & NFLHIP_ROTATE_CENTERED) != 0, floor = (flags & NFLHIP_ROTATE_FLOOR) != 0, cap = is_capturing(st);
  const uint64_t *const *recs = nullptr;
  int rc;
  {  // the tables first: a repeated modulus is refused with the builder's message before anything is enqueued
    std::lock_guard<std::mutex> l2(ctx->ks_mu);
    rc = keyswitch_records(ctx, K, alpha, st, &recs);
  }
  if (rc) return rc;
  int plan = flags & (NFLHIP_ROTATE_SEQUENCE | NFLHIP_ROTATE_HOISTED);
  if (!plan) plan = count >= 2 ? NFLHIP_ROTATE_HOISTED : NFLHIP_ROTATE_SEQUENCE;
  const int modes = flags & (NFLHIP_ROTATE_CENTERED | NFLHIP_ROTATE_FLOOR);
  // what a call while capturing may do: repeat a (k_special, alpha, plan, modes) already served at this batch and count * batch or larger
  const std::array<size_t, 3> wkey = {K, alpha, (size_t)(plan | modes)}, wsizes = {batch, count * batch, 0};
  if (cap && !warm_covers(ctx->rot_warm, wkey, wsizes))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "rotate: the first call for a (k_special, alpha, plan), or for a larger batch, allocates, which a stream capture cannot do");
  const bool seq = plan == NFLHIP_ROTATE_SEQUENCE;
  const ModupRoute route = modup_default_route(ctx);
  // sequence: T0, T1, T2 and a polynomial of ones; hoisted: X, U, S, Y
  const size_t xb = seq ? 3 * batch * qb + qb : modup_x_bytes(ctx, route, batch, L);
  const size_t ub = seq ? 0 : batch * dnum * pb, sb = seq ? 0 : 2 * count * batch * pb, yb = seq ? 0 : 2 * count * batch * qb;
  if ((rc = set_device(ctx))) return rc;
  nflhip_ctx *child = nullptr;
  if ((rc = kept_rows_child(ctx, L, cap, &child)) || (rc = ws_begin(ctx, ctx->rot_ws, xb + ub + sb + yb, cap, st, "rotate: the"))) return rc;
  char *X = (char *)ctx->rot_ws.buf;
  if (seq) {
    char *T0 = X, *T1 = T0 + batch * qb, *T2 = T1 + batch * qb, *ones = T2 + batch * qb;
    const bool pw = (((uintptr_t)T0 | (uintptr_t)c0) & 15u) == 0 && (batch * qb) % 16 == 0;  // what nflhip_pointwise_dev serves
    if (c0 && !pw) {  // a polynomial of ones: every byte 0, then the low byte of every word 1
      HIPCHK(ctx, hipMemsetAsync(ones, 0, qb, st));
      HIPCHK(ctx, hipMemset2DAsync(ones, ctx->word, 1, 1, L * ctx->shape.n, st));
    }
    for (size_t m = 0; m < count; ++m) {
      // (the mode bits are the key switch's; at a level the public entry would read the key in this context's layout)
      if ((rc = kl ? keyswitch_run(ctx, T0, T1, c1, keys[m], batch, K, alpha, modes, st, kl)
                   : nflhip_keyswitch_ntt_dev(ctx, T0, T1, c1, keys[m], batch, K, alpha, modes, st)))
        return rc;
      const char *y0 = T0;
      if (c0 && pw) {
        if ((rc = nflhip_pointwise_dev(child, NFLHIP_OP_ADD, T0, T0, c0, nullptr, batch, st))) return rc;
      } else if (c0) {
        const nflhip_dot_operand a = {T0, 1, 1}, b = {ones, 0, 0};
        if ((rc = nflhip_dot_dev(child, T2, &a, &b, c0, batch, 1, 0, st))) return rc;
        y0 = T2;
      }
      if ((rc = nflhip_automorphism_dev(child, out0s[m], y0, batch, ks[m], NFLHIP_FORM_NTT, st))) return rc;
      if ((rc = nflhip_automorphism_dev(child, out1s[m], T1, batch, ks[m], NFLHIP_FORM_NTT, st))) return rc;
    }
    if ((rc = set_device(ctx))) return rc;
  } else {
    char *U = X + xb, *S = U + ub, *Y = S + sb;
    nflhip_dot_operand u;
    if ((rc = modup_copy_in(ctx, route, X, c1, batch, L, st))) return rc;
    if ((rc = modup_run(ctx, child, route, U, X, recs, batch, L, alpha, centred, "rotate", st, &u))) return rc;
    void *douts[2 * NFLHIP_ROTATE_MAX_OUTPUTS], *pouts[2 * NFLHIP_ROTATE_MAX_OUTPUTS];
    const void *dbs[2 * NFLHIP_ROTATE_MAX_OUTPUTS], *pins[2 * NFLHIP_ROTATE_MAX_OUTPUTS];
    uint64_t pks[2 * NFLHIP_ROTATE_MAX_OUTPUTS];
    unsigned add_mask = 0;
    for (size_t m = 0; m < count; ++m)
      for (size_t c = 0; c < 2; ++c) {
        const size_t p = 2 * m + c;
        douts[p] = S + p * batch * pb;
        dbs[p] = (const char *)keys[m] + c * (kl ? kl->knm * row : pb);
        pins[p] = Y + p * batch * qb;
        pouts[p] = c ? out1s[m] : out0s[m];
        pks[p] = ks[m];
        if (c == 0) add_mask |= 1u << p;
      }
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      if (kl)
        return launch_dot_multi_level<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, u.group_stride, u.term_stride,
                                         (const T *const *)dbs, 2 * count, batch, dnum, 1, *kl, st);
      return launch_dot_multi<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, u.group_stride, u.term_stride, (const T *const *)dbs, 2,
                                 2 * count, batch, dnum, 1, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, "rotate: inner products");
    if ((rc = nflhip_moddown_ntt_dev(ctx, Y, S, 2 * count * batch, K, floor ? NFLHIP_MODDOWN_FLOOR : 0, st)) || (rc = set_device(ctx))) return rc;
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_permute_add_ntt<T>(ctx->shape, ctx->tabs, (T *const *)pouts, (const T *const *)pins, pks, add_mask, (int)(2 * count),
                                       (const T *)c0, L, batch, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, "rotate: permutation");
  }
  if ((rc = ws_end(ctx, ctx->rot_ws, cap, st))) return rc;
  if (!cap) warm_note(ctx->rot_warm, wkey, wsizes);
  return NFLHIP_OK;
}
int nflhip_rotate_hoisted_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                  const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                  int flags, void *stream) {
  int rc = rotate_check(ctx, d_out0s, d_out1s, d_c0, d_c1, d_keys, ks, count, batch, k_special, alpha, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  return rotate_run(ctx, d_out0s, d_out1s, d_c0, d_c1, d_keys, ks, count, batch, k_special, alpha, flags, (hipStream_t)stream);
}

// The weighted sum of NTT-form automorphisms (kernels_lintrans.hip; include/nflhip.h "weighted sums of automorphisms"): one launch,
// the pointers in the kernel arguments, nothing allocated.
int nflhip_automorphism_mac_dev(nflhip_ctx *ctx, void *d_out, const void *d_addend, const void *const *d_ins, const void *const *d_weights,
                                const uint64_t *ks, size_t terms, size_t batch, size_t rows, int flags, void *stream) {
  int rc = mac_check(ctx, d_out, d_addend, d_ins, d_weights, ks, terms, batch, rows, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_permute_mac_ntt<T>(ctx->shape, ctx->tabs, (T *)d_out, (const T *)d_addend, (const T *const *)d_ins, (const T *const *)d_weights, ks,
                                     (int)terms, batch, rows, 1, 0, 0, (flags & NFLHIP_MAC_DOUBLE_BUFFER) != 0, (hipStream_t)stream);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "automorphism_mac");
  return NFLHIP_OK;
}
// The same for several outputs that share the inputs (kernels_bsgs.hip; include/nflhip.h "weighted sums of automorphisms into several
// outputs"): one launch per kMacMultiJB outputs, the pointers in the kernel arguments, nothing allocated.
int nflhip_automorphism_mac_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const void *const *d_addends, const void *const *d_ins,
                                      const void *const *d_weights, const uint64_t *ks, size_t outputs, size_t terms, size_t batch, size_t rows,
                                      int flags, void *stream) {
  int rc = mac_multi_check(ctx, d_outs, d_addends, d_ins, d_weights, ks, outputs, terms, batch, rows, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_permute_mac_multi_ntt<T>(ctx->shape, ctx->tabs, (T *const *)d_outs, (const T *const *)d_addends, (const T *const *)d_ins,
                                           (const T *const *)d_weights, ks, (int)outputs, (int)terms, batch, rows, 1, 0, 0, (hipStream_t)stream);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "automorphism_mac_multi");
  return NFLHIP_OK;
}

// Slot linear transforms (kernels_lintrans.hip; include/nflhip.h "slot linear transforms"): the key-switch sums of one c1 against up to
// 16 keys, each permuted, multiplied by its plaintext diagonal and added up WHILE STILL ON ALL nm ROWS, then ONE mod-down of the two
// sums; the c0 terms and the unkeyed (k = 1, NULL key) terms are added on the L rows afterwards.  Two plans with the same words:
//   sequence  X = c1 embedded in nm rows, per-digit nflhip_baseconv_ntt_dev into U = [dnum][batch][nm][n]; per keyed (m, c)
//             nflhip_dot_dev into T, nflhip_automorphism_dev into P, nflhip_dot_dev (one term, the addend in place) of P against the
//             weight into A = [2][batch][nm][n]; nflhip_moddown_ntt_dev; per term nflhip_automorphism_dev of c0 and nflhip_dot_dev
//             with the addend in place on the child context over rows [0, L)
//   hoisted   the mod-up as in rotate_run into U; k_dot_multi into S = [2 keyed][batch][nm][n]; k_permute_mac_ntt with
//             blockIdx.y the component into A; one mod-down straight into out0 / out1; k_permute_mac_ntt on L rows, the addend in
//             place, once for out0 (the c0 terms) and once for out1 (the unkeyed terms), where there are any
// Default: hoisted, always.  The starting rule (hoisted from two keyed terms on) did not survive the measurement: with ONE keyed term
// the hoisted plan measured x1.07 - x1.18 against the sequence, well beyond the blocks' spread, and with none it is the one-launch
// primitive against a loop of automorphism + dot (profiles/r16_lintrans.txt).  The sequence is the cross-check.
// kl: ctx is a level context and the keys AND the weights lie in its parent's layout (nflhip_lintrans_level_ntt_dev).  Sequence: the
// key dots through dot_key, the one-term dot against the weight on all rows through the level-key operand too (one term, so the term
// stride is moot; no gather, no copy).  Hoisted: the instances of kernels_level_rotate.hip for k_dot_multi and for the
// k_permute_mac_ntt pass on all rows.  The passes on the kept rows need nothing: rows [0, level) of a parent-layout weight are a prefix.
// Lock order: lt_mu, then ks_mu, then bcn_mu.
static int lintrans_run(nflhip_ctx *ctx, void *out0, void *out1, const void *c0, const void *c1, const void *const *keys, const void *const *weights,
                        const uint64_t *ks, size_t count, size_t batch, size_t K, size_t alpha, int flags, hipStream_t st,
                        const KeyLevel *kl = nullptr) {
  std::lock_guard<std::mutex> lk(ctx->lt_mu);
  const size_t nm = ctx->shape.nm, L = nm - K, dnum = (L + alpha - 1) / alpha, row = ctx->shape.n * ctx->word, pb = nm * row, qb = L * row;
  const bool centred = (flags & NFLHIP_LINTRANS_CENTERED) != 0, floor = (flags & NFLHIP_LINTRANS_FLOOR) != 0, cap = is_capturing(st);
  const uint64_t *const *recs = nullptr;
  int rc;
  {  // the tables first: a repeated modulus is refused with the builder's message before anything is enqueued
    std::lock_guard<std::mutex> l2(ctx->ks_mu);
    rc = keyswitch_records(ctx, K, alpha, st, &recs);
  }
  if (rc) return rc;
  // the keyed terms, in order; the rest are the unrotated diagonals
  const void *kkeys[NFLHIP_LINTRANS_MAX_TERMS], *kw[NFLHIP_LINTRANS_MAX_TERMS], *uw[NFLHIP_LINTRANS_MAX_TERMS], *uin[NFLHIP_LINTRANS_MAX_TERMS],
      *cin[NFLHIP_LINTRANS_MAX_TERMS];
  uint64_t kks[NFLHIP_LINTRANS_MAX_TERMS], uks[NFLHIP_LINTRANS_MAX_TERMS];
  size_t keyed = 0, unkeyed = 0;
  for (size_t m = 0; m < count; ++m) {
    cin[m] = c0;
    if (keys[m]) {
      kkeys[keyed] = keys[m];
      kw[keyed] = weights[m];
      kks[keyed++] = ks[m];
    } else {
      uw[unkeyed] = weights[m];
      uin[unkeyed] = c1;
      uks[unkeyed++] = 1;
    }
  }
  int plan = flags & (NFLHIP_LINTRANS_SEQUENCE | NFLHIP_LINTRANS_HOISTED);
  if (!plan) plan = NFLHIP_LINTRANS_HOISTED;
  const int modes = flags & (NFLHIP_LINTRANS_CENTERED | NFLHIP_LINTRANS_FLOOR);
  const size_t down = !keyed ? 0 : moddown_pair_adjacent(ctx, out0, out1, batch, K) ? 2 * batch : batch;  // the polynomials of one mod-down call
  // what a call while capturing may do: repeat a (k_special, alpha, plan, modes) already served at this batch, keyed * batch and mod-down or larger
  const std::array<size_t, 3> wkey = {K, alpha, (size_t)(plan | modes)}, wsizes = {batch, keyed * batch, down};
  if (cap && !warm_covers(ctx->lt_warm, wkey, wsizes))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "lintrans: the first call for a (k_special, alpha, plan), or for a larger batch, allocates, which a stream capture cannot do");
  const bool seq = plan == NFLHIP_LINTRANS_SEQUENCE;
  const ModupRoute route = seq ? kModupPerDigit : modup_default_route(ctx);
  // sequence: X, U, T, P, A and the permuted c0 on L rows; hoisted: X, U, S, A
  const size_t xb = keyed ? modup_x_bytes(ctx, route, batch, L) : 0, ub = keyed ? batch * dnum * pb : 0;
  const size_t sb = !keyed ? 0 : seq ? 2 * batch * pb : 2 * keyed * batch * pb, ab = keyed ? 2 * batch * pb : 0, tb = seq && c0 ? batch * qb : 0;
  if ((rc = set_device(ctx))) return rc;
  nflhip_ctx *child = nullptr;
  if ((rc = kept_rows_child(ctx, L, cap, &child)) || (rc = ws_begin(ctx, ctx->lt_ws, xb + ub + sb + ab + tb, cap, st, "lintrans: the"))) return rc;
  char *X = (char *)ctx->lt_ws.buf, *U = X + xb, *S = U + ub, *A = S + sb, *T0 = A + ab;
  const size_t pw = pb / ctx->word;  // words of a polynomial of nm rows
  if (keyed) {
    nflhip_dot_operand a;  // the digits
    if ((rc = modup_copy_in(ctx, route, X, c1, batch, L, st))) return rc;
    if ((rc = modup_run(ctx, child, route, U, X, recs, batch, L, alpha, centred, "lintrans", st, &a))) return rc;
    if (seq) {
      char *T = S, *P = S + batch * pb;
      const nflhip_dot_operand pa = {P, 1, 0};
      for (size_t m = 0; m < keyed; ++m)
        for (size_t c = 0; c < 2; ++c) {
          char *Ac = A + c * batch * pb;
          if ((rc = dot_key(ctx, T, &a, kkeys[m], c, nullptr, batch, dnum, kl, st))) return rc;
          if ((rc = nflhip_automorphism_dev(ctx, P, T, batch, kks[m], NFLHIP_FORM_NTT, st))) return rc;
          if (kl) {  // the diagonal lies in the parent's layout as a key component does: the level-key operand, one term
            if ((rc = dot_key(ctx, Ac, &pa, kw[m], 0, m ? Ac : nullptr, batch, 1, kl, st))) return rc;
          } else {
            const nflhip_dot_operand w = {kw[m], 0, 0};
            if ((rc = nflhip_dot_dev(ctx, Ac, &pa, &w, m ? Ac : nullptr, batch, 1, 0, st))) return rc;
          }
        }
    } else {
      void *douts[2 * NFLHIP_LINTRANS_MAX_TERMS];
      const void *dbs[2 * NFLHIP_LINTRANS_MAX_TERMS], *mins[NFLHIP_LINTRANS_MAX_TERMS];
      for (size_t m = 0; m < keyed; ++m) {
        for (size_t c = 0; c < 2; ++c) {
          douts[2 * m + c] = S + (2 * m + c) * batch * pb;
          dbs[2 * m + c] = (const char *)kkeys[m] + c * (kl ? kl->knm * row : pb);
        }
        mins[m] = douts[2 * m];  // component c of term m lies c batch polynomials behind
      }
      hipError_t e = with_limb(ctx, [&](auto z) {
        typedef decltype(z) T;
        hipError_t r = kl ? launch_dot_multi_level<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, a.group_stride, a.term_stride,
                                                      (const T *const *)dbs, 2 * keyed, batch, dnum, 1, *kl, st)
                          : launch_dot_multi<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, a.group_stride, a.term_stride,
                                                (const T *const *)dbs, 2, 2 * keyed, batch, dnum, 1, st);
        if (r != hipSuccess) return r;
        if (kl)  // (the passes on the kept rows below need nothing: rows [0, level) of a parent-layout diagonal are a prefix)
          return launch_permute_mac_ntt_level<T>(ctx->shape, ctx->tabs, (T *)A, nullptr, (const T *const *)mins, (const T *const *)kw, kks, (int)keyed,
                                                 batch, 2, batch * pw, batch * pw, *kl, st);
        return launch_permute_mac_ntt<T>(ctx->shape, ctx->tabs, (T *)A, nullptr, (const T *const *)mins, (const T *const *)kw, kks, (int)keyed, batch,
                                         nm, 2, batch * pw, batch * pw, 0, st);
      });
      if (e != hipSuccess) return hipfail(ctx, e, "lintrans: inner products and weighted sum");
    }
    if ((rc = moddown_pair(ctx, out0, out1, A, batch, K, floor, st))) return rc;
  }
  // the terms on L rows: every diagonal against sigma(c0) into out0, the unrotated unkeyed ones against c1 into out1
  if (!keyed && !c0) HIPCHK(ctx, hipMemsetAsync(out0, 0, batch * qb, st));  // (out1 has a term: with no keyed one, every term is unkeyed)
  if (seq) {
    for (size_t m = 0; m < count && c0; ++m) {
      const nflhip_dot_operand a = {T0, 1, 0}, w = {weights[m], 0, 0};
      if ((rc = nflhip_automorphism_dev(child, T0, c0, batch, ks[m], NFLHIP_FORM_NTT, st))) return rc;
      if ((rc = nflhip_dot_dev(child, out0, &a, &w, keyed || m ? out0 : nullptr, batch, 1, 0, st))) return rc;
    }
    for (size_t m = 0; m < unkeyed; ++m) {
      const nflhip_dot_operand a = {c1, 1, 0}, w = {uw[m], 0, 0};
      if ((rc = nflhip_dot_dev(child, out1, &a, &w, keyed || m ? out1 : nullptr, batch, 1, 0, st))) return rc;
    }
    if ((rc = set_device(ctx))) return rc;
  } else {
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      hipError_t r = hipSuccess;
      if (c0)
        r = launch_permute_mac_ntt<T>(ctx->shape, ctx->tabs, (T *)out0, keyed ? (const T *)out0 : nullptr, (const T *const *)cin, (const T *const *)weights,
                                      ks, (int)count, batch, L, 1, 0, 0, 0, st);
      if (r == hipSuccess && unkeyed)
        r = launch_permute_mac_ntt<T>(ctx->shape, ctx->tabs, (T *)out1, keyed ? (const T *)out1 : nullptr, (const T *const *)uin, (const T *const *)uw, uks,
                                      (int)unkeyed, batch, L, 1, 0, 0, 0, st);
      return r;
    });
    if (e != hipSuccess) return hipfail(ctx, e, "lintrans: the terms on the kept rows");
  }
  if ((rc = ws_end(ctx, ctx->lt_ws, cap, st))) return rc;
  if (!cap) warm_note(ctx->lt_warm, wkey, wsizes);
  return NFLHIP_OK;
}
int nflhip_lintrans_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_keys,
                            const void *const *d_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags,
                            void *stream) {
  int rc = lintrans_check(ctx, d_out0, d_out1, d_c0, d_c1, d_keys, d_weights, ks, count, batch, k_special, alpha, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  return lintrans_run(ctx, d_out0, d_out1, d_c0, d_c1, d_keys, d_weights, ks, count, batch, k_special, alpha, flags, (hipStream_t)stream);
}

// The tensor product of two degree-1 ciphertexts (kernels_mulrelin.hip; include/nflhip.h "ciphertext multiplication"): one launch,
// nothing allocated.
int nflhip_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1, const void *d_b0,
                          const void *d_b1, size_t batch, size_t rows, int flags, void *stream) {
  int rc = tensor_check(ctx, d_out0, d_out1, d_out2, d_a0, d_a1, d_b0, d_b1, batch, rows, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_tensor_ntt<T>(ctx->shape, ctx->tabs, (T *)d_out0, (T *)d_out1, (T *)d_out2, (const T *)d_a0, (const T *)d_a1, (const T *)d_b0,
                                (const T *)d_b1, batch, rows, rows, rows * ctx->shape.n, rows * ctx->shape.n, nullptr, (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "tensor");
}

// RNS scale-and-round by t/Q (kernels_scale_round.hip; include/nflhip.h "BFV multiplication").  The record of a (ks, t)
// (host_tables.cpp build_scale_round_record) is built and uploaded by the first call that names it, under the rules of
// baseconv_record.
static int scale_round_record(nflhip_ctx *ctx, size_t ks, uint64_t t, hipStream_t st, const uint64_t **rec) {
  std::lock_guard<std::mutex> lk(ctx->srec_mu);
  const std::array<uint64_t, 2> key = {(uint64_t)ks, t};
  auto it = ctx->srec.find(key);
  if (it != ctx->srec.end()) {
    *rec = (const uint64_t *)it->second;
    return NFLHIP_OK;
  }
  std::vector<uint64_t> h;
  std::string err;
  int rc;
  try {
    rc = build_scale_round_record(ctx->shape.limb_bits, ctx->h_P, ks, t, &h, &err);
  } catch (const std::bad_alloc &) {
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory while building the scale-round tables");
  }
  if (rc) return fail(ctx, rc, err);  // (host arithmetic only: a repeated modulus is refused before any device use)
  if (is_capturing(st))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "scale_round: the first call for a (ks, t) uploads its tables, which a stream capture cannot do");
  if ((rc = set_device(ctx))) return rc;
  void *d = nullptr;
  HIPCHK(ctx, hipMalloc(&d, h.size() * sizeof(uint64_t)));
  hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hipfail(ctx, e, "scale_round: table upload");
  }
  try {
    ctx->srec[key] = d;
  } catch (const std::bad_alloc &) {
    (void)hipFree(d);
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  }
  *rec = (const uint64_t *)d;
  return NFLHIP_OK;
}
// Plans of the coefficient form: the one-pass kernel where its register plans hold the rows; two passes -- Y into workspace 1, then
// k_baseconv from there with the second record -- for larger shapes and under NFLHIP_SCALE_ROUND_TWO_PASS.  KEEP is one pass always.
// The NTT form composes around it as baseconv_ntt_composed does: the input copied into workspace 0 and inverse-transformed by this
// context, the result forward-transformed by the child context over the rows written.
static int scale_round_run(nflhip_ctx *ctx, void *out, const void *in, size_t batch, size_t ks, uint64_t t, int flags, bool ntt, hipStream_t st) {
  if (batch == 0) return NFLHIP_OK;  // (touches nothing: no record is built for an empty batch)
  const uint64_t *rec = nullptr;
  int rc = scale_round_record(ctx, ks, t, st, &rec);
  if (rc || (rc = set_device(ctx))) return rc;
  const size_t nm = ctx->shape.nm, kd = nm - ks, row = ctx->shape.n * ctx->word;
  const bool centred = !(flags & NFLHIP_SCALE_ROUND_FLOOR), keep = (flags & NFLHIP_SCALE_ROUND_KEEP) != 0, regs = scale_round_in_registers(ks, kd);
  const bool two = !keep && (!regs || (flags & NFLHIP_SCALE_ROUND_TWO_PASS));
  auto pass = [&](void *o, const void *i, bool kp) {
    return with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_scale_round<T>(ctx->shape, ctx->tabs, (T *)o, (const T *)i, rec, batch, ks, centred, kp, !regs, st);
    });
  };
  hipError_t e;
  if (!ntt && !two) {  // one launch, nothing allocated
    e = pass(out, in, keep);
    return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "scale_round");
  }
  std::lock_guard<std::mutex> lk(ctx->sr_mu);
  const bool cap = is_capturing(st);
  const char *what = "scale_round: the";
  nflhip_ctx *child = nullptr;
  if (ntt) {
    std::lock_guard<std::mutex> lc(ctx->bcn_mu);
    if ((rc = keep ? bcn_child(ctx, ks, kd, cap, &child) : bcn_child(ctx, 0, ks, cap, &child))) return rc;
  }
  if ((rc = set_device(ctx))) return rc;
  if (two && (rc = ws_grow(ctx, ctx->sr_ws[1], batch * kd * row, cap, what))) return rc;
  if ((rc = ws_begin(ctx, ctx->sr_ws[0], ntt ? batch * nm * row : 0, cap, st, what))) return rc;
  const void *src = in;
  if (ntt) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->sr_ws[0].buf, in, batch * nm * row, hipMemcpyDefault, st));
    if ((rc = nflhip_ntt_inv_dev(ctx, ctx->sr_ws[0].buf, batch, st)) || (rc = set_device(ctx))) return rc;
    src = ctx->sr_ws[0].buf;
  }
  if (two) {
    void *Y = ctx->sr_ws[1].buf;
    if ((e = pass(Y, src, true)) != hipSuccess) return hipfail(ctx, e, "scale_round: first pass");
    e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_baseconv_rows<T>(ctx->shape, ctx->tabs, (T *)out, ks, (const T *)Y, kd, rec + scale_round_back_offset(ks, kd), batch, kd, 0, ks, 1, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, "scale_round: second pass");
  } else if ((e = pass(out, src, keep)) != hipSuccess) {
    return hipfail(ctx, e, "scale_round");
  }
  if (ntt && ((rc = nflhip_ntt_fwd_dev(child, out, batch, st)) || (rc = set_device(ctx)))) return rc;
  return ws_end(ctx, ctx->sr_ws[0], cap, st);
}
int nflhip_scale_round_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  int rc = scale_round_check(ctx, d_out, d_in, batch, ks, t, flags, nullptr);  // in full, before any device use
  if (rc) return rc;
  return scale_round_run(ctx, d_out, d_in, batch, ks, t, flags, false, (hipStream_t)stream);
}
int nflhip_scale_round_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  int rc = scale_round_check(ctx, d_out, d_in, batch, ks, t, flags, nullptr);  // in full, before any device use
  if (rc) return rc;
  return scale_round_run(ctx, d_out, d_in, batch, ks, t, flags, true, (hipStream_t)stream);
}

// The scale-invariant tensor product of BFV (include/nflhip.h "BFV multiplication"), the four steps of its definition through the
// entries above: the inputs embedded in E = [4 or 2][batch][nm][n] and base-extended as ONE batch in place; the tensor product into
// T = [3][batch][nm][n]; the scale-round of T as ONE batch of 3 batch, straight into the outputs where they follow each other in
// memory, else into R = [3][batch][L][n] and copied out.  Both records are built BEFORE anything is enqueued; every read of the
// inputs precedes every write of an output, so an output may be an input.
int nflhip_bfv_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1, const void *d_b0,
                              const void *d_b1, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  int rc = bfv_tensor_check(ctx, d_out0, d_out1, d_out2, d_a0, d_a1, d_b0, d_b1, batch, ks, t, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *rec = nullptr;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, pb = nm * row, ob = batch * ks * row, nin = d_b0 ? 4 : 2;
  if ((rc = scale_round_record(ctx, ks, t, st, &rec)) || (rc = baseconv_record(ctx, 0, ks, 0, nm, false, st, &rec)) || (rc = set_device(ctx))) return rc;
  std::lock_guard<std::mutex> lk(ctx->bfv_mu);
  const bool cap = is_capturing(st), dense = (char *)d_out1 == (char *)d_out0 + ob && (char *)d_out2 == (char *)d_out1 + ob;
  if ((rc = ws_begin(ctx, ctx->bfv_ws, (nin + 3) * batch * pb + (dense ? 0 : 3 * ob), cap, st, "bfv_tensor: the"))) return rc;
  char *E = (char *)ctx->bfv_ws.buf, *T = E + nin * batch * pb, *R = dense ? (char *)d_out0 : T + 3 * batch * pb;
  const void *const ins[4] = {d_a0, d_a1, d_b0, d_b1};
  for (size_t k = 0; k < nin; ++k)
    HIPCHK(ctx, hipMemcpy2DAsync(E + k * batch * pb, pb, ins[k], ks * row, ks * row, batch, hipMemcpyDefault, st));  // (a caller's buffer may be pinned host memory)
  if ((rc = nflhip_baseconv_ntt_dev(ctx, E, E, nin * batch, 0, ks, 0, nm, NFLHIP_BASECONV_CENTERED, st))) return rc;
  if ((rc = nflhip_tensor_ntt_dev(ctx, T, T + batch * pb, T + 2 * batch * pb, E, E + batch * pb, d_b0 ? E + 2 * batch * pb : nullptr,
                                  d_b0 ? E + 3 * batch * pb : nullptr, batch, nm, 0, st)))
    return rc;
  if ((rc = scale_round_run(ctx, R, T, 3 * batch, ks, t, flags, true, st)) || (rc = set_device(ctx))) return rc;
  if (!dense) {
    void *const outs[3] = {d_out0, d_out1, d_out2};
    for (size_t k = 0; k < 3; ++k) HIPCHK(ctx, hipMemcpyAsync(outs[k], R + k * ob, ob, hipMemcpyDefault, st));
  }
  return ws_end(ctx, ctx->bfv_ws, cap, st);
}

// Ciphertext multiplication with relinearisation (kernels_mulrelin.hip; include/nflhip.h "ciphertext multiplication"): the tensor
// product d0, d1, d2 on the L kept rows, the key-switch sums of d2 with pi (.) d_c as their addend, one mod-down by the last K
// (RESCALE: K + 1) moduli.  Three plans with the same words:
//   sequence  existing entries only: a, b copied into S = [a0 a1 | b1 b0] = [4][batch][L][n]; nflhip_dot_dev on the child context over
//             rows [0, L) into D = [3][batch][L][n] (one term for d0 and d2, two for d1); D embedded into X = [3][batch][nm][n] (zeroed
//             first); A_c = X_c (.) C by a one-term nflhip_dot_dev, C the constant polynomial of pi; per-digit nflhip_baseconv_ntt_dev
//             from X_2 into U = [dnum][batch][nm][n]; nflhip_dot_dev into A_c with A_c as the addend
//   merged    k_tensor_ntt once: d2 into X (embedded in nm rows for the per-digit route, else L rows dense), pi d_c into A; the mod-up
//             as in rotate_run; nflhip_dot_dev into A_c with A_c as the addend
//   fused     k_tensor_modup_dot_fused straight from the inputs to A; bounded as the key switch's one-launch kernel
// then nflhip_moddown_ntt_dev -- one call of 2 batch polynomials when out1 follows out0 in memory, else one per output.  Every read
// of a and b is enqueued before the mod-down, so an output may be an input.
// Default: see mulrelin_default_plan.  Lock order: mr_mu, then ks_mu, then bcn_mu.
static int mulrelin_pi(nflhip_ctx *ctx, size_t K, hipStream_t st, const uint64_t **pi, const void **cpoly) {  // under mr_mu
  const size_t nm = ctx->shape.nm, L = nm - K, n = ctx->shape.n, head = 2 * nm * sizeof(uint64_t);
  auto it = ctx->mr_pi.find(K);
  if (it == ctx->mr_pi.end()) {
    if (is_capturing(st))
      return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "mulrelin: the first call for a k_special uploads its tables, which a stream capture cannot do");
    const int W = ctx->shape.limb_bits;
    std::vector<uint64_t> h(2 * nm + (nm * n * ctx->word + 7) / 8, 0);
    for (size_t j = 0; j < L; ++j) {
      const uint64_t p = ctx->h_P[j];
      unsigned __int128 v = 1;
      for (size_t k = L; k < nm; ++k) v = v * (ctx->h_P[k] % p) % p;
      h[2 * j] = (uint64_t)v;
      h[2 * j + 1] = (uint64_t)((v << W) / p);  // floor(pi 2^W / p), pi < p < 2^(W-2)
      with_limb(ctx, [&](auto z) {
        typedef decltype(z) T;
        T *row = reinterpret_cast<T *>(h.data() + 2 * nm) + j * n;
        for (size_t i = 0; i < n; ++i) row[i] = (T)v;
        return 0;
      });
    }
    int rc = set_device(ctx);
    if (rc) return rc;
    void *d = nullptr;
    HIPCHK(ctx, hipMalloc(&d, h.size() * sizeof(uint64_t)));
    hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hipfail(ctx, e, "mulrelin: table upload");
    }
    try {
      it = ctx->mr_pi.emplace(K, d).first;
    } catch (const std::bad_alloc &) {
      (void)hipFree(d);
      return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
    }
  }
  *pi = (const uint64_t *)it->second;
  *cpoly = (const char *)it->second + head;
  return NFLHIP_OK;
}
// Which plan serves by default.  The starting rule: the one-launch kernel where it fits (not for contexts created under
// NFLHIP_VARIANT=hipcc), the merged plan otherwise.
static int mulrelin_default_plan(const nflhip_ctx *ctx, size_t L, size_t dnum, bool centred) {
  if (!ctx->shape.compiled_only && keyswitch_fused_fits(L, dnum, ctx->shape.n, ctx->word, centred)) return NFLHIP_MULRELIN_FUSED;
  return NFLHIP_MULRELIN_MERGED;
}
// The sum over terms: the merged plan; the one-launch kernel is not built for it.
static int mulrelin_dot_default_plan() { return NFLHIP_MULRELIN_MERGED; }
// `dot`: the sum over terms (include/nflhip.h "sums of ciphertext products") -- the tensor stage forms (D0, D1, D2) from the four
// operands (strides in polynomials of L rows; b0.ptr == nullptr: the squares), a0 .. b1 are not read and `batch` is the groups.
struct MrDot {
  nflhip_dot_operand a0, a1, b0, b1;
  size_t terms;
};
static TensorDotOperand tensor_dot_operand(const nflhip_dot_operand *x) {  // (the launcher's own type: kernels.h does not see nflhip.h)
  return x ? TensorDotOperand{x->ptr, x->group_stride, x->term_stride} : TensorDotOperand{nullptr, 0, 0};
}
static int mulrelin_run(nflhip_ctx *ctx, void *out0, void *out1, const void *a0, const void *a1, const void *b0, const void *b1, const void *key,
                        size_t batch, size_t K, size_t alpha, int flags, hipStream_t st, const KeyLevel *kl = nullptr, const MrDot *dot = nullptr) {
  std::lock_guard<std::mutex> lk(ctx->mr_mu);
  const size_t nm = ctx->shape.nm, n = ctx->shape.n, L = nm - K, dnum = (L + alpha - 1) / alpha, row = n * ctx->word, pb = nm * row, qb = L * row;
  const bool centred = (flags & NFLHIP_MULRELIN_CENTERED) != 0, floor = (flags & NFLHIP_MULRELIN_FLOOR) != 0;
  const bool resc = (flags & NFLHIP_MULRELIN_RESCALE) != 0, cap = is_capturing(st);
  const size_t down = K + (resc ? 1 : 0), kept = nm - down;
  const uint64_t *const *recs = nullptr;
  const uint64_t *pi = nullptr, *drec = nullptr;
  const void *cpoly = nullptr;
  int rc;
  {  // the tables first: a repeated modulus is refused with the builder's message before anything is enqueued
    std::lock_guard<std::mutex> l2(ctx->ks_mu);
    rc = keyswitch_records(ctx, K, alpha, st, &recs);
  }
  // the mod-down by K + 1 rows: its record is built HERE only so that a repeated modulus is refused before anything is enqueued; the
  // mod-down entry below looks it up again itself
  if (!rc && resc) rc = baseconv_record(ctx, kept, down, 0, kept, true, st, &drec);
  (void)drec;
  if (rc) return rc;
  try {
    rc = mulrelin_pi(ctx, K, st, &pi, &cpoly);
  } catch (const std::bad_alloc &) {
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  }
  if (rc) return rc;
  int plan = flags & (NFLHIP_MULRELIN_SEQUENCE | NFLHIP_MULRELIN_MERGED | NFLHIP_MULRELIN_FUSED);
  if (plan == NFLHIP_MULRELIN_FUSED && !keyswitch_fused_fits(L, dnum, n, ctx->word, centred))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "mulrelin: the rows of this call do not fit the one-launch kernel's LDS");
  if (dot && plan == NFLHIP_MULRELIN_FUSED)
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "mulrelin_dot: the one-launch kernel serves one product (terms == 1, dense operands)");
  if (!plan) plan = dot ? mulrelin_dot_default_plan() : mulrelin_default_plan(ctx, L, dnum, centred);
  const int modes = flags & (NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_FLOOR | NFLHIP_MULRELIN_RESCALE);
  // what a call while capturing may do: repeat a (k_special, alpha, plan, modes) already served at this batch or a larger one
  const std::array<size_t, 3> wkey = {K, alpha, (size_t)(plan | modes)}, wsizes = {batch, 0, 0};
  if (cap && !warm_covers(ctx->mr_warm, wkey, wsizes))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "mulrelin: the first call for a (k_special, alpha, plan), or for a larger batch, allocates, which a stream capture cannot do");
  const bool seq = plan == NFLHIP_MULRELIN_SEQUENCE, fused = plan == NFLHIP_MULRELIN_FUSED;
  const ModupRoute route = seq ? kModupPerDigit : modup_default_route(ctx);
  // sequence: S, D, X, U, A; merged: X, U, A; fused: A
  const size_t sb = seq ? 7 * batch * qb : 0, xb = fused ? 0 : seq ? 3 * batch * pb : modup_x_bytes(ctx, route, batch, L);
  const size_t ub = fused ? 0 : batch * dnum * pb, ab = 2 * batch * pb;
  if ((rc = set_device(ctx))) return rc;
  nflhip_ctx *child = nullptr;
  // (the L-row context: the sequence's tensor product, the merged plan's inverse transform)
  if (!fused && (rc = kept_rows_child(ctx, L, cap, &child))) return rc;
  if ((rc = ws_begin(ctx, ctx->mr_ws, sb + xb + ub + ab, cap, st, "mulrelin: the"))) return rc;
  char *S = (char *)ctx->mr_ws.buf, *X = S + sb, *U = X + xb, *A = U + ub;
  nflhip_dot_operand u = {nullptr, 0, 0};
  if (fused) {
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      if (kl) return launch_tensor_modup_dot_fused_level<T>(ctx->shape, ctx->tabs, (T *)A, (const T *)a0, (const T *)a1, (const T *)b0, (const T *)b1,
                                                            (const T *)key, recs, pi, batch, L, alpha, centred, *kl, st);
      return launch_tensor_modup_dot_fused<T>(ctx->shape, ctx->tabs, (T *)A, (const T *)a0, (const T *)a1, (const T *)b0, (const T *)b1, (const T *)key,
                                              recs, pi, batch, L, alpha, centred, st);
    });
    if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "mulrelin: the rows of this call do not fit the one-launch kernel's LDS");
    if (e != hipSuccess) return hipfail(ctx, e, "mulrelin (fused)");
  } else if (seq) {
    char *D = S + 4 * batch * qb, *X2 = X + 2 * batch * pb;
    if (dot) {  // D straight from the operands, four sums of products on the kept rows (the squares: b is a, D1 = 2 sum a0 a1)
      const nflhip_dot_operand *y0 = dot->b0.ptr ? &dot->b0 : &dot->a0, *y1 = dot->b0.ptr ? &dot->b1 : &dot->a1;
      if ((rc = nflhip_dot_dev(child, D, &dot->a0, y0, nullptr, batch, dot->terms, 0, st))) return rc;
      if ((rc = nflhip_dot_dev(child, D + batch * qb, &dot->a0, y1, nullptr, batch, dot->terms, 0, st))) return rc;
      if ((rc = nflhip_dot_dev(child, D + batch * qb, &dot->a1, y0, D + batch * qb, batch, dot->terms, 0, st))) return rc;
      if ((rc = nflhip_dot_dev(child, D + 2 * batch * qb, &dot->a1, y1, nullptr, batch, dot->terms, 0, st))) return rc;
    } else {
      const void *const src[4] = {a0, a1, b1 ? b1 : a1, b0 ? b0 : a0};  // S = [a0 a1 | b1 b0]: d1 = a0 b1 + a1 b0 term by term
      for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipMemcpyAsync(S + k * batch * qb, src[k], batch * qb, hipMemcpyDefault, st));  // (a staged caller's inputs may be pinned host memory)
      const nflhip_dot_operand sa0 = {S, 1, batch}, sa1 = {S + batch * qb, 1, batch}, sb1 = {S + 2 * batch * qb, 1, batch}, sb0 = {S + 3 * batch * qb, 1, batch};
      if ((rc = nflhip_dot_dev(child, D, &sa0, &sb0, nullptr, batch, 1, 0, st))) return rc;
      if ((rc = nflhip_dot_dev(child, D + batch * qb, &sa0, &sb1, nullptr, batch, 2, 0, st))) return rc;
      if ((rc = nflhip_dot_dev(child, D + 2 * batch * qb, &sa1, &sb1, nullptr, batch, 1, 0, st))) return rc;
    }
    if ((rc = set_device(ctx))) return rc;
    HIPCHK(ctx, hipMemsetAsync(X, 0, 3 * batch * pb, st));
    HIPCHK(ctx, hipMemcpy2DAsync(X, pb, D, qb, qb, 3 * batch, hipMemcpyDeviceToDevice, st));
    const nflhip_dot_operand c = {cpoly, 0, 0};
    for (size_t k = 0; k < 2; ++k) {
      const nflhip_dot_operand x = {X + k * batch * pb, 1, 0};
      if ((rc = nflhip_dot_dev(ctx, A + k * batch * pb, &x, &c, nullptr, batch, 1, 0, st))) return rc;
    }
    if ((rc = modup_run(ctx, child, route, U, X2, recs, batch, L, alpha, centred, "mulrelin", st, &u))) return rc;
  } else {
    const size_t pw = pb / ctx->word, qw = qb / ctx->word;
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      if (dot) {
        const TensorDotOperand o[4] = {tensor_dot_operand(&dot->a0), tensor_dot_operand(&dot->a1), tensor_dot_operand(&dot->b0), tensor_dot_operand(&dot->b1)};
        return launch_tensor_dot_ntt<T>(ctx->shape, ctx->tabs, (T *)A, (T *)(A + batch * pb), (T *)X, &o[0], &o[1], o[2].ptr ? &o[2] : nullptr,
                                        o[2].ptr ? &o[3] : nullptr, batch, dot->terms, L, nm, pw, route == kModupPerDigit ? pw : qw, pi, st);
      }
      return launch_tensor_ntt<T>(ctx->shape, ctx->tabs, (T *)A, (T *)(A + batch * pb), (T *)X, (const T *)a0, (const T *)a1, (const T *)b0, (const T *)b1,
                                  batch, L, nm, pw, route == kModupPerDigit ? pw : qw, pi, st);
    });
    if (e != hipSuccess) return hipfail(ctx, e, "mulrelin: tensor");
    if ((rc = modup_run(ctx, child, route, U, X, recs, batch, L, alpha, centred, "mulrelin", st, &u))) return rc;  // (no copy-in: the tensor wrote X)
  }
  for (size_t c = 0; c < 2 && !fused; ++c)
    if ((rc = dot_key(ctx, A + c * batch * pb, &u, key, c, A + c * batch * pb, batch, dnum, kl, st))) return rc;
  if ((rc = moddown_pair(ctx, out0, out1, A, batch, down, floor, st)) || (rc = ws_end(ctx, ctx->mr_ws, cap, st))) return rc;
  if (!cap) warm_note(ctx->mr_warm, wkey, wsizes);
  return NFLHIP_OK;
}
int nflhip_mulrelin_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1,
                            const void *d_key, size_t batch, size_t k_special, size_t alpha, int flags, void *stream) {
  int rc = mulrelin_check(ctx, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_key, batch, k_special, alpha, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  return mulrelin_run(ctx, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_key, batch, k_special, alpha, flags, (hipStream_t)stream);
}


// The two at a level (include/nflhip.h "leveled key switching"): by definition the entries above on the level context with the live
// rows and digits of the key.  level == L forwards.  Below it the digits are those of min(alpha, level): one short digit when alpha
// exceeds the level.
size_t nflhip_keyswitch_level_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha, size_t level) {
  return keyswitch_level_digits(ctx, k_special, alpha, level);
}
// where a call at `level` runs: on the context itself at the top (the key is in its layout: *kl is not for use), else on the level
// context with the key's KeyLevel
static int level_context(nflhip_ctx *ctx, size_t K, size_t level, hipStream_t st, nflhip_ctx **run, KeyLevel *kl) {
  const size_t nm = ctx->shape.nm, L = nm - K;
  *run = ctx;
  *kl = {nm, level, L - level};
  if (level == L) return NFLHIP_OK;
  int rc = set_device(ctx);
  return rc ? rc : level_child(ctx, K, level, is_capturing(st), run);
}
int nflhip_keyswitch_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch, size_t k_special,
                                   size_t alpha, size_t level, int flags, void *stream) {
  int rc = level_check(ctx, k_special, level, "keyswitch");  // in full, before any device use
  if (!rc) rc = keyswitch_check(ctx, d_out0, d_out1, d_in, d_key, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  return keyswitch_run(run, d_out0, d_out1, d_in, d_key, batch, k_special, std::min(alpha, level), flags, (hipStream_t)stream, run == ctx ? nullptr : &kl);
}
int nflhip_mulrelin_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1,
                                  const void *d_key, size_t batch, size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  int rc = level_check(ctx, k_special, level, "mulrelin");  // in full, before any device use
  if (!rc) rc = mulrelin_check(ctx, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_key, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  return mulrelin_run(run, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_key, batch, k_special, std::min(alpha, level), flags, (hipStream_t)stream,
                      run == ctx ? nullptr : &kl);
}
// Sums of ciphertext products (kernels_tensor_dot.hip; include/nflhip.h "sums of ciphertext products"): the tensor product summed
// over terms in one launch, nothing allocated; and the multiplication over it -- mulrelin_run with the four operands for its tensor
// stage and the groups as its batch, on the level context.  One product of dense operands IS nflhip_mulrelin_level_ntt_dev.
int nflhip_tensor_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                              const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, size_t groups, size_t terms, size_t rows, int flags,
                              void *stream) {
  int rc = tensor_dot_check(ctx, d_out0, d_out1, d_out2, a0, a1, b0, b1, groups, terms, rows, flags);  // in full, before any device use
  if (rc || groups == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const TensorDotOperand o[4] = {tensor_dot_operand(a0), tensor_dot_operand(a1), tensor_dot_operand(b0), tensor_dot_operand(b1)};
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_tensor_dot_ntt<T>(ctx->shape, ctx->tabs, (T *)d_out0, (T *)d_out1, (T *)d_out2, &o[0], &o[1], b0 ? &o[2] : nullptr, b0 ? &o[3] : nullptr,
                                    groups, terms, rows, rows, rows * ctx->shape.n, rows * ctx->shape.n, nullptr, (hipStream_t)stream);
  });
  return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "tensor_dot");
}
int nflhip_mulrelin_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                                const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, const void *d_key, size_t groups, size_t terms,
                                size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  int rc = level_check(ctx, k_special, level, "mulrelin_dot");  // in full, before any device use
  if (!rc) rc = mulrelin_dot_check(ctx, d_out0, d_out1, a0, a1, b0, b1, d_key, groups, terms, k_special, alpha, level, flags);
  if (rc || groups == 0) return rc;
  const auto dense = [groups](const nflhip_dot_operand *x) { return !x || groups == 1 || x->group_stride == 1; };
  if (terms == 1 && dense(a0) && dense(a1) && dense(b0) && dense(b1))
    return nflhip_mulrelin_level_ntt_dev(ctx, d_out0, d_out1, a0->ptr, a1->ptr, b0 ? b0->ptr : nullptr, b1 ? b1->ptr : nullptr, d_key, groups, k_special,
                                         alpha, level, flags, stream);
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  const nflhip_dot_operand none = {nullptr, 0, 0};
  const MrDot dot = {*a0, *a1, b0 ? *b0 : none, b1 ? *b1 : none, terms};
  return mulrelin_run(run, d_out0, d_out1, nullptr, nullptr, nullptr, nullptr, d_key, groups, k_special, std::min(alpha, level), flags, (hipStream_t)stream,
                      run == ctx ? nullptr : &kl, &dot);
}
// Hoisted rotations and linear transforms at a level (kernels_level_rotate.hip; include/nflhip.h "rotations and linear transforms at
// a level"): rotate_run and lintrans_run on the level context, whose records, workspaces, events, warm maps and kept-rows child are
// its own; the Galois keys and the diagonals stay in this context's layout and the KeyLevel travels to the launchers that read them.
int nflhip_rotate_hoisted_level_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                        const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                        size_t level, int flags, void *stream) {
  int rc = level_check(ctx, k_special, level, "rotate");  // in full, before any device use
  if (!rc) rc = rotate_check(ctx, d_out0s, d_out1s, d_c0, d_c1, d_keys, ks, count, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  return rotate_run(run, d_out0s, d_out1s, d_c0, d_c1, d_keys, ks, count, batch, k_special, std::min(alpha, level), flags, (hipStream_t)stream,
                    run == ctx ? nullptr : &kl);
}
int nflhip_lintrans_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_keys,
                                  const void *const *d_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                  size_t level, int flags, void *stream) {
  int rc = level_check(ctx, k_special, level, "lintrans");  // in full, before any device use
  if (!rc) rc = lintrans_check(ctx, d_out0, d_out1, d_c0, d_c1, d_keys, d_weights, ks, count, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  return lintrans_run(run, d_out0, d_out1, d_c0, d_c1, d_keys, d_weights, ks, count, batch, k_special, std::min(alpha, level), flags,
                      (hipStream_t)stream, run == ctx ? nullptr : &kl);
}

// BSGS slot linear transforms (kernels_bsgs.hip; include/nflhip.h "BSGS slot linear transforms", which states the map): n1 baby steps
// whose key-switch sums S are formed ONCE, n2 giant steps whose inner sums V_j are weighted sums of the permuted S on all rows, the
// giant step's key switch on mod-down(V_{j,1}) + W_{j,1}, its permutation accumulated into A on all rows, ONE mod-down of A.  ctx is
// the context the call runs on: the level context below the top, with the keys and the weights in its parent's layout (kl), as
// lintrans_run.  Two plans with the same words:
//   sequence  per giant step, through public entries only: the per-digit mod-up, dot_key, nflhip_automorphism_dev + a one-term dot per
//             (i, c) for V, nflhip_automorphism_mac_dev on the kept rows for W, nflhip_moddown_ntt_dev, nflhip_pointwise_dev for the
//             sums, also Y_c + O_c in the scratch, from where out_c is a device copy (the outputs may have any alignment, which
//             nflhip_pointwise_dev does not serve)
//   hoisted   the mod-up of c1 and k_dot_multi once; giants of one kind (keyed, then unkeyed) in groups of kBsgsGroup:
//             k_permute_mac_multi_ntt into V = [2][cnt][batch] (blockIdx.y the component), one mod-down of V_1 into v = [cnt][batch],
//             k_permute_mac_multi_ntt on the kept rows adds W_{.,1} in place, one modup_run over cnt * batch polynomials, dot_key per
//             (j, c) in place of V (V_{j,0} the addend of T_{j,0}), k_permute_sum_ntt into A; then moddown_pair and the passes on the
//             kept rows: k_permute_mac_multi_ntt on c0 for every W_{j,0}, k_permute_sum_ntt into out0, k_permute_mac_ntt of the unkeyed
//             giants' W_{j,1} into out1
// Default: hoisted.  Lock order: bsgs_mu, then ks_mu, then bcn_mu.
static constexpr size_t kBsgsGroup = 4;
static int bsgs_run(nflhip_ctx *ctx, void *out0, void *out1, const void *c0, const void *c1, const void *const *bkeys, const uint64_t *bks, size_t n1,
                    const void *const *gkeys, const uint64_t *gks, size_t n2, const void *const *weights, size_t batch, size_t K, size_t alpha,
                    int flags, hipStream_t st, const KeyLevel *kl) {
  std::lock_guard<std::mutex> lk(ctx->bsgs_mu);
  const size_t nm = ctx->shape.nm, L = nm - K, dnum = (L + alpha - 1) / alpha, row = ctx->shape.n * ctx->word, pb = nm * row, qb = L * row;
  const size_t pw = pb / ctx->word;  // words of a polynomial of nm rows
  const bool centred = (flags & NFLHIP_BSGS_CENTERED) != 0, floor = (flags & NFLHIP_BSGS_FLOOR) != 0, cap = is_capturing(st);
  const int mdflags = floor ? NFLHIP_MODDOWN_FLOOR : 0;
  const uint64_t *const *recs = nullptr;
  int rc;
  {  // the tables first: a repeated modulus is refused with the builder's message before anything is enqueued
    std::lock_guard<std::mutex> l2(ctx->ks_mu);
    rc = keyswitch_records(ctx, K, alpha, st, &recs);
  }
  if (rc) return rc;
  // the steps by kind, in order
  size_t kbi[NFLHIP_BSGS_MAX_BABY], ubi[NFLHIP_BSGS_MAX_BABY], kgj[NFLHIP_BSGS_MAX_GIANT], ugj[NFLHIP_BSGS_MAX_GIANT];
  size_t kb = 0, ub = 0, kg = 0, ug = 0;
  for (size_t i = 0; i < n1; ++i) (bkeys[i] ? kbi[kb++] : ubi[ub++]) = i;
  for (size_t j = 0; j < n2; ++j) (gkeys[j] ? kgj[kg++] : ugj[ug++]) = j;
  int plan = flags & (NFLHIP_BSGS_SEQUENCE | NFLHIP_BSGS_HOISTED);
  if (!plan) plan = NFLHIP_BSGS_HOISTED;
  const bool seq = plan == NFLHIP_BSGS_SEQUENCE, sums = kb || kg;  // sums: something lives on all rows and is modded down at the end
  // (the sequence adds with nflhip_pointwise_dev, which serves whole 16-byte groups: every scratch region is then 16-byte aligned too)
  if (seq && ((batch * pb) | (batch * qb)) % 16)
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "bsgs: the sequence plan adds element-wise on whole 16-byte groups; this batch of rows this short is served by the hoisted plan");
  const int modes = flags & (NFLHIP_BSGS_CENTERED | NFLHIP_BSGS_FLOOR);
  const size_t G = seq ? 1 : std::min(kBsgsGroup, std::max(kg, kb ? ug : (size_t)0)), Gk = seq ? (kg ? 1 : 0) : std::min(kBsgsGroup, kg);
  const size_t down = !sums ? 0 : seq || moddown_pair_adjacent(ctx, out0, out1, batch, K) ? 2 * batch : batch;
  // what a call while capturing may do: repeat a (k_special, alpha, plan, modes, kinds of steps) already served at these sizes or larger
  const std::array<size_t, 3> wkey = {K, alpha, (size_t)(plan | modes | (kb ? 1 : 0) | (kg ? 2 : 0) | (c0 ? 4 : 0))},
                              wsizes = {batch, std::max(Gk, (size_t)1) * batch, down};
  if (cap && !warm_covers(ctx->bsgs_warm, wkey, wsizes))
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "bsgs: the first call for a (k_special, alpha, level, plan), or for larger sizes, allocates, which a stream capture cannot do");
  const ModupRoute route = seq ? kModupPerDigit : modup_default_route(ctx);
  // the regions, in order: X U S A V v X2 U2 W, then (sequence) P T Pq O0 O1 Y
  const size_t xb = kb ? modup_x_bytes(ctx, route, batch, L) : 0, ub_ = kb ? batch * dnum * pb : 0, sb = 2 * kb * batch * pb;
  const size_t ab = sums ? 2 * batch * pb : 0, vb = kb || !seq ? 2 * G * batch * pb : 0, vq = Gk * batch * qb;
  const size_t x2b = Gk ? modup_x_bytes(ctx, route, Gk * batch, L) : 0, u2b = Gk * batch * dnum * pb, wqb = c0 ? (seq ? 1 : n2) * batch * qb : 0;
  const size_t seqb = seq ? 3 * batch * pb + 5 * batch * qb : 0;
  if ((rc = set_device(ctx))) return rc;
  nflhip_ctx *child = nullptr;
  if ((rc = kept_rows_child(ctx, L, cap, &child)) ||
      (rc = ws_begin(ctx, ctx->bsgs_ws, xb + ub_ + sb + ab + vb + vq + x2b + u2b + wqb + seqb, cap, st, "bsgs: the")))
    return rc;
  char *X = (char *)ctx->bsgs_ws.buf, *U = X + xb, *S = U + ub_, *A = S + sb, *V = A + ab, *v = V + vb, *X2 = v + vq, *U2 = X2 + x2b, *W = U2 + u2b;
  auto wt = [&](size_t j, size_t i) { return weights[j * n1 + i]; };
  nflhip_dot_operand u;  // the digits of c1
  if (kb) {
    if ((rc = modup_copy_in(ctx, route, X, c1, batch, L, st))) return rc;
    if ((rc = modup_run(ctx, child, route, U, X, recs, batch, L, alpha, centred, "bsgs", st, &u))) return rc;
  }
  bool a_init = false, o0_init = false, o1_init = false;
  if (seq) {
    char *P = W + wqb, *T = P + batch * pb, *Pq = T + 2 * batch * pb, *O0 = Pq + batch * qb, *O1 = O0 + batch * qb, *Y = O1 + batch * qb;
    const void *cin[NFLHIP_BSGS_MAX_BABY], *cw[NFLHIP_BSGS_MAX_BABY];
    uint64_t cks[NFLHIP_BSGS_MAX_BABY];
    for (size_t m = 0; m < kb; ++m)
      for (size_t c = 0; c < 2; ++c)
        if ((rc = dot_key(ctx, S + (2 * m + c) * batch * pb, &u, bkeys[kbi[m]], c, nullptr, batch, dnum, kl, st))) return rc;
    // acc = x the first time (the automorphism with k = 1), acc += x after it; on ctx (nm rows) or child (L rows).  Scratch regions are
    // whole rows from a hipMalloc base, so 16-byte aligned: what nflhip_pointwise_dev serves
    auto accumulate = [&](nflhip_ctx *on, void *acc, const void *x, bool first) {
      return first ? nflhip_automorphism_dev(on, acc, x, batch, 1, NFLHIP_FORM_NTT, st) : nflhip_pointwise_dev(on, NFLHIP_OP_ADD, acc, acc, x, nullptr, batch, st);
    };
    for (size_t j = 0; j < n2; ++j) {
      const bool keyed = gkeys[j] != nullptr;
      if (kb)  // V_{j,c} into V = [2][batch]
        for (size_t c = 0; c < 2; ++c) {
          char *Vc = V + c * batch * pb;
          bool first = true;
          const nflhip_dot_operand pa = {P, 1, 0};
          for (size_t m = 0; m < kb; ++m) {
            if (!wt(j, kbi[m])) continue;
            if ((rc = nflhip_automorphism_dev(ctx, P, S + (2 * m + c) * batch * pb, batch, bks[kbi[m]], NFLHIP_FORM_NTT, st))) return rc;
            if (kl) {  // the diagonal lies in the parent's layout as a key component does: the level-key operand, one term
              if ((rc = dot_key(ctx, Vc, &pa, wt(j, kbi[m]), 0, first ? nullptr : Vc, batch, 1, kl, st))) return rc;
            } else {
              const nflhip_dot_operand w = {wt(j, kbi[m]), 0, 0};
              if ((rc = nflhip_dot_dev(ctx, Vc, &pa, &w, first ? nullptr : Vc, batch, 1, 0, st))) return rc;
            }
            first = false;
          }
          if (first) HIPCHK(ctx, hipMemsetAsync(Vc, 0, batch * pb, st));
        }
      size_t nw = 0;  // W_{j,0} into W
      for (size_t i = 0; i < n1 && c0; ++i)
        if (wt(j, i)) cin[nw] = c0, cw[nw] = wt(j, i), cks[nw++] = bks[i];
      if (c0 && (rc = nflhip_automorphism_mac_dev(ctx, W, nullptr, cin, cw, cks, nw, batch, L, 0, st))) return rc;
      nw = 0;  // the terms of W_{j,1}
      for (size_t m = 0; m < ub; ++m)
        if (wt(j, ubi[m])) cin[nw] = c1, cw[nw] = wt(j, ubi[m]), cks[nw++] = 1;
      if (keyed) {
        if (kb && (rc = nflhip_moddown_ntt_dev(ctx, v, V + batch * pb, batch, K, mdflags, st))) return rc;
        if (nw) {
          if ((rc = nflhip_automorphism_mac_dev(ctx, v, kb ? v : nullptr, cin, cw, cks, nw, batch, L, 0, st))) return rc;
        } else if (!kb) {
          HIPCHK(ctx, hipMemsetAsync(v, 0, batch * qb, st));
        }
        nflhip_dot_operand u2;
        if ((rc = modup_copy_in(ctx, route, X2, v, batch, L, st))) return rc;
        if ((rc = modup_run(ctx, child, route, U2, X2, recs, batch, L, alpha, centred, "bsgs", st, &u2))) return rc;
        for (size_t c = 0; c < 2; ++c) {
          char *Tc = T + c * batch * pb, *Ac = A + c * batch * pb;
          if ((rc = dot_key(ctx, Tc, &u2, gkeys[j], c, c == 0 && kb ? V : nullptr, batch, dnum, kl, st))) return rc;
          if (a_init) {
            if ((rc = nflhip_automorphism_dev(ctx, P, Tc, batch, gks[j], NFLHIP_FORM_NTT, st)) || (rc = accumulate(ctx, Ac, P, false))) return rc;
          } else if ((rc = nflhip_automorphism_dev(ctx, Ac, Tc, batch, gks[j], NFLHIP_FORM_NTT, st))) {
            return rc;
          }
        }
        a_init = true;
        if (c0) {
          if (o0_init) {
            if ((rc = nflhip_automorphism_dev(child, Pq, W, batch, gks[j], NFLHIP_FORM_NTT, st)) || (rc = accumulate(child, O0, Pq, false))) return rc;
          } else if ((rc = nflhip_automorphism_dev(child, O0, W, batch, gks[j], NFLHIP_FORM_NTT, st))) {
            return rc;
          }
          o0_init = true;
        }
      } else {
        if (kb) {
          for (size_t c = 0; c < 2; ++c)
            if ((rc = accumulate(ctx, A + c * batch * pb, V + c * batch * pb, !a_init))) return rc;
          a_init = true;
        }
        if (c0) {
          if ((rc = accumulate(child, O0, W, !o0_init))) return rc;
          o0_init = true;
        }
        if (nw) {
          if ((rc = nflhip_automorphism_mac_dev(ctx, O1, o1_init ? O1 : nullptr, cin, cw, cks, nw, batch, L, 0, st))) return rc;
          o1_init = true;
        }
      }
    }
    if (a_init && (rc = nflhip_moddown_ntt_dev(ctx, Y, A, 2 * batch, K, mdflags, st))) return rc;
    // out_c = Y_c + O_c, added in the scratch; the copy out serves any alignment of the outputs
    for (size_t c = 0; c < 2; ++c) {
      char *Yc = Y + c * batch * qb, *Oc = c ? O1 : O0;
      const bool o_init = c ? o1_init : o0_init;
      void *out = c ? out1 : out0;
      if (a_init && o_init && (rc = accumulate(child, Yc, Oc, false))) return rc;
      if ((a_init || o_init) && (rc = set_device(ctx))) return rc;
      if (a_init || o_init) HIPCHK(ctx, hipMemcpyAsync(out, a_init ? Yc : Oc, batch * qb, hipMemcpyDeviceToDevice, st));
      else HIPCHK(ctx, hipMemsetAsync(out, 0, batch * qb, st));
    }
    if ((rc = set_device(ctx))) return rc;
  } else {
    void *douts[2 * NFLHIP_BSGS_MAX_BABY], *vouts[NFLHIP_BSGS_MAX_GIANT];
    const void *dbs[2 * NFLHIP_BSGS_MAX_BABY], *sins[NFLHIP_BSGS_MAX_BABY], *pins[NFLHIP_BSGS_MAX_GIANT];
    const void *gw[NFLHIP_BSGS_MAX_GIANT * NFLHIP_BSGS_MAX_BABY];
    uint64_t kks[NFLHIP_BSGS_MAX_BABY], pks[NFLHIP_BSGS_MAX_GIANT], ones_k[NFLHIP_BSGS_MAX_BABY];
    const void *c1s[NFLHIP_BSGS_MAX_BABY], *c0s[NFLHIP_BSGS_MAX_BABY];
    for (size_t i = 0; i < NFLHIP_BSGS_MAX_BABY; ++i) c1s[i] = c1, c0s[i] = c0, ones_k[i] = 1;
    if (kb) {
      for (size_t m = 0; m < kb; ++m) {
        for (size_t c = 0; c < 2; ++c) {
          douts[2 * m + c] = S + (2 * m + c) * batch * pb;
          dbs[2 * m + c] = (const char *)bkeys[kbi[m]] + c * (kl ? kl->knm * row : pb);
        }
        sins[m] = douts[2 * m];  // component c of baby m lies c batch polynomials behind
        kks[m] = bks[kbi[m]];
      }
      hipError_t e = with_limb(ctx, [&](auto z) {
        typedef decltype(z) T;
        return kl ? launch_dot_multi_level<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, u.group_stride, u.term_stride,
                                              (const T *const *)dbs, 2 * kb, batch, dnum, 1, *kl, st)
                  : launch_dot_multi<T>(ctx->shape, ctx->tabs, (T *const *)douts, (const T *)U, u.group_stride, u.term_stride, (const T *const *)dbs, 2,
                                        2 * kb, batch, dnum, 1, st);
      });
      if (e != hipSuccess) return hipfail(ctx, e, "bsgs: the babies' inner products");
    }
    // the giants of one kind in groups: V = [2][cnt][batch] on all rows
    for (int kind = 0; kind < 2; ++kind) {
      const bool keyed = kind == 0;
      const size_t total = keyed ? kg : kb ? ug : 0;  // (an unkeyed giant with no keyed baby has nothing on all rows)
      const size_t *js = keyed ? kgj : ugj;
      for (size_t g0 = 0; g0 < total; g0 += kBsgsGroup) {
        const size_t cnt = std::min(kBsgsGroup, total - g0);
        char *V1 = V + cnt * batch * pb;
        for (size_t s = 0; s < cnt; ++s) {
          vouts[s] = V + s * batch * pb;
          pins[s] = vouts[s];
          pks[s] = keyed ? gks[js[g0 + s]] : 1;
          for (size_t m = 0; m < kb; ++m) gw[s * kb + m] = wt(js[g0 + s], kbi[m]);
        }
        if (kb) {
          hipError_t e = with_limb(ctx, [&](auto z) {
            typedef decltype(z) T;
            if (kl)
              return launch_permute_mac_multi_ntt_level<T>(ctx->shape, ctx->tabs, (T *const *)vouts, nullptr, (const T *const *)sins, (const T *const *)gw,
                                                           kks, (int)cnt, (int)kb, batch, 2, batch * pw, cnt * batch * pw, *kl, st);
            return launch_permute_mac_multi_ntt<T>(ctx->shape, ctx->tabs, (T *const *)vouts, nullptr, (const T *const *)sins, (const T *const *)gw, kks,
                                                   (int)cnt, (int)kb, batch, nm, 2, batch * pw, cnt * batch * pw, st);
          });
          if (e != hipSuccess) return hipfail(ctx, e, "bsgs: the inner sums");
        }
        if (keyed) {
          if (kb && ((rc = nflhip_moddown_ntt_dev(ctx, v, V1, cnt * batch, K, mdflags, st)) || (rc = set_device(ctx)))) return rc;
          if (ub) {  // W_{j,1} on the kept rows, onto the mod-down's result
            for (size_t s = 0; s < cnt; ++s) {
              vouts[s] = v + s * batch * qb;
              for (size_t m = 0; m < ub; ++m) gw[s * ub + m] = wt(js[g0 + s], ubi[m]);
            }
            hipError_t e = with_limb(ctx, [&](auto z) {
              typedef decltype(z) T;
              return launch_permute_mac_multi_ntt<T>(ctx->shape, ctx->tabs, (T *const *)vouts, kb ? (const T *const *)vouts : nullptr,
                                                     (const T *const *)c1s, (const T *const *)gw, ones_k, (int)cnt, (int)ub, batch, L, 1, 0, 0, st);
            });
            if (e != hipSuccess) return hipfail(ctx, e, "bsgs: the unrotated babies");
          }
          nflhip_dot_operand u2;
          if ((rc = modup_copy_in(ctx, route, X2, v, cnt * batch, L, st))) return rc;
          if ((rc = modup_run(ctx, child, route, U2, X2, recs, cnt * batch, L, alpha, centred, "bsgs", st, &u2))) return rc;
          for (size_t s = 0; s < cnt; ++s)
            for (size_t c = 0; c < 2; ++c) {
              const nflhip_dot_operand a = {U2 + s * batch * u2.group_stride * pb, u2.group_stride, u2.term_stride};
              char *o = (c ? V1 : V) + s * batch * pb;  // T_{j,c} in place of V_{j,c}
              if ((rc = dot_key(ctx, o, &a, gkeys[js[g0 + s]], c, c == 0 && kb ? o : nullptr, batch, dnum, kl, st))) return rc;
            }
          if ((rc = set_device(ctx))) return rc;
        }
        hipError_t e = with_limb(ctx, [&](auto z) {
          typedef decltype(z) T;
          return launch_permute_sum_ntt<T>(ctx->shape, ctx->tabs, (T *)A, a_init ? (const T *)A : nullptr, (const T *const *)pins, pks, (int)cnt, batch, nm,
                                           2, cnt * batch * pw, batch * pw, st);
        });
        if (e != hipSuccess) return hipfail(ctx, e, "bsgs: the giant steps' permutation");
        a_init = true;
      }
    }
    if (a_init) {
      if ((rc = moddown_pair(ctx, out0, out1, A, batch, K, floor, st))) return rc;
      o0_init = o1_init = true;
    }
    // the passes on the kept rows
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      hipError_t r = hipSuccess;
      if (c0) {
        for (size_t j = 0; j < n2; ++j) vouts[j] = W + j * batch * qb, pins[j] = vouts[j];
        r = launch_permute_mac_multi_ntt<T>(ctx->shape, ctx->tabs, (T *const *)vouts, nullptr, (const T *const *)c0s, (const T *const *)weights, bks, (int)n2,
                                            (int)n1, batch, L, 1, 0, 0, st);
        if (r == hipSuccess)
          r = launch_permute_sum_ntt<T>(ctx->shape, ctx->tabs, (T *)out0, o0_init ? (const T *)out0 : nullptr, (const T *const *)pins, gks, (int)n2, batch, L,
                                        1, 0, 0, st);
        o0_init = true;
      }
      for (size_t s = 0; s < ug && ub && r == hipSuccess; ++s) {  // the unkeyed giants' W_{j,1}
        int nw = 0;
        for (size_t m = 0; m < ub; ++m)
          if (wt(ugj[s], ubi[m])) gw[nw++] = wt(ugj[s], ubi[m]);
        if (!nw) continue;
        r = launch_permute_mac_ntt<T>(ctx->shape, ctx->tabs, (T *)out1, o1_init ? (const T *)out1 : nullptr, (const T *const *)c1s, (const T *const *)gw,
                                      ones_k, nw, batch, L, 1, 0, 0, 0, st);
        o1_init = true;
      }
      return r;
    });
    if (e != hipSuccess) return hipfail(ctx, e, "bsgs: the terms on the kept rows");
    if (!o0_init) HIPCHK(ctx, hipMemsetAsync(out0, 0, batch * qb, st));
    if (!o1_init) HIPCHK(ctx, hipMemsetAsync(out1, 0, batch * qb, st));
  }
  if ((rc = ws_end(ctx, ctx->bsgs_ws, cap, st))) return rc;
  if (!cap) warm_note(ctx->bsgs_warm, wkey, wsizes);
  return NFLHIP_OK;
}
int nflhip_bsgs_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_bkeys, const uint64_t *bks,
                        size_t n1, const void *const *d_gkeys, const uint64_t *gks, size_t n2, const void *const *d_weights, size_t batch,
                        size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  int rc = bsgs_check(ctx, d_out0, d_out1, d_c0, d_c1, d_bkeys, bks, n1, d_gkeys, gks, n2, d_weights, batch, k_special, alpha, level, flags);  // in full, before any device use
  if (rc || batch == 0) return rc;
  nflhip_ctx *run = nullptr;
  KeyLevel kl;
  if ((rc = level_context(ctx, k_special, level, (hipStream_t)stream, &run, &kl))) return rc;
  return bsgs_run(run, d_out0, d_out1, d_c0, d_c1, d_bkeys, bks, n1, d_gkeys, gks, n2, d_weights, batch, k_special, std::min(alpha, level), flags,
                  (hipStream_t)stream, run == ctx ? nullptr : &kl);
}

int nflhip_pointwise_dev(nflhip_ctx *ctx, int op, void *o, const void *a, const void *b, const void *bp, size_t batch,
                         void *stream) {
  CHECK_CTX(ctx);
  if (op < 0 || op > 4) return fail(ctx, NFLHIP_ERR_INVALID, "unknown element-wise op");
  if (batch && (!o || !a || (op != NFLHIP_OP_COMPUTE_SHOUP && !b) || (op == NFLHIP_OP_MUL_SHOUP && !bp)))
    return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_pointwise<T>(ctx->shape, ctx->tabs, op, (T *)o, (const T *)a, (const T *)b, (const T *)bp, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "pointwise");
  return NFLHIP_OK;
}

static int eval_dev(nflhip_ctx *ctx, void *out, const void *const *ops, size_t nops, const unsigned char *prog, size_t len,
                    size_t batch, void *stream, const unsigned *strides = nullptr, unsigned out_stride = 1) {
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_eval_expr<T>(ctx->shape, ctx->tabs, (T *)out, ops, (int)nops, prog, (int)len, batch, st, strides, out_stride);
  });
  if (e == hipErrorInvalidValue) return fail(ctx, NFLHIP_ERR_INVALID, "malformed expression program");
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "row shorter than one 16-byte vector");
  if (e != hipSuccess) return hipfail(ctx, e, "eval");
  return NFLHIP_OK;
}

static int polymul_any(nflhip_ctx *ctx, void *c, const void *a, const void *b, int b_is_ntt, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (batch && (!c || !a || !b)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (batch == 0) return NFLHIP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rc = fast_family(ctx, b_is_ntt ? 1 : 0, c, a, b, batch, st);
  if (rc != NFLHIP_ERR_UNSUPPORTED) return rc;
  return with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return polymul_composed<T>(ctx, (T *)c, (const T *)a, (const T *)b, b_is_ntt, batch, st);
  });
}

int nflhip_eval_dev(nflhip_ctx *ctx, void *d_out, const void *const *d_operands, size_t noperands,
                    const unsigned char *program, size_t proglen, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (!program || !d_operands || (batch && !d_out)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (noperands == 0 || noperands > NFLHIP_EXPR_MAX_OPERANDS || proglen == 0 || proglen > NFLHIP_EXPR_MAX_LEN)
    return fail(ctx, NFLHIP_ERR_INVALID, "expression program too large");
  for (size_t i = 0; i < noperands; ++i)
    if (batch && !d_operands[i]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  return eval_dev(ctx, d_out, d_operands, noperands, program, proglen, batch, stream);
}

int nflhip_eval_strided_dev(nflhip_ctx *ctx, void *d_out, size_t out_stride, const void *const *d_operands,
                            const size_t *strides, size_t noperands, const unsigned char *program, size_t proglen,
                            size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (!program || !d_operands || !strides || (batch && !d_out)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (noperands == 0 || noperands > NFLHIP_EXPR_MAX_OPERANDS || proglen == 0 || proglen > NFLHIP_EXPR_MAX_LEN)
    return fail(ctx, NFLHIP_ERR_INVALID, "expression program too large");
  unsigned sd[NFLHIP_EXPR_MAX_OPERANDS];
  for (size_t i = 0; i < noperands; ++i) {
    if (batch && !d_operands[i]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    if (strides[i] > 0xffffffffu) return fail(ctx, NFLHIP_ERR_INVALID, "operand stride out of range");
    sd[i] = (unsigned)strides[i];
  }
  if (out_stride == 0 || out_stride > 0xffffffffu) return fail(ctx, NFLHIP_ERR_INVALID, "the result stride must be positive");
  return eval_dev(ctx, d_out, d_operands, noperands, program, proglen, batch, stream, sd, (unsigned)out_stride);
}

int nflhip_polymul_dev(nflhip_ctx *ctx, void *c, const void *a, const void *b, size_t batch, void *stream) {
  return polymul_any(ctx, c, a, b, 0, batch, stream);
}
int nflhip_polymul_ntt_dev(nflhip_ctx *ctx, void *c, const void *a, const void *bntt, size_t batch, void *stream) {
  return polymul_any(ctx, c, a, bntt, 1, batch, stream);
}

// ---------------------------------------------------------------------------
// transform-fused pipelines
// ---------------------------------------------------------------------------
static int check_operand(const nflhip_ctx *ctx, const nflhip_operand *o, size_t batch, bool words_only, const char *what) {
  if (!o || (batch && !o->ptr)) return fail(ctx, NFLHIP_ERR_INVALID, std::string("NULL operand: ") + what);
  if (o->format < NFLHIP_FMT_WORDS || o->format > NFLHIP_FMT_I32 || (words_only && o->format != NFLHIP_FMT_WORDS))
    return fail(ctx, NFLHIP_ERR_INVALID, std::string("operand format: ") + what);
  if (o->stride > 0xffffffffu || (batch > 1 && (uint64_t)o->stride * (batch - 1) > 0xffffffffull))
    return fail(ctx, NFLHIP_ERR_INVALID, std::string("operand stride out of range: ") + what);
  return NFLHIP_OK;
}

static hipError_t expand_any(nflhip_ctx *ctx, void *dst, const nflhip_operand *src, size_t batch, hipStream_t st) {
  return with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_expand_small<T>(ctx->shape, ctx->tabs, (T *)dst, src->ptr, src->format, (unsigned)src->stride, batch, st);
  });
}

// out0 of a two-result call lies over (part of) an input of the SECOND result (k1 or e1): the one aliasing in which a plan that
// stores the first result before it has read the second one's inputs would change them under its own feet
static bool first_result_overlaps(nflhip_ctx *ctx, const void *out0, const nflhip_operand *in, size_t batch) {
  const size_t per = in->format == NFLHIP_FMT_WORDS ? poly_bytes(ctx, 1) : ctx->shape.n << (in->format - NFLHIP_FMT_I8);
  const char *o = (const char *)out0, *k = (const char *)in->ptr;
  return o < k + ((batch - 1) * in->stride + 1) * per && k < o + poly_bytes(ctx, batch);
}

static int fused_fwd_composed(nflhip_ctx *ctx, void *out0, void *out1, const nflhip_operand *x, const nflhip_operand *k0,
                              const nflhip_operand *e0, const nflhip_operand *k1, const nflhip_operand *e1, size_t batch,
                              hipStream_t st) {
  // the same result from the plain kernels: expand / gather into the context's scratch, transform there, one fused
  // multiply-add pass per result (what serves every shape without a generated kernel, and NFLHIP_VARIANT=hipcc)
  const size_t bytes = poly_bytes(ctx, batch);
  std::unique_lock<std::mutex> lk(ctx->scratch_mu);
  const bool cap = is_capturing(st);
  // three polynomials of scratch per batch element only when the first result lies over an input of the second one (then every
  // input is read before anything is stored); otherwise two: e1 is transformed into e0's place after the first result is out
  const bool overlap = out1 && (first_result_overlaps(ctx, out0, e1, batch) || first_result_overlaps(ctx, out0, k1, batch));
  int rc = ensure_scratch(ctx, (overlap ? 3 : 2) * bytes);
  if (rc) return rc;
  if (!cap && ctx->ev_scratch_valid) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_scratch, 0));
  if (!cap && ctx->ev_prev_valid)
    for (int j = 0; j < 2; ++j) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_done[j], 0));
  void *s0 = ctx->scratch, *s1 = (char *)ctx->scratch + bytes, *s2 = (char *)ctx->scratch + 2 * bytes;
  static const unsigned char prog[5] = {0, 1, NFLHIP_EXPR_MUL, 2, NFLHIP_EXPR_ADD};
  // rows of 32768 words with int8 polynomials and keys shared by the batch (the LWE demo at the reference's largest configuration):
  // the noise polynomials go from their bytes straight to NTT words in the scratch, then ONE kernel transforms x in registers and
  // writes X k + e' for both results -- 6 polynomial passes over HBM instead of 17
  if (ctx->shape.limb_bits == 64 && ctx->shape.logn == 15 && x->format == NFLHIP_FMT_I8 && e0->format == NFLHIP_FMT_I8 &&
      (!out1 || e1->format == NFLHIP_FMT_I8) && x->stride == 1 && e0->stride == 1 && (!out1 || e1->stride == 1) && k0->stride == 0 &&
      (!out1 || k1->stride == 0)) {
    hipError_t e5 = launch_row32k_fwd_i8_u64(ctx->shape, ctx->tabs, (uint64_t *)s0, e0->ptr, batch, st);
    if (e5 == hipSuccess && out1) e5 = launch_row32k_fwd_i8_u64(ctx->shape, ctx->tabs, (uint64_t *)s1, e1->ptr, batch, st);
    if (e5 == hipSuccess)
      e5 = launch_row32k_fwd_fma_i8_u64(ctx->shape, ctx->tabs, (uint64_t *)out0, (uint64_t *)out1, x->ptr, (const uint64_t *)k0->ptr,
                                        (const uint64_t *)s0, out1 ? (const uint64_t *)k1->ptr : nullptr, (const uint64_t *)s1, batch, st);
    if (e5 != hipErrorNotSupported) {
      if (e5 != hipSuccess) return hipfail(ctx, e5, "fwd_fma: 32768-word row kernels");
      if (!cap) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_scratch, st));
        ctx->ev_scratch_valid = true;
        for (int j = 0; j < 2; ++j)
          if (ctx->aux[j]) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[j], ctx->ev_scratch, 0));
      }
      return NFLHIP_OK;
    }
  }
  hipError_t e = expand_any(ctx, s0, x, batch, st);
  if (e != hipSuccess) return hipfail(ctx, e, "fwd_fma: expand");
  rc = nflhip_ntt_fwd_dev(ctx, s0, batch, st);
  if (rc) return rc;
  // a result may alias a dense input of the same call (nflhip.h): every input polynomial is read into the scratch BEFORE the
  // first result is stored (e1 may be out0), and when out0 overlaps a per-element k1 the first result waits in the scratch
  // until the second has been computed -- the generated kernels read a whole row of every operand before they store, the
  // composed plan gives the same guarantee
  if (!overlap) {
    for (int h = 0; h < (out1 ? 2 : 1); ++h) {
      e = expand_any(ctx, s1, h ? e1 : e0, batch, st);
      if (e != hipSuccess) return hipfail(ctx, e, "fwd_fma: expand");
      rc = nflhip_ntt_fwd_dev(ctx, s1, batch, st);
      if (rc) return rc;
      const nflhip_operand *kk = h ? k1 : k0;
      const void *ops[3] = {s0, kk->ptr, s1};
      const unsigned sd[3] = {1, (unsigned)kk->stride, 1};
      rc = eval_dev(ctx, h ? out1 : out0, ops, 3, prog, sizeof(prog), batch, st, sd, 1);
      if (rc) return rc;
    }
  } else {
    for (int h = 0; h < 2; ++h) {
      void *sh = h ? s2 : s1;
      e = expand_any(ctx, sh, h ? e1 : e0, batch, st);
      if (e != hipSuccess) return hipfail(ctx, e, "fwd_fma: expand");
      rc = nflhip_ntt_fwd_dev(ctx, sh, batch, st);
      if (rc) return rc;
    }
    const bool hold0 = first_result_overlaps(ctx, out0, k1, batch);
    for (int h = 0; h < 2; ++h) {
      const nflhip_operand *kk = h ? k1 : k0;
      void *sh = h ? s2 : s1;
      const void *ops[3] = {s0, kk->ptr, sh};
      const unsigned sd[3] = {1, (unsigned)kk->stride, 1};
      rc = eval_dev(ctx, h ? out1 : (hold0 ? s1 : out0), ops, 3, prog, sizeof(prog), batch, st, sd, 1);
      if (rc) return rc;
    }
    if (hold0) HIPCHK(ctx, hipMemcpyAsync(out0, s1, bytes, hipMemcpyDeviceToDevice, st));
  }
  if (!cap) {  // the scratch is reused by the next call on any stream: order it after this one
    HIPCHK(ctx, hipEventRecord(ctx->ev_scratch, st));
    ctx->ev_scratch_valid = true;
    for (int j = 0; j < 2; ++j)
      if (ctx->aux[j]) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[j], ctx->ev_scratch, 0));
  }
  return NFLHIP_OK;
}

static int fused_fwd_any(nflhip_ctx *ctx, void *out0, void *out1, const nflhip_operand *x, const nflhip_operand *k0,
                         const nflhip_operand *e0, const nflhip_operand *k1, const nflhip_operand *e1, size_t batch,
                         void *stream) {
  CHECK_CTX(ctx);
  const bool two = k1 != nullptr;
  if (batch && (!out0 || (two && !out1))) return fail(ctx, NFLHIP_ERR_INVALID, "NULL result pointer");
  int rc = check_operand(ctx, x, batch, false, "x");
  if (!rc) rc = check_operand(ctx, k0, batch, true, "k0");
  if (!rc) rc = check_operand(ctx, e0, batch, false, "e0");
  if (!rc && two) rc = check_operand(ctx, k1, batch, true, "k1");
  if (!rc && two) rc = check_operand(ctx, e1, batch, false, "e1");
  if (rc) return rc;
  if (batch == 0) return NFLHIP_OK;
  // a result may lie over a DENSE input (nflhip.h); over an operand the whole batch shares (stride 0, batch > 1) it would be
  // written by one batch element while the others still read it: refused, not raced
  if (batch > 1) {
    const nflhip_operand *ins[5] = {x, k0, e0, k1, e1};
    void *outs[2] = {out0, two ? out1 : nullptr};
    for (const nflhip_operand *in : ins)
      for (void *o : outs)
        if (in && o && in->stride == 0 && first_result_overlaps(ctx, o, in, batch))
          return fail(ctx, NFLHIP_ERR_INVALID, "a result overlaps an operand shared by the batch (stride 0)");
  }
  hipStream_t st = (hipStream_t)stream;
  // (the generated two-result kernels store a row of out0 before they load that row of k1 and, the row-resident ones, of e1: a
  // first result laid over an input of the second -- legal, nflhip.h -- takes the composed plan, which reads every polynomial
  // before it stores and holds out0 back when it must)
  if (ctx->shape.limb_bits == 64 && !(two && (first_result_overlaps(ctx, out0, k1, batch) || first_result_overlaps(ctx, out0, e1, batch)))) {
    const void *xs[3] = {x->ptr, e0->ptr, two ? e1->ptr : nullptr};
    const unsigned xstr[3] = {(unsigned)x->stride, (unsigned)e0->stride, two ? (unsigned)e1->stride : 0u};
    const int xf[3] = {x->format, e0->format, two ? e1->format : 0};
    const void *ks[2] = {k0->ptr, two ? k1->ptr : nullptr};
    const unsigned kstr[2] = {(unsigned)k0->stride, two ? (unsigned)k1->stride : 0u};
    hipError_t e = launch_fused_asm_u64(ctx->shape, ctx->tabs, two ? 0 : 1, (uint64_t *)out0, (uint64_t *)out1, xs, xstr, xf, ks, kstr,
                                        batch, st);
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "fwd_fma(fused)");
  }
  // short rows (1024 / 2048 words; 4096 for 32-bit limbs): the wave-per-row kernels transform x once, keep it in registers and
  // multiply-add each transformed noise row in place (kernels_wave.hip k_row_fwd_fma) -- operands of one format, strides 0 / 1
  const bool aliased = two && (first_result_overlaps(ctx, out0, k1, batch) || first_result_overlaps(ctx, out0, e1, batch));
  // (compact rows are fetched 16 bytes per lane: their arrays must be 16-byte aligned -- device allocations are; a caller's odd offset
  //  into one takes the composed plan)
  const bool aligned16 = ((((uintptr_t)x->ptr) | ((uintptr_t)e0->ptr) | (two ? (uintptr_t)e1->ptr : 0)) & 15) == 0;
  if (!aliased && aligned16 && !ctx->cyclic && !ctx->shape.compiled_only && x->format == e0->format && (!two || e1->format == x->format) && x->stride <= 1 &&
      e0->stride <= 1 && k0->stride <= 1 && (!two || (e1->stride <= 1 && k1->stride <= 1))) {
    hipError_t e = hipErrorNotSupported;
    if (ctx->shape.limb_bits == 32)
      e = launch_row_fwd_fma_u32(ctx->shape, ctx->tabs, x->format, (uint32_t *)out0, (uint32_t *)out1, x->ptr, (unsigned)x->stride,
                                 (const uint32_t *)k0->ptr, (unsigned)k0->stride, e0->ptr, (unsigned)e0->stride, two ? (const uint32_t *)k1->ptr : nullptr,
                                 two ? (unsigned)k1->stride : 0u, two ? e1->ptr : nullptr, two ? (unsigned)e1->stride : 0u, batch, st);
    else if (ctx->shape.limb_bits == 64)
      e = launch_row_fwd_fma_u64(ctx->shape, ctx->tabs, x->format, (uint64_t *)out0, (uint64_t *)out1, x->ptr, (unsigned)x->stride,
                                 (const uint64_t *)k0->ptr, (unsigned)k0->stride, e0->ptr, (unsigned)e0->stride, two ? (const uint64_t *)k1->ptr : nullptr,
                                 two ? (unsigned)k1->stride : 0u, two ? e1->ptr : nullptr, two ? (unsigned)e1->stride : 0u, batch, st);
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "fwd_fma(rows)");
  }
  return fused_fwd_composed(ctx, out0, out1, x, k0, e0, k1, e1, batch, st);
}

int nflhip_fwd_fma_dev(nflhip_ctx *ctx, void *d_out, const nflhip_operand *x, const nflhip_operand *k, const nflhip_operand *e,
                       size_t batch, void *stream) {
  return fused_fwd_any(ctx, d_out, nullptr, x, k, e, nullptr, nullptr, batch, stream);
}

int nflhip_fwd_fma2_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const nflhip_operand *x, const nflhip_operand *k0,
                        const nflhip_operand *e0, const nflhip_operand *k1, const nflhip_operand *e1, size_t batch, void *stream) {
  if (!k1 || !e1) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  return fused_fwd_any(ctx, d_out0, d_out1, x, k0, e0, k1, e1, batch, stream);
}

int nflhip_fma_inv_dev(nflhip_ctx *ctx, void *d_out, const nflhip_operand *a, const nflhip_operand *k, const nflhip_operand *b,
                       int subtract, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (batch && !d_out) return fail(ctx, NFLHIP_ERR_INVALID, "NULL result pointer");
  int rc = check_operand(ctx, a, batch, true, "a");
  if (!rc) rc = check_operand(ctx, k, batch, true, "k");
  if (!rc) rc = check_operand(ctx, b, batch, true, "b");
  if (rc) return rc;
  if (batch == 0) return NFLHIP_OK;
  hipStream_t st = (hipStream_t)stream;
  if (ctx->shape.limb_bits == 64) {
    const void *xs[3] = {a->ptr, b->ptr, nullptr};
    const unsigned xstr[3] = {(unsigned)a->stride, (unsigned)b->stride, 0u};
    const int xf[3] = {0, 0, 0};
    const void *ks[2] = {k->ptr, nullptr};
    const unsigned kstr[2] = {(unsigned)k->stride, 0u};
    hipError_t e = launch_fused_asm_u64(ctx->shape, ctx->tabs, subtract ? 2 : 3, (uint64_t *)d_out, nullptr, xs, xstr, xf, ks, kstr, batch, st);
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "fma_inv(fused)");
  }
  // short rows (1024 / 2048 words; 4096 for 32-bit limbs): the wave-per-row kernels multiply-subtract in the registers their
  // inverse transform starts from (kernels_wave.hip k_row_fma_inv)
  if (a->stride == 1 && b->stride == 1 && k->stride <= 1 && !ctx->cyclic) {
    hipError_t e = hipErrorNotSupported;
    if (ctx->shape.limb_bits == 32)
      e = launch_row_fma_inv_u32(ctx->shape, ctx->tabs, subtract, (uint32_t *)d_out, (const uint32_t *)a->ptr, (const uint32_t *)k->ptr,
                                 (int)k->stride, (const uint32_t *)b->ptr, batch, st);
    else if (ctx->shape.limb_bits == 64)
      e = launch_row_fma_inv_u64(ctx->shape, ctx->tabs, subtract, (uint64_t *)d_out, (const uint64_t *)a->ptr, (const uint64_t *)k->ptr,
                                 (int)k->stride, (const uint64_t *)b->ptr, batch, st);
    if (e == hipSuccess) return NFLHIP_OK;
    if (e != hipErrorNotSupported) return hipfail(ctx, e, "fma_inv(rows)");
  }
  // composed: one fused multiply-add / -subtract pass into the result, inverse transform in place
  const unsigned char prog[5] = {0, 1, 2, NFLHIP_EXPR_MUL, (unsigned char)(subtract ? NFLHIP_EXPR_SUB : NFLHIP_EXPR_ADD)};
  const void *ops[3] = {b->ptr, a->ptr, k->ptr};
  const unsigned sd[3] = {(unsigned)b->stride, (unsigned)a->stride, (unsigned)k->stride};
  rc = eval_dev(ctx, d_out, ops, 3, prog, sizeof(prog), batch, stream, sd, 1);
  if (rc) return rc;
  return nflhip_ntt_inv_dev(ctx, d_out, batch, stream);
}

int nflhip_has_fused_kernels(const nflhip_ctx *ctx) {
  if (!ctx || ctx->shape.compiled_only || ctx->cyclic || ctx->shape.nm > 65535) return 0;
  const Shape &s = ctx->shape;
  if (s.limb_bits == 64) return s.small_delta && s.logn >= 10 && s.logn <= 15;    // 1024 / 2048: the wave-per-row kernels; 4096 ... 32768: generated
  return s.limb_bits == 32 && s.logn >= 10 && s.logn <= 12;                       // the wave-per-row kernels
}

int nflhip_expand_small_dev(nflhip_ctx *ctx, void *d_data, const nflhip_operand *src, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (batch && !d_data) return fail(ctx, NFLHIP_ERR_INVALID, "NULL result pointer");
  int rc = check_operand(ctx, src, batch, false, "src");
  if (rc) return rc;
  hipError_t e = expand_any(ctx, d_data, src, batch, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(ctx, e, "expand_small");
  return NFLHIP_OK;
}

static int any_cmp_dev(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int want_eq, int *result, void *stream) {
  CHECK_CTX(ctx);
  if (!result || (batch && (!a || !b))) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  return flag_call(ctx, st, "any_cmp", result, [&](auto z, int *flag, int token) {
    typedef decltype(z) T;
    return launch_any_cmp<T>(ctx->shape, ctx->tabs, (const T *)a, (const T *)b, batch, want_eq, flag, token, st);
  });
}
int nflhip_check_range_dev(nflhip_ctx *ctx, const void *d_data, size_t batch, int *bad, void *stream) {
  CHECK_CTX(ctx);
  if (!bad || (batch && !d_data)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  return flag_call(ctx, st, "check_range", bad, [&](auto z, int *flag, int token) {
    typedef decltype(z) T;
    return launch_check_range<T>(ctx->shape, ctx->tabs, (const T *)d_data, batch, flag, token, st);
  });
}

int nflhip_any_eq_dev(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int *result, void *stream) {
  return any_cmp_dev(ctx, a, b, batch, 1, result, stream);
}
int nflhip_any_neq_dev(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int *result, void *stream) {
  return any_cmp_dev(ctx, a, b, batch, 0, result, stream);
}

int nflhip_crt_lift_dev(nflhip_ctx *ctx, uint64_t *limbs, const void *d, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (batch && (!limbs || !d)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  if (ctx->tabs.qhat_w && batch) {
    // any number of moduli: the limb-serial kernel over a stream-ordered scratch (the unreduced sums)
    uint64_t *scr = nullptr;
    const size_t words = batch * ctx->shape.n * (size_t)ctx->tabs.crt_Lw;
    HIPCHK(ctx, hipMallocAsync((void **)&scr, words * sizeof(uint64_t), st));
    hipError_t we = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_crt_lift_wide<T>(ctx->shape, ctx->tabs, limbs, (const T *)d, batch, scr, st);
    });
    (void)hipFreeAsync(scr, st);
    if (we != hipSuccess) return hipfail(ctx, we, "crt_lift (wide)");
    return NFLHIP_OK;
  }
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_crt_lift<T>(ctx->shape, ctx->tabs, limbs, (const T *)d, batch, st);
  });
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "crt_lift: more than 32 moduli");
  if (e != hipSuccess) return hipfail(ctx, e, "crt_lift");
  return NFLHIP_OK;
}

int nflhip_crt_project_dev(nflhip_ctx *ctx, void *d, const uint64_t *limbs, size_t L_in, size_t batch, void *stream) {
  CHECK_CTX(ctx);
  if (batch && (!limbs || !d)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (L_in == 0 || L_in > (1u << 20)) return fail(ctx, NFLHIP_ERR_INVALID, "L_in out of range");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_crt_project<T>(ctx->shape, ctx->tabs, (T *)d, limbs, L_in, batch, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "crt_project");
  return NFLHIP_OK;
}

int nflhip_fill_uniform_dev(nflhip_ctx *ctx, void *d, size_t first_poly, size_t batch, uint64_t seed, int operand,
                            void *stream) {
  CHECK_CTX(ctx);
  if (batch && !d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_fill_uniform<T>(ctx->shape, ctx->tabs, (T *)d, first_poly, batch, seed, operand, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "fill_uniform");
  return NFLHIP_OK;
}

// ---------------------------------------------------------------------------
// samplers
// ---------------------------------------------------------------------------
struct nflhip_gauss {
  GaussTable tab;
  uint64_t *d_cdt = nullptr;
  int device = 0;
  int draw_bits = 64;   // keystream bits a sample normally consumes (nflhip_gauss_set_draw_bits): 64, or 32 = the narrow draw
  uint16_t *d_lut = nullptr;   // the narrow draw's bucket table (kernels_sample.hip gauss_bucket_table); NULL: table too long for LDS
};
static inline int gauss_narrow(const nflhip_gauss *g) { return g->draw_bits == 32 ? 1 : 0; }

int nflhip_random_words_dev(nflhip_ctx *ctx, uint64_t *d_out, uint64_t first_word, size_t nwords, const unsigned char *key,
                            uint64_t stream_id, void *stream) {
  CHECK_CTX(ctx);
  if (!key || (nwords && !d_out)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipError_t e = launch_random_words(d_out, first_word, nwords, key, stream_id, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(ctx, e, "random_words");
  return NFLHIP_OK;
}

int nflhip_sample_dev(nflhip_ctx *ctx, void *d, size_t first_poly, size_t batch, int dist, uint64_t p0, uint64_t p1,
                      const unsigned char *key, uint64_t stream_id, void *stream) {
  CHECK_CTX(ctx);
  if (!key || (batch && !d)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  const int dist_in = dist;
  dist &= ~(NFLHIP_DIST_REFERENCE_WORDS | NFLHIP_DIST_NARROW);
  if (dist < NFLHIP_DIST_UNIFORM || dist > NFLHIP_DIST_HWT) return fail(ctx, NFLHIP_ERR_INVALID, "unknown distribution");
  if ((dist_in & NFLHIP_DIST_NARROW) && dist != NFLHIP_DIST_UNIFORM)
    return fail(ctx, NFLHIP_ERR_INVALID, "the narrow draw applies to the uniform rule only (the others read one word per coefficient)");
  if (dist == NFLHIP_DIST_BOUNDED) {
    if (p0 == 0 || p0 >= (((uint64_t)1) << 62)) return fail(ctx, NFLHIP_ERR_INVALID, "upper_bound out of range");
    for (uint64_t p : ctx->h_P)  // core.hpp:205-210
      if (p0 >= p) return fail(ctx, NFLHIP_ERR_INVALID, "core: upper_bound is larger than the modulus");
    if (p1 == 0) return fail(ctx, NFLHIP_ERR_INVALID, "amplifier must be positive");
  }
  if (dist == NFLHIP_DIST_ZO && p0 > 255) return fail(ctx, NFLHIP_ERR_INVALID, "rho is a byte");
  if (dist == NFLHIP_DIST_HWT && (p0 == 0 || p0 > ctx->shape.n))  // assert at core.hpp:349
    return fail(ctx, NFLHIP_ERR_INVALID, "hamming weight must be in [1, degree]");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_sample<T>(ctx->shape, ctx->tabs, (T *)d, first_poly, batch, dist_in, p0, p1, key, stream_id, st);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "sample");
  return NFLHIP_OK;
}

int nflhip_sample_seq_dev(nflhip_ctx *ctx, void *d, size_t batch, int dist, uint64_t p0, uint64_t p1, const unsigned char *key,
                          uint64_t first_stream_id, uint64_t stream_id_stride, void *stream) {
  // argument checks are those of nflhip_sample_dev (same messages): validate through it with an empty batch
  int rc = nflhip_sample_dev(ctx, d, 0, 0, dist, p0, p1, key, first_stream_id, stream);
  if (rc) return rc;
  if (batch && !d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_sample<T>(ctx->shape, ctx->tabs, (T *)d, 0, batch, dist, p0, p1, key, first_stream_id, st, 1, stream_id_stride);
  });
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "sequence mode needs degree >= 8");
  if (e != hipSuccess) return hipfail(ctx, e, "sample_seq");
  return NFLHIP_OK;
}

int nflhip_sample_gauss_seq_dev(nflhip_ctx *ctx, void *d, size_t batch, const nflhip_gauss *g, uint64_t amplifier,
                                const unsigned char *key, uint64_t first_stream_id, uint64_t stream_id_stride, void *stream) {
  CHECK_CTX(ctx);
  if (!key || !g || (batch && !d)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (g->device != ctx->device) return fail(ctx, NFLHIP_ERR_INVALID, "gaussian table lives on another device");
  if (amplifier == 0) return fail(ctx, NFLHIP_ERR_INVALID, "amplifier must be positive");
  hipStream_t st = (hipStream_t)stream;
  const int w = g->tab.words, en = (int)g->tab.entries;
  const long long x0 = g->tab.x_min;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_sample_gauss<T>(ctx->shape, ctx->tabs, (T *)d, 0, batch, g->d_cdt, w, en, x0, amplifier, key, first_stream_id, st, 1, stream_id_stride, gauss_narrow(g), g->d_lut);
  });
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "sequence mode needs degree >= 8 (>= 16 under the 32-bit draw)");
  if (e != hipSuccess) return hipfail(ctx, e, "sample_gauss_seq");
  return NFLHIP_OK;
}

// The table of a parameter set is computed once per process (448-bit fixed point on the host: milliseconds) and shared by every context's
// generator: the header's FastGaussianNoise asks for it when it is CONSTRUCTED (nflhip_gauss_table with no output buffer) -- where the
// reference builds its MPFR table -- so that the first polynomial drawn from it does not carry the construction
static int cached_gauss_table(double sigma, unsigned security, unsigned samples, double center, GaussTable *out, std::string *err) {
  // (checked before the lookup: a NaN compares equivalent to every key)
  if (check_gauss_params(sigma, security, samples, center, err)) return 1;
  typedef std::tuple<double, unsigned, unsigned, double> Key;
  static std::mutex mu;
  static std::map<Key, std::shared_ptr<const GaussTable>> cache;
  const Key key(sigma, security, samples, center);
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::shared_ptr<GaussTable> t = std::make_shared<GaussTable>();
    if (build_gauss_table(sigma, security, samples, center, t.get(), err)) return 1;
    if (cache.size() >= 64) cache.clear();
    it = cache.emplace(key, t).first;
  }
  *out = *it->second;
  return 0;
}

int nflhip_gauss_create(nflhip_ctx *ctx, nflhip_gauss **out, double sigma, unsigned security, unsigned samples,
                        double center) {
  CHECK_CTX(ctx);
  if (!out) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  std::unique_ptr<nflhip_gauss> g(new (std::nothrow) nflhip_gauss());
  if (!g) return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
  std::string err;
  try {
    if (cached_gauss_table(sigma, security, samples, center, &g->tab, &err)) return fail(ctx, NFLHIP_ERR_INVALID, err);
  } catch (const std::bad_alloc &) {
    return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory while building the gaussian table");
  }
  g->device = ctx->device;
  const size_t bytes = g->tab.cdt.size() * sizeof(uint64_t);
  HIPCHK(ctx, hipMalloc((void **)&g->d_cdt, bytes));
  hipError_t e = hipMemcpy(g->d_cdt, g->tab.cdt.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(g->d_cdt);
    return hipfail(ctx, e, "gauss table upload");
  }
  const std::vector<uint16_t> lut = gauss_bucket_table(g->tab.cdt.data(), g->tab.words, g->tab.entries);
  if (!lut.empty()) {
    e = hipMalloc((void **)&g->d_lut, lut.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(g->d_lut, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(g->d_cdt);
      if (g->d_lut) (void)hipFree(g->d_lut);
      return hipfail(ctx, e, "gauss bucket table upload");
    }
  }
  *out = g.release();
  return NFLHIP_OK;
}

int nflhip_gauss_table(double sigma, unsigned security, unsigned samples, double center, long long *x_min, size_t *entries,
                       int *words, unsigned *bit_precision, double *tail, uint64_t *h_table, size_t cap_words) {
  GaussTable tab;
  std::string err;
  try {
    if (cached_gauss_table(sigma, security, samples, center, &tab, &err)) return fail(nullptr, NFLHIP_ERR_INVALID, err);
  } catch (const std::bad_alloc &) {
    return fail(nullptr, NFLHIP_ERR_NOMEM, "out of host memory while building the gaussian table");
  }
  if (x_min) *x_min = tab.x_min;
  if (entries) *entries = tab.entries;
  if (words) *words = tab.words;
  if (bit_precision) *bit_precision = tab.bit_precision;
  if (tail) *tail = tab.tail;
  if (h_table) {
    if (cap_words < tab.cdt.size()) return fail(nullptr, NFLHIP_ERR_INVALID, "output buffer too small");
    std::memcpy(h_table, tab.cdt.data(), tab.cdt.size() * sizeof(uint64_t));
  }
  return NFLHIP_OK;
}

int nflhip_gauss_set_draw_bits(nflhip_gauss *g, int bits) {
  if (!g || (bits != 64 && bits != 32)) return NFLHIP_ERR_INVALID;
  g->draw_bits = bits;
  return NFLHIP_OK;
}
int nflhip_gauss_draw_bits(const nflhip_gauss *g) { return g ? g->draw_bits : 0; }

int nflhip_gauss_destroy(nflhip_ctx *ctx, nflhip_gauss *g) {
  if (!g) return NFLHIP_OK;
  (void)ctx;  // never dereferenced: a FastGaussianNoise with static storage may outlive the context that built its table
  (void)hipSetDevice(g->device);
  if (g->d_cdt) (void)hipFree(g->d_cdt);
  if (g->d_lut) (void)hipFree(g->d_lut);
  delete g;
  return NFLHIP_OK;
}

int nflhip_gauss_info(const nflhip_gauss *g, long long *x_min, size_t *entries, int *words, unsigned *bit_precision,
                      double *tail, uint64_t *h_table) {
  if (!g) return NFLHIP_ERR_INVALID;
  if (x_min) *x_min = g->tab.x_min;
  if (entries) *entries = g->tab.entries;
  if (words) *words = g->tab.words;
  if (bit_precision) *bit_precision = g->tab.bit_precision;
  if (tail) *tail = g->tab.tail;
  if (h_table) std::memcpy(h_table, g->tab.cdt.data(), g->tab.cdt.size() * sizeof(uint64_t));
  return NFLHIP_OK;
}

int nflhip_sample_gauss_dev(nflhip_ctx *ctx, void *d, size_t first_poly, size_t batch, const nflhip_gauss *g,
                            uint64_t amplifier, const unsigned char *key, uint64_t stream_id, void *stream) {
  CHECK_CTX(ctx);
  if (!key || !g || (batch && !d)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (g->device != ctx->device) return fail(ctx, NFLHIP_ERR_INVALID, "gaussian table lives on another device");
  if (amplifier == 0) return fail(ctx, NFLHIP_ERR_INVALID, "amplifier must be positive");
  hipStream_t st = (hipStream_t)stream;
  const int w = g->tab.words, en = (int)g->tab.entries;
  const long long x0 = g->tab.x_min;
  hipError_t e = with_limb(ctx, [&](auto z) {
    typedef decltype(z) T;
    return launch_sample_gauss<T>(ctx->shape, ctx->tabs, (T *)d, first_poly, batch, g->d_cdt, w, en, x0, amplifier, key, stream_id, st, 0, 0, gauss_narrow(g), g->d_lut);
  });
  if (e != hipSuccess) return hipfail(ctx, e, "sample_gauss");
  return NFLHIP_OK;
}

static int gauss_small_any(nflhip_ctx *ctx, void *d_out, int format, size_t first_poly, size_t batch, const nflhip_gauss *g,
                           uint64_t amplifier, const unsigned char *key, uint64_t stream_id, void *stream, int seq_on,
                           uint64_t seq_stride) {
  CHECK_CTX(ctx);
  if (!key || !g || (batch && !d_out)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (g->device != ctx->device) return fail(ctx, NFLHIP_ERR_INVALID, "gaussian table lives on another device");
  if (amplifier == 0) return fail(ctx, NFLHIP_ERR_INVALID, "amplifier must be positive");
  if (format < NFLHIP_FMT_I8 || format > NFLHIP_FMT_I32) return fail(ctx, NFLHIP_ERR_INVALID, "the compact format is int8, int16 or int32");
  // every sample x * amplifier must fit the format and stay below every modulus (so that p + v is its residue)
  const long long lo = g->tab.x_min, hi = g->tab.x_min + (long long)g->tab.entries - 1;
  const uint64_t mag = (uint64_t)std::max(lo < 0 ? -lo : lo, hi < 0 ? -hi : hi);
  const uint64_t cap = format == NFLHIP_FMT_I8 ? 127u : format == NFLHIP_FMT_I16 ? 32767u : 2147483647u;
  if (amplifier > cap || mag > cap / amplifier) return fail(ctx, NFLHIP_ERR_INVALID, "the samples do not fit the compact format");
  for (uint64_t p : ctx->h_P)
    if (mag * amplifier >= p) return fail(ctx, NFLHIP_ERR_INVALID, "the samples are not below the modulus");
  hipError_t e = launch_gauss_small(ctx->shape, d_out, format, first_poly, batch, g->d_cdt, g->tab.words, (int)g->tab.entries,
                                    g->tab.x_min, amplifier, key, stream_id, (hipStream_t)stream, seq_on, seq_stride, gauss_narrow(g), g->d_lut);
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "sequence mode needs degree >= 8 (>= 16 under the 32-bit draw)");
  if (e != hipSuccess) return hipfail(ctx, e, "sample_gauss_small");
  return NFLHIP_OK;
}

int nflhip_sample_gauss_small_dev(nflhip_ctx *ctx, void *d_out, int format, size_t first_poly, size_t batch,
                                  const nflhip_gauss *g, uint64_t amplifier, const unsigned char *key, uint64_t stream_id,
                                  void *stream) {
  return gauss_small_any(ctx, d_out, format, first_poly, batch, g, amplifier, key, stream_id, stream, 0, 0);
}

int nflhip_sample_gauss_small_seq_dev(nflhip_ctx *ctx, void *d_out, int format, size_t batch, const nflhip_gauss *g,
                                      uint64_t amplifier, const unsigned char *key, uint64_t first_stream_id,
                                      uint64_t stream_id_stride, void *stream) {
  return gauss_small_any(ctx, d_out, format, 0, batch, g, amplifier, key, first_stream_id, stream, 1, stream_id_stride);
}

int nflhip_sample_gauss_small_multi_dev(nflhip_ctx *ctx, void *const *d_out, size_t count, int format, size_t batch, const nflhip_gauss *g,
                                        const uint64_t *amplifier, const unsigned char *key, const uint64_t *stream_id,
                                        const uint64_t *stream_id_stride, void *stream) {
  CHECK_CTX(ctx);
  if (!key || !g || !d_out || !amplifier || !stream_id) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (count < 1 || count > 4) return fail(ctx, NFLHIP_ERR_INVALID, "one to four draws per call");
  if (g->device != ctx->device) return fail(ctx, NFLHIP_ERR_INVALID, "gaussian table lives on another device");
  if (format < NFLHIP_FMT_I8 || format > NFLHIP_FMT_I32) return fail(ctx, NFLHIP_ERR_INVALID, "the compact format is int8, int16 or int32");
  const long long lo = g->tab.x_min, hi = g->tab.x_min + (long long)g->tab.entries - 1;
  const uint64_t mag = (uint64_t)std::max(lo < 0 ? -lo : lo, hi < 0 ? -hi : hi);
  const uint64_t cap = format == NFLHIP_FMT_I8 ? 127u : format == NFLHIP_FMT_I16 ? 32767u : 2147483647u;
  for (size_t j = 0; j < count; ++j) {   // (the checks of gauss_small_any, per draw)
    if (batch && !d_out[j]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
    if (amplifier[j] == 0) return fail(ctx, NFLHIP_ERR_INVALID, "amplifier must be positive");
    if (amplifier[j] > cap || mag > cap / amplifier[j]) return fail(ctx, NFLHIP_ERR_INVALID, "the samples do not fit the compact format");
    for (uint64_t p : ctx->h_P)
      if (mag * amplifier[j] >= p) return fail(ctx, NFLHIP_ERR_INVALID, "the samples are not below the modulus");
  }
  hipError_t e = launch_gauss_small_multi(ctx->shape, d_out, count, format, batch, g->d_cdt, g->tab.words, (int)g->tab.entries, g->tab.x_min,
                                          amplifier, key, stream_id, stream_id_stride, (hipStream_t)stream, gauss_narrow(g), g->d_lut);
  if (e == hipErrorNotSupported) return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "sequence mode needs degree >= 8 (>= 16 under the 32-bit draw)");
  if (e != hipSuccess) return hipfail(ctx, e, "sample_gauss_small_multi");
  return NFLHIP_OK;
}

int nflhip_gauss_noise_dev(nflhip_ctx *ctx, int64_t *d_out, uint64_t first_sample, size_t count, const nflhip_gauss *g,
                           const unsigned char *key, uint64_t stream_id, void *stream) {
  CHECK_CTX(ctx);
  if (!key || !g || (count && !d_out)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (g->device != ctx->device) return fail(ctx, NFLHIP_ERR_INVALID, "gaussian table lives on another device");
  hipError_t e = launch_gauss_noise((long long *)d_out, first_sample, count, g->d_cdt, g->tab.words, (int)g->tab.entries,
                                    g->tab.x_min, key, stream_id, (hipStream_t)stream, gauss_narrow(g));
  if (e != hipSuccess) return hipfail(ctx, e, "gauss_noise");
  return NFLHIP_OK;
}

// ---------------------------------------------------------------------------
// core::ntt / core::inv_ntt: the cyclic transform of single rows
// ---------------------------------------------------------------------------
static int row_child(nflhip_ctx *ctx, size_t cm, int inverse_tables, hipStream_t st, nflhip_ctx **out) {
  std::lock_guard<std::mutex> lk(ctx->row_mu);
  if (ctx->row_ctx.empty()) ctx->row_ctx.assign(2 * ctx->shape.nm, nullptr);
  nflhip_ctx *&slot = ctx->row_ctx[2 * cm + (inverse_tables ? 1 : 0)];
  if (!slot) {
    const int rc = child_create(ctx, 1, [cm](size_t) { return cm; }, inverse_tables ? 2 : 1, is_capturing(st),
                                "ntt_row: the first call for a (modulus, table set) creates its context, which a stream capture cannot do", &slot);
    if (rc) return rc;
  }
  *out = slot;
  return NFLHIP_OK;
}

int nflhip_ntt_row_dev(nflhip_ctx *ctx, void *d_rows, size_t cm, int mode, size_t rows, void *stream) {
  CHECK_CTX(ctx);
  if (cm >= ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "modulus index out of range");
  if (mode < 0 || mode > 3) return fail(ctx, NFLHIP_ERR_INVALID, "unknown row-transform mode");
  if (rows == 0) return NFLHIP_OK;
  if (!d_rows) return fail(ctx, NFLHIP_ERR_INVALID, "NULL data pointer");
  nflhip_ctx *child = nullptr;
  int rc = row_child(ctx, cm, mode & NFLHIP_ROW_INVERSE_TABLES, (hipStream_t)stream, &child);
  if (rc) return rc;
  auto bitrev = [&]() -> int {   // core::inv_ntt: permut, ntt, permut (core.hpp:549-554)
    if (!(mode & NFLHIP_ROW_BITREV_IO)) return NFLHIP_OK;
    hipError_t e = with_limb(ctx, [&](auto z) {
      typedef decltype(z) T;
      return launch_bitrev_rows<T>(ctx->shape, (T *)d_rows, rows, (hipStream_t)stream);
    });
    return e == hipSuccess ? NFLHIP_OK : hipfail(ctx, e, "ntt_row: bit reversal");
  };
  rc = bitrev();
  if (!rc) rc = nflhip_ntt_fwd_dev(child, d_rows, rows, stream);
  if (!rc) rc = bitrev();
  return rc;
}

// ---------------------------------------------------------------------------
// memory helpers
// ---------------------------------------------------------------------------
int nflhip_stream_create(nflhip_ctx *ctx, void **stream) {
  CHECK_CTX(ctx);
  if (!stream) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipStream_t s = nullptr;
  HIPCHK(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void *)s;
  return NFLHIP_OK;
}
int nflhip_stream_destroy(nflhip_ctx *ctx, void *stream) {
  CHECK_CTX(ctx);
  if (stream) HIPCHK(ctx, hipStreamDestroy((hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_memcpy_d2d(nflhip_ctx *ctx, void *d_dst, const void *d_src, size_t bytes, void *stream) {
  CHECK_CTX(ctx);
  HIPCHK(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_memset_dev(nflhip_ctx *ctx, void *d_dst, int byte, size_t bytes, void *stream) {
  CHECK_CTX(ctx);
  HIPCHK(ctx, hipMemsetAsync(d_dst, byte, bytes, (hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_broadcast_dev(nflhip_ctx *ctx, void *d_dst, const void *d_one, size_t count, void *stream) {
  CHECK_CTX(ctx);
  if (count && (!d_dst || !d_one)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipError_t e = launch_broadcast(d_dst, d_one, poly_bytes(ctx, 1), count, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(ctx, e, "broadcast");
  return NFLHIP_OK;
}
int nflhip_random_bytes(int device, unsigned char *h_out, size_t nbytes, const unsigned char *key, uint64_t stream_id) {
  if (nbytes == 0) return NFLHIP_OK;
  if (!h_out || !key) return fail(nullptr, NFLHIP_ERR_INVALID, "NULL argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, NFLHIP_ERR_NO_DEVICE, "no HIP device available (this engine has no CPU fallback)");
  HIPCHK(nullptr, hipSetDevice(device));
  const size_t nwords = (nbytes + 7) / 8;
  uint64_t *d = nullptr;
  HIPCHK(nullptr, hipMalloc((void **)&d, nwords * 8));
  hipError_t e = launch_random_words(d, 0, nwords, key, stream_id, nullptr);
  std::vector<uint64_t> tmp;
  if (e == hipSuccess && (nbytes & 7)) {
    tmp.resize(nwords);
    e = hipMemcpy(tmp.data(), d, nwords * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) memcpy(h_out, tmp.data(), nbytes);
  } else if (e == hipSuccess) {
    e = hipMemcpy(h_out, d, nbytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e != hipSuccess) return hipfail(nullptr, e, "random_bytes");
  return NFLHIP_OK;
}

int nflhip_malloc(nflhip_ctx *ctx, void **p, size_t bytes) {
  CHECK_CTX(ctx);
  if (!p) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  hipError_t e = hipMalloc(p, bytes ? bytes : 1);
  if (e == hipErrorOutOfMemory) return fail(ctx, NFLHIP_ERR_NOMEM, "hipMalloc: out of device memory");
  if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc");
  return NFLHIP_OK;
}
int nflhip_free(nflhip_ctx *ctx, void *p) {
  CHECK_CTX(ctx);
  if (p) HIPCHK(ctx, hipFree(p));
  return NFLHIP_OK;
}
int nflhip_memcpy_h2d(nflhip_ctx *ctx, void *d, const void *h, size_t bytes, void *stream) {
  CHECK_CTX(ctx);
  HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_memcpy_d2h(nflhip_ctx *ctx, void *h, const void *d, size_t bytes, void *stream) {
  CHECK_CTX(ctx);
  HIPCHK(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_stream_sync(nflhip_ctx *ctx, void *stream) {
  CHECK_CTX(ctx);
  HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
  return NFLHIP_OK;
}
int nflhip_stream_idle(nflhip_ctx *ctx, void *stream, int *idle) {
  CHECK_CTX(ctx);
  if (!idle) return fail(ctx, NFLHIP_ERR_INVALID, "idle is NULL");
  const hipError_t e = hipStreamQuery((hipStream_t)stream);
  if (e == hipErrorNotReady) (void)hipGetLastError();  // "not ready" is an answer, not an error: do not leave it for the next launch's check
  else if (e != hipSuccess) HIPCHK(ctx, e);
  *idle = e == hipSuccess ? 1 : 0;
  return NFLHIP_OK;
}

// ---------------------------------------------------------------------------
// in-library timing of the metric kernel: HIP events on the launch stream
// ---------------------------------------------------------------------------
int nflhip_time_polymul_dev(nflhip_ctx *ctx, void *c, const void *a, const void *b, size_t batch, int iters, void *stream,
                            float *ms_per_pass) {
  CHECK_CTX(ctx);
  if (!ms_per_pass || iters <= 0) return fail(ctx, NFLHIP_ERR_INVALID, "bad timing arguments");
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0, e1;
  HIPCHK(ctx, hipEventCreate(&e0));
  hipError_t he = hipEventCreate(&e1);
  if (he == hipSuccess) he = hipEventRecord(e0, st);
  if (he != hipSuccess) {
    (void)hipEventDestroy(e0);
    return hipfail(ctx, he, "timing events");
  }
  for (int i = 0; i < iters; ++i) {
    int rc = nflhip_polymul_dev(ctx, c, a, b, batch, stream);
    if (rc) {
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      return rc;
    }
  }
  float ms = 0.f;
  he = hipEventRecord(e1, st);
  if (he == hipSuccess) he = hipEventSynchronize(e1);
  if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (he != hipSuccess) return hipfail(ctx, he, "timing events");
  *ms_per_pass = ms / (float)iters;
  return NFLHIP_OK;
}

}  // extern "C"
