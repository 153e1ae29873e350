// ctx.h -- the context of include/nflhip.h and the error / staging helpers shared by the C-ABI translation units:
// api.hip (context, upload of the tables host_tables.cpp computes, device-pointer entry points) and api_host.hip (host-pointer entry points).  Not installed.
#pragma once
#include "../../include/nflhip.h"

#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

namespace nflhip {
int set_error(int code, const std::string &msg);  // api.hip: the calling thread's nflhip_last_error text
}

// A context-owned device buffer that calls on any stream share (api.hip ws_begin / ws_end / ws_free): it grows on demand, never while
// capturing, and successive calls are ordered on it by an event that is recorded and waited on outside any capture.
struct Workspace {
  void *buf = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  bool ev_valid = false;
};
// What a call while capturing may repeat (api.hip warm_covers / warm_note): per (k_special, alpha, plan | modes) the largest sizes
// served so far outside a capture -- up to three per family, the unused ones 0.
typedef std::map<std::array<size_t, 3>, std::array<size_t, 3>> WarmMap;
typedef std::map<std::array<size_t, 2>, struct nflhip_ctx *> ChildMap;

struct nflhip_ctx {
  int device = 0;
  nflhip::Shape shape{};
  nflhip::DevTables tabs{};
  size_t word = 8;  // bytes per limb
  // host-pointer path: staging buffers + private stream, serialised by a mutex
  std::mutex mu;
  hipStream_t hstream = nullptr;
  void *stage[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t stage_bytes[4] = {0, 0, 0, 0};
  // a staging buffer of up to kStageHostMax bytes is PINNED HOST memory the kernels read and write directly (one polynomial per call, the
  // nfl::poly surface: a 128 KiB operand crosses PCIe inside the kernel in less time than a copy engine needs to start); larger ones are device
  // memory filled by copies
  bool stage_host[4] = {false, false, false, false};
  bool flag_host = false;          // tabs.flag is pinned host memory
  // large host-pointer calls: a three-slot pipeline of pinned staging chunks (HostPipe, api_host.hip), created on first use
  struct HostPipe *pipe = nullptr;
  // scratch for the composed (non-fused) polymul path, per stream use is serialised by the caller
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  std::mutex scratch_mu;
  // large-row polymul pipeline: two helper streams so that the HBM-bound streaming passes of one
  // chunk overlap the VALU-bound fused kernel of another; ev_prev orders successive calls on the scratch
  hipStream_t aux[2] = {nullptr, nullptr};
  hipEvent_t ev_start = nullptr, ev_done[2] = {nullptr, nullptr};
  bool ev_prev_valid = false;
  hipEvent_t ev_scratch = nullptr;  // end of the last single-stream pipeline that used the scratch
  bool ev_scratch_valid = false;
  // any_eq / any_neq: every call owns one result slot (device int) for its memset + kernel + readback, so host
  // threads comparing on distinct streams never share a flag
  static constexpr int kCmpSlots = 32;
  std::mutex cmp_mu[kCmpSlots];
  int cmp_token[kCmpSlots] = {};   // the token of the slot's latest comparison (under its mutex)
  std::atomic<unsigned> cmp_next{0};
  // host copies for introspection
  std::vector<uint64_t> h_Q;                     // moduli_product limbs
  std::vector<std::vector<uint64_t>> h_lifting;  // lifting_integers[cm]
  std::vector<uint64_t> h_P;
  std::vector<uint64_t> h_roots, h_invk, h_phi;  // params<T>::primitive_roots / invkMaxPolyDegree, phi = 2n-th root per modulus
  int kmax_log2 = 0;
  // core::ntt(x, wtab, winvtab, p) (core.hpp:455-532) on the device: one single-modulus child context per
  // (modulus, table set) whose twiddle table is the CYCLIC one, created on first use -- see nflhip_ntt_row_dev
  int cyclic = 0;  // 0: negacyclic tables (the normal context); 1 / 2: cyclic over omega / omega^-1 (child contexts)
  std::mutex row_mu;
  std::vector<nflhip_ctx *> row_ctx;  // [2 * cm + inverse_tables]
  // composed NTT-form rescale (api.hip rescale_composed): child contexts over the last modulus alone and over the first nm - 1,
  // created on first use, never while capturing, and the workspace that holds the inverse-transformed dropped rows.  Under resc_mu.
  std::mutex resc_mu;
  nflhip_ctx *resc_last = nullptr, *resc_kept = nullptr;
  Workspace resc_ws;
  // RNS base conversion / mod-down (api.hip baseconv_record): the device record of every pair of row ranges used so far, keyed by
  // (s0, ks, d0, kd, moddown); built and uploaded on first use under bconv_mu, freed with the context
  std::mutex bconv_mu;
  std::map<std::array<size_t, 5>, void *> bconv;
  // composed NTT-form base conversion / mod-down (api.hip baseconv_ntt_composed): child contexts over row ranges of this one,
  // keyed by (first row, count) and created on first use; workspace 0 holds the gathered source rows [batch][ks][n], workspace 1 the
  // converted rows of a destination range that is not the whole context; calls are ordered on both by the event of workspace 0 (the
  // event of workspace 1 is never created).  All under bcn_mu.
  std::mutex bcn_mu;
  ChildMap bcn_child;
  Workspace bcn_ws[2];
  // leveled key switching / multiplication (api.hip level_child): the context over the rows [0, level) and [nm - k_special, nm) of
  // this one, keyed by (k_special, level), created on first use, never while capturing, destroyed with this context; its records,
  // workspaces and warm maps are its own.  Under bcn_mu.
  ChildMap lvl_child;
  // hybrid key switching (api.hip keyswitch_run): per (k_special, alpha) the device array of its digits' record pointers; the warm
  // map's size is the batch; one workspace for the embedded / inverse-transformed input, the mod-upped digits and the two sums.  All
  // under ks_mu.
  std::mutex ks_mu;
  std::map<std::array<size_t, 2>, void *> ks_recs;
  WarmMap ks_warm;
  Workspace ks_ws;
  // hoisted rotations (api.hip rotate_run): the warm map's sizes are the batch and count * batch; one workspace for the mod-up's
  // input, the digits, the sums and the mod-down's result (the sequence: one key switch's two results).  All under rot_mu, which is
  // taken BEFORE ks_mu and bcn_mu.
  std::mutex rot_mu;
  WarmMap rot_warm;
  Workspace rot_ws;
  // slot linear transforms (api.hip lintrans_run): the warm map's sizes are the batch, keyed * batch and the polynomials of one
  // mod-down call; one workspace for the mod-up's input, the digits, the key-switch sums and the two accumulated sums.  All under
  // lt_mu, which is taken BEFORE ks_mu and bcn_mu.
  std::mutex lt_mu;
  WarmMap lt_warm;
  Workspace lt_ws;
  // BSGS slot linear transforms (api.hip bsgs_run): the warm map's key carries, next to (k_special, alpha), the plan, the modes and the
  // kinds of steps (keyed babies or none, keyed giants or none, c0 or none); its sizes are the batch, the polynomials of a group's
  // mod-down and mod-up (min(4, keyed giants) * batch; the sequence: batch) and the polynomials of the last mod-down call -- what the
  // calls underneath allocate by.  More keyed babies or giant steps than before only grow the workspace, which ws_begin refuses
  // while capturing, before anything is enqueued.  One workspace for both mod-ups, the babies' key-switch sums, a group of giant
  // steps and the two accumulated sums.  All under bsgs_mu, which is taken BEFORE ks_mu and bcn_mu.
  std::mutex bsgs_mu;
  WarmMap bsgs_warm;
  Workspace bsgs_ws;
  // ciphertext multiplication (api.hip mulrelin_run): per k_special one device block -- nm pairs (pi_j = P mod p_j, its Shoup
  // companion; zeros on the special rows), then the constant polynomial [nm][n] that holds pi_j in every word of row j (the
  // sequence's one-term dot) -- built on the host at the first call for that k_special; the warm map's size is the batch; one
  // workspace for the tensor's components, the mod-up's input, the digits and the two sums.  All under mr_mu, which is taken BEFORE
  // ks_mu and bcn_mu.
  std::mutex mr_mu;
  std::map<size_t, void *> mr_pi;
  WarmMap mr_warm;
  Workspace mr_ws;
  // scale-and-round by t/Q (api.hip scale_round_record / scale_round_run): the device record of every (ks, t) used so far, built and
  // uploaded on first use under srec_mu, freed with the context; workspace 0 holds the inverse-transformed copy of an NTT-form input,
  // workspace 1 the words Y of the two-pass plan; calls are ordered on both by the event of workspace 0.  The workspaces under sr_mu,
  // which is taken BEFORE srec_mu and bcn_mu.
  std::mutex srec_mu, sr_mu;
  std::map<std::array<uint64_t, 2>, void *> srec;
  Workspace sr_ws[2];
  // BFV tensor product (api.hip nflhip_bfv_tensor_ntt_dev): one workspace for the embedded inputs, the tensor's three components on
  // nmoduli rows and, where the outputs do not follow each other in memory, the scaled components.  Under bfv_mu, which is taken
  // BEFORE sr_mu.
  std::mutex bfv_mu;
  Workspace bfv_ws;
};

void pipe_destroy(nflhip_ctx *ctx);  // api_host.hip: frees the context's host-pointer pipeline

inline int fail(const nflhip_ctx *ctx, int code, const std::string &msg) {
  (void)ctx;
  return nflhip::set_error(code, msg);
}
inline int hipfail(const nflhip_ctx *ctx, hipError_t e, const char *where) {
  return fail(ctx, e == hipErrorNoDevice || e == hipErrorInvalidDevice ? NFLHIP_ERR_NO_DEVICE : NFLHIP_ERR_HIP,
              std::string(where) + ": " + hipGetErrorString(e));
}
#define HIPCHK(ctx, call)                                   \
  do {                                                      \
    hipError_t _e = (call);                                 \
    if (_e != hipSuccess) return hipfail(ctx, _e, #call);   \
  } while (0)

inline int set_device(const nflhip_ctx *ctx) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return NFLHIP_OK;
}
#define CHECK_CTX(ctx)                                                \
  do {                                                                \
    if (!(ctx)) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL"); \
    int _rc = set_device(ctx);                                        \
    if (_rc) return _rc;                                              \
  } while (0)

inline size_t poly_bytes(const nflhip_ctx *ctx, size_t batch) { return batch * ctx->shape.nm * ctx->shape.n * ctx->word; }
inline bool bytes_overlap(const void *a, const void *b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}


// nflhip_rescale / nflhip_rescale_dev: every argument check, before any device use (`host`: the staged host-pointer variant)
inline int rescale_check(const nflhip_ctx *ctx, const void *out, const void *in, size_t batch, int form, bool host) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "rescale: a cyclic row context has no modulus chain");
  if (ctx->shape.nm < 2) return fail(ctx, NFLHIP_ERR_INVALID, "rescale needs at least two moduli");
  const int plan = form & (NFLHIP_RESCALE_COMPOSED | NFLHIP_RESCALE_FUSED), base = form & ~plan;  // a plan flag: NTT form only, one at most
  if ((base != NFLHIP_FORM_COEFF && base != NFLHIP_FORM_NTT) || (plan && base != NFLHIP_FORM_NTT) ||
      plan == (NFLHIP_RESCALE_COMPOSED | NFLHIP_RESCALE_FUSED))
    return fail(ctx, NFLHIP_ERR_INVALID, "unknown polynomial form");
  if (!ctx->tabs.resc) return fail(ctx, NFLHIP_ERR_INVALID, "rescale: the last modulus repeats an earlier one");
  if (batch == 0) return NFLHIP_OK;
  if (!out || !in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t row = ctx->shape.n * ctx->word, ib = batch * ctx->shape.nm * row, ob = ib - batch * row;
  const uintptr_t x = (uintptr_t)out, y = (uintptr_t)in;
  if (x < y + ib && y < x + ob) return fail(ctx, NFLHIP_ERR_INVALID, host ? "the output overlaps the input" : "the output overlaps the input (the strides differ: never in place)");
  return NFLHIP_OK;
}
// nflhip_dot_dev / nflhip_dot_ptrs_dev: every argument check, before any device use.  An operand's extent is the
// (groups - 1) group_stride + (terms - 1) term_stride + 1 polynomials from its ptr; the output may overlap no byte of it, and the
// addend is the output itself or apart from it.
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bbytes && y < x + abytes;
}
inline int dot_check_out(const nflhip_ctx *ctx, const void *out, size_t obytes, const void *addend) {
  if (addend && addend != out && ranges_overlap(out, obytes, addend, obytes))
    return fail(ctx, NFLHIP_ERR_INVALID, "dot: the addend overlaps the output without being the output");
  return NFLHIP_OK;
}
inline int dot_check(const nflhip_ctx *ctx, const void *out, const nflhip_dot_operand *a, const nflhip_dot_operand *b, const void *addend,
                     size_t groups, size_t terms, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "dot: not on a cyclic row context");
  if (flags & ~NFLHIP_DOT_UNTILED) return fail(ctx, NFLHIP_ERR_INVALID, "dot: unknown flag bits");
  if (terms == 0 || terms > nflhip::kDotMaxTerms) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the number of terms is out of range (1 to 2^31)");
  if (!a || !b) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (groups == 0) return NFLHIP_OK;
  if (!out || !a->ptr || !b->ptr) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t pb = poly_bytes(ctx, 1);
  size_t obytes;
  if (__builtin_mul_overflow(groups, pb, &obytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the output size overflows");
  for (const nflhip_dot_operand *x : {a, b}) {
    size_t g, t, polys, bytes;
    if (__builtin_mul_overflow(groups - 1, x->group_stride, &g) || __builtin_mul_overflow(terms - 1, x->term_stride, &t) ||
        __builtin_add_overflow(g, t, &polys) || __builtin_add_overflow(polys, (size_t)1, &polys) || __builtin_mul_overflow(polys, pb, &bytes))
      return fail(ctx, NFLHIP_ERR_INVALID, "dot: an operand's extent overflows");
    if (ranges_overlap(out, obytes, x->ptr, bytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the output overlaps an operand");
  }
  return dot_check_out(ctx, out, obytes, addend);
}
// nflhip_decompose_dev / nflhip_decompose / nflhip_gadget_mul_dev: every argument check, before any device use.  format < 0: gadget_mul
// (words out, no flags).  *obytes: the size of the output.
inline size_t decompose_terms(const nflhip_ctx *ctx, int w) {
  if (!ctx || ctx->cyclic) return 0;
  const int bits = ctx->shape.limb_bits - 2;
  if (w < 1 || w > bits - 1) return 0;
  return ctx->shape.nm * (size_t)((bits + w - 1) / w);
}
inline int decompose_check(const nflhip_ctx *ctx, const void *out, int format, const void *in, size_t batch, int w, int flags, size_t *obytes) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  const char *what = format < 0 ? "gadget_mul" : "decompose";
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": not on a cyclic row context");
  if (format < 0) format = NFLHIP_FMT_WORDS;
  if (format != NFLHIP_FMT_WORDS && format != NFLHIP_FMT_I8 && format != NFLHIP_FMT_I16 && format != NFLHIP_FMT_I32)
    return fail(ctx, NFLHIP_ERR_INVALID, "decompose: unknown output format");
  const int plan = flags & (NFLHIP_DECOMP_COMPOSED | NFLHIP_DECOMP_FUSED), form = flags & ~(plan | NFLHIP_DECOMP_SIGNED);
  if (form != NFLHIP_FORM_COEFF && form != NFLHIP_FORM_NTT) return fail(ctx, NFLHIP_ERR_INVALID, "decompose: unknown flag bits");
  if (plan == (NFLHIP_DECOMP_COMPOSED | NFLHIP_DECOMP_FUSED) || (plan && form != NFLHIP_FORM_NTT))  // a plan flag: NTT form only, one at most
    return fail(ctx, NFLHIP_ERR_INVALID, "decompose: a plan flag goes with the NTT form, one at most");
  if (form == NFLHIP_FORM_NTT && format != NFLHIP_FMT_WORDS) return fail(ctx, NFLHIP_ERR_INVALID, "decompose: the NTT form is for words output");
  const size_t terms = decompose_terms(ctx, w);
  const int wmax = format == NFLHIP_FMT_I8 ? 7 : format == NFLHIP_FMT_I16 ? 15 : format == NFLHIP_FMT_I32 ? 31 : ctx->shape.limb_bits - 3;
  if (terms == 0 || w > wmax)
    return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": the digit width is out of range (1 to modulus bits - 1; 7 / 15 / 31 for a compact format)");
  if (terms > 65535 || ctx->shape.nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": more than 65535 terms");
  if (batch == 0) return NFLHIP_OK;
  if (!out || !in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t esz = format == NFLHIP_FMT_WORDS ? ctx->word * ctx->shape.nm : (size_t)1 << (format - 1);  // bytes per coefficient of a term
  size_t polys, ob, ib;
  if (__builtin_mul_overflow(batch, terms, &polys) || __builtin_mul_overflow(polys, ctx->shape.n * esz, &ob) ||
      __builtin_mul_overflow(batch, poly_bytes(ctx, 1), &ib))
    return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": the output size overflows");
  if (ranges_overlap(out, ob, in, ib)) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": the output overlaps the input");
  if (obytes) *obytes = ob;
  return NFLHIP_OK;
}
// nflhip_baseconv_dev / nflhip_baseconv / nflhip_moddown_dev / nflhip_moddown: every argument check, before any device use.
// moddown: s0 = nm - k, ks = k, d0 = 0, kd = nm - k and the output is the dense [batch][kd][n], which may not overlap the input;
// otherwise the output is [batch][nm][n]: the input itself or apart from it.  (A repeated source modulus, or for the mod-down a kept
// modulus that repeats a dropped one, is found by the table builder, on the host as well: api.hip baseconv_record.)
inline int baseconv_check(const nflhip_ctx *ctx, const void *out, const void *in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd,
                          int flags, bool moddown) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  const char *what = moddown ? "moddown" : "baseconv";
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": a cyclic row context has no modulus chain");
  if (flags & ~(moddown ? NFLHIP_MODDOWN_FLOOR : NFLHIP_BASECONV_CENTERED)) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": unknown flag bits");
  const size_t nm = ctx->shape.nm;
  if (moddown && (ks == 0 || ks >= nm)) return fail(ctx, NFLHIP_ERR_INVALID, "moddown: k is out of range (1 to nmoduli - 1)");
  if (ks == 0 || kd == 0 || s0 >= nm || ks > nm - s0 || d0 >= nm || kd > nm - d0)
    return fail(ctx, NFLHIP_ERR_INVALID, "baseconv: a row range is empty or outside the context");
  if (nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": more than 65535 rows");
  if (batch == 0) return NFLHIP_OK;
  if (!out || !in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t row = ctx->shape.n * ctx->word;
  size_t ib, ob;
  if (__builtin_mul_overflow(batch, nm * row, &ib) || __builtin_mul_overflow(batch, (moddown ? kd : nm) * row, &ob))
    return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": the size overflows");
  if ((moddown || out != in) && ranges_overlap(out, ob, in, ib))
    return fail(ctx, NFLHIP_ERR_INVALID, moddown ? "moddown: the output overlaps the input (the strides differ: never in place)"
                                                 : "baseconv: the output overlaps the input without being the input");
  return NFLHIP_OK;
}
// the NTT-form entries: the same checks, after the plan flags (one at most) are taken off
inline int baseconv_ntt_check(const nflhip_ctx *ctx, const void *out, const void *in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd,
                              int flags, bool moddown) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  const int plan = flags & (NFLHIP_BASECONV_NTT_COMPOSED | NFLHIP_BASECONV_NTT_FUSED);
  if (plan == (NFLHIP_BASECONV_NTT_COMPOSED | NFLHIP_BASECONV_NTT_FUSED))
    return fail(ctx, NFLHIP_ERR_INVALID, moddown ? "moddown_ntt: one plan flag at most" : "baseconv_ntt: one plan flag at most");
  return baseconv_check(ctx, out, in, batch, s0, ks, d0, kd, flags & ~plan, moddown);
}
// nflhip_keyswitch_ntt_dev / nflhip_keyswitch_ntt: every argument check short of the tables (a repeated modulus is found by their
// builder, api.hip keyswitch_records), before any device use
inline size_t keyswitch_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha) {
  if (!ctx || ctx->cyclic) return 0;
  const size_t nm = ctx->shape.nm;
  if (k_special == 0 || k_special >= nm || alpha == 0 || alpha > nm - k_special) return 0;
  return (nm - k_special + alpha - 1) / alpha;
}
// the level entries: the level against the context, ahead of the checks of the top-level entries (which then take the level)
inline size_t keyswitch_level_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha, size_t level) {
  if (keyswitch_digits(ctx, k_special, alpha) == 0 || level == 0 || level > ctx->shape.nm - k_special) return 0;
  return (level + alpha - 1) / alpha;
}
inline int level_check(const nflhip_ctx *ctx, size_t k_special, size_t level, const char *what) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": a cyclic row context has no modulus chain");
  if (k_special == 0 || k_special >= ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": k_special is out of range (1 to nmoduli - 1)");
  if (level == 0 || level > ctx->shape.nm - k_special) return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": the level is out of range (1 to nmoduli - k_special)");
  return NFLHIP_OK;
}
// The head of the checks of the four entries over a (k_special, alpha) key (`what`): the context, the flag bits against the entry's
// plan and mode masks, one plan flag at most, then -- where the entry counts keys -- `count_error`, the message of a count out of
// range (NULL: in range), then k_special, alpha and the rows.
inline int keyswitch_family_check(const nflhip_ctx *ctx, const char *what, int flags, int plans, int modes, const char *count_error,
                                  size_t k_special, size_t alpha) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  const std::string w(what);
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, w + ": a cyclic row context has no modulus chain");
  const int plan = flags & plans;
  if (flags & ~(plans | modes)) return fail(ctx, NFLHIP_ERR_INVALID, w + ": unknown flag bits");
  if (plan & (plan - 1)) return fail(ctx, NFLHIP_ERR_INVALID, w + ": one plan flag at most");
  if (count_error) return fail(ctx, NFLHIP_ERR_INVALID, count_error);
  const size_t nm = ctx->shape.nm;
  if (k_special == 0 || k_special >= nm) return fail(ctx, NFLHIP_ERR_INVALID, w + ": k_special is out of range (1 to nmoduli - 1)");
  if (keyswitch_digits(ctx, k_special, alpha) == 0) return fail(ctx, NFLHIP_ERR_INVALID, w + ": alpha is out of range (1 to nmoduli - k_special)");
  if (nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, w + ": more than 65535 rows");
  return NFLHIP_OK;
}
// (level: the operands' rows and the digits of a call below the top level, 1 <= level <= L checked by level_check; 0: the top level)
inline int keyswitch_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *in, const void *key, size_t batch,
                           size_t k_special, size_t alpha, int flags, size_t level = 0) {
  int rc = keyswitch_family_check(ctx, "keyswitch", flags, NFLHIP_KEYSWITCH_COMPOSED | NFLHIP_KEYSWITCH_FUSED | NFLHIP_KEYSWITCH_SEQUENCE,
                                  NFLHIP_KEYSWITCH_CENTERED | NFLHIP_KEYSWITCH_FLOOR, nullptr, k_special, alpha);
  if (rc || batch == 0) return rc;
  const size_t nm = ctx->shape.nm, dnum = keyswitch_digits(ctx, k_special, alpha);
  if (!out0 || !out1 || !in || !key) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t row = ctx->shape.n * ctx->word, L = level ? level : nm - k_special, kd = level ? (level + alpha - 1) / alpha : dnum;
  size_t ob, sb, kb, polys;
  // (sb: the largest scratch of any plan -- the embedded input, the digits and the two sums, [batch][1 + dnum + 2][nm][n])
  if (__builtin_mul_overflow(batch, L * row, &ob) || __builtin_mul_overflow(batch, dnum + 3, &polys) || __builtin_mul_overflow(polys, nm * row, &sb) ||
      __builtin_mul_overflow(2 * kd, nm * row, &kb))  // (kb: the digits that are read)
    return fail(ctx, NFLHIP_ERR_INVALID, "keyswitch: the size overflows");
  const void *const ptr[4] = {out0, out1, in, key};
  const size_t len[4] = {ob, ob, ob, kb};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      if (ranges_overlap(ptr[a], len[a], ptr[b], len[b])) return fail(ctx, NFLHIP_ERR_INVALID, "keyswitch: out0, out1, in and key may not overlap");
  return NFLHIP_OK;
}
// nflhip_dot_multi_dev: every argument check, before any device use.  Every output against the extent of a, of every b_o and against
// every other output; the b pointers may alias each other.
inline int dot_multi_check(const nflhip_ctx *ctx, void *const *outs, const nflhip_dot_operand *a, const void *const *bs, size_t b_ts,
                           size_t outputs, size_t groups, size_t terms, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: not on a cyclic row context");
  if (flags & ~NFLHIP_DOT_UNTILED) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: unknown flag bits");
  if (outputs == 0 || outputs > NFLHIP_DOT_MULTI_MAX_OUTPUTS) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: the number of outputs is out of range (1 to 32)");
  if (terms == 0 || terms > nflhip::kDotMaxTerms) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: the number of terms is out of range (1 to 2^31)");
  if (!a || !outs || !bs) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (groups == 0) return NFLHIP_OK;
  if (!a->ptr) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t o = 0; o < outputs; ++o)
    if (!outs[o] || !bs[o]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t pb = poly_bytes(ctx, 1);
  size_t obytes, g, t, polys, abytes, bbytes;
  if (__builtin_mul_overflow(groups, pb, &obytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: the output size overflows");
  if (__builtin_mul_overflow(groups - 1, a->group_stride, &g) || __builtin_mul_overflow(terms - 1, a->term_stride, &t) ||
      __builtin_add_overflow(g, t, &polys) || __builtin_add_overflow(polys, (size_t)1, &polys) || __builtin_mul_overflow(polys, pb, &abytes) ||
      __builtin_mul_overflow(terms - 1, b_ts, &t) || __builtin_add_overflow(t, (size_t)1, &polys) || __builtin_mul_overflow(polys, pb, &bbytes))
    return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: an operand's extent overflows");
  for (size_t o = 0; o < outputs; ++o) {
    if (ranges_overlap(outs[o], obytes, a->ptr, abytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: an output overlaps an operand");
    for (size_t q = 0; q < outputs; ++q) {
      if (ranges_overlap(outs[o], obytes, bs[q], bbytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: an output overlaps an operand");
      if (q < o && ranges_overlap(outs[o], obytes, outs[q], obytes)) return fail(ctx, NFLHIP_ERR_INVALID, "dot_multi: two outputs overlap");
    }
  }
  return NFLHIP_OK;
}
// nflhip_rotate_hoisted_ntt_dev / nflhip_rotate_hoisted_ntt: every argument check short of the tables (a repeated modulus is found by
// their builder, api.hip keyswitch_records), before any device use
inline int rotate_check(const nflhip_ctx *ctx, void *const *out0s, void *const *out1s, const void *c0, const void *c1, const void *const *keys,
                        const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags, size_t level = 0) {
  int rc = keyswitch_family_check(ctx, "rotate", flags, NFLHIP_ROTATE_SEQUENCE | NFLHIP_ROTATE_HOISTED, NFLHIP_ROTATE_CENTERED | NFLHIP_ROTATE_FLOOR,
                                  count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS ? "rotate: the number of rotations is out of range (1 to 16)" : nullptr,
                                  k_special, alpha);
  if (rc || batch == 0) return rc;
  const size_t nm = ctx->shape.nm, dnum = keyswitch_digits(ctx, k_special, alpha);
  if (!ks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL multiplier array");
  for (size_t m = 0; m < count; ++m)
    if ((ks[m] & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "rotate: the exponent k must be odd");
  if (!out0s || !out1s || !c1 || !keys) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t m = 0; m < count; ++m)
    if (!out0s[m] || !out1s[m] || !keys[m]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  // (level: as keyswitch_check)
  const size_t row = ctx->shape.n * ctx->word, L = level ? level : nm - k_special, kd = level ? (level + alpha - 1) / alpha : dnum;
  size_t ob, sb, kb, polys;
  // (sb: the largest scratch of either plan -- [batch][1 + dnum + 4 count][nm][n] -- on top of the key switch's own; kb: the digits that are read)
  if (__builtin_mul_overflow(batch, L * row, &ob) || __builtin_mul_overflow(batch, dnum + 3 + 4 * count, &polys) ||
      __builtin_mul_overflow(polys, nm * row, &sb) || __builtin_mul_overflow(2 * kd, nm * row, &kb))
    return fail(ctx, NFLHIP_ERR_INVALID, "rotate: the size overflows");
  for (size_t m = 0; m < 2 * count; ++m) {
    const void *o = m < count ? out0s[m] : out1s[m - count];
    if ((c0 && ranges_overlap(o, ob, c0, ob)) || ranges_overlap(o, ob, c1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "rotate: an output overlaps c0 or c1");
    for (size_t q = 0; q < count; ++q)
      if (ranges_overlap(o, ob, keys[q], kb)) return fail(ctx, NFLHIP_ERR_INVALID, "rotate: an output overlaps a key");
    for (size_t q = 0; q < m; ++q)
      if (ranges_overlap(o, ob, q < count ? out0s[q] : out1s[q - count], ob)) return fail(ctx, NFLHIP_ERR_INVALID, "rotate: two outputs overlap");
  }
  return NFLHIP_OK;
}
// nflhip_automorphism_mac_dev / nflhip_automorphism_mac: every argument check, before any device use
inline int mac_check(const nflhip_ctx *ctx, const void *out, const void *addend, const void *const *ins, const void *const *weights,
                     const uint64_t *ks, size_t terms, size_t batch, size_t rows, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: not on a cyclic row context");
  if (flags & ~NFLHIP_MAC_DOUBLE_BUFFER) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: unknown flag bits");
  if (terms == 0 || terms > NFLHIP_MAC_MAX_TERMS) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: the number of terms is out of range (1 to 16)");
  if (rows == 0 || rows > ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: rows is out of range (1 to nmoduli)");
  if (batch == 0) return NFLHIP_OK;
  if (!ks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL multiplier array");
  for (size_t t = 0; t < terms; ++t)
    if ((ks[t] & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: the exponent k must be odd");
  if (!out || !ins || !weights) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t t = 0; t < terms; ++t)
    if (!ins[t] || !weights[t]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t row = ctx->shape.n * ctx->word, wb = rows * row;
  size_t ob;
  if (__builtin_mul_overflow(batch, wb, &ob)) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: the size overflows");
  if (addend && addend != out && ranges_overlap(out, ob, addend, ob))
    return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: the addend overlaps the output without being the output");
  for (size_t t = 0; t < terms; ++t)
    if (ranges_overlap(out, ob, ins[t], ob) || ranges_overlap(out, ob, weights[t], wb))
      return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac: the output overlaps an input or a weight");
  return NFLHIP_OK;
}
// nflhip_lintrans_ntt_dev / nflhip_lintrans_ntt: every argument check short of the tables (a repeated modulus is found by their
// builder, api.hip keyswitch_records), before any device use
inline int lintrans_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *c0, const void *c1, const void *const *keys,
                          const void *const *weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags,
                          size_t level = 0) {
  int rc = keyswitch_family_check(ctx, "lintrans", flags, NFLHIP_LINTRANS_SEQUENCE | NFLHIP_LINTRANS_HOISTED, NFLHIP_LINTRANS_CENTERED | NFLHIP_LINTRANS_FLOOR,
                                  count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS ? "lintrans: the number of terms is out of range (1 to 16)" : nullptr,
                                  k_special, alpha);
  if (rc || batch == 0) return rc;
  const size_t nm = ctx->shape.nm, dnum = keyswitch_digits(ctx, k_special, alpha);
  if (!ks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL multiplier array");
  for (size_t m = 0; m < count; ++m)
    if ((ks[m] & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: the exponent k must be odd");
  if (!out0 || !out1 || !c1 || !keys || !weights) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t m = 0; m < count; ++m) {
    if (!weights[m]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    if (!keys[m] && (ks[m] & (2 * ctx->shape.n - 1)) != 1)
      return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: a NULL key goes with k = 1 mod 2 degree only (the unrotated diagonal)");
  }
  // (level: as keyswitch_check; a weight is a whole polynomial of this context at every level)
  const size_t row = ctx->shape.n * ctx->word, L = level ? level : nm - k_special, wb = nm * row, kd = level ? (level + alpha - 1) / alpha : dnum;
  size_t ob, sb, kb, polys;
  // (sb: the largest scratch of either plan -- [batch][dnum + 6 + 2 count][nm][n]; kb: the digits that are read)
  if (__builtin_mul_overflow(batch, L * row, &ob) || __builtin_mul_overflow(batch, dnum + 6 + 2 * count, &polys) ||
      __builtin_mul_overflow(polys, wb, &sb) || __builtin_mul_overflow(2 * kd, wb, &kb))
    return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: the size overflows");
  if (ranges_overlap(out0, ob, out1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: the two outputs overlap");
  for (const void *o : {out0, out1}) {
    if ((c0 && ranges_overlap(o, ob, c0, ob)) || ranges_overlap(o, ob, c1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: an output overlaps c0 or c1");
    for (size_t m = 0; m < count; ++m) {
      if (keys[m] && ranges_overlap(o, ob, keys[m], kb)) return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: an output overlaps a key");
      if (ranges_overlap(o, ob, weights[m], wb)) return fail(ctx, NFLHIP_ERR_INVALID, "lintrans: an output overlaps a weight");
    }
  }
  return NFLHIP_OK;
}
// nflhip_automorphism_mac_multi_dev / nflhip_automorphism_mac_multi: every argument check, before any device use.  weights =
// [outputs][terms], a NULL entry the zero weight; every overlap of an output with an input, a weight or another output is refused
inline int mac_multi_check(const nflhip_ctx *ctx, void *const *outs, const void *const *addends, const void *const *ins, const void *const *weights,
                           const uint64_t *ks, size_t outputs, size_t terms, size_t batch, size_t rows, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: not on a cyclic row context");
  if (flags) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: unknown flag bits");
  if (outputs == 0 || outputs > NFLHIP_MAC_MULTI_MAX_OUTPUTS) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: the number of outputs is out of range (1 to 16)");
  if (terms == 0 || terms > NFLHIP_MAC_MAX_TERMS) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: the number of terms is out of range (1 to 16)");
  if (rows == 0 || rows > ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: rows is out of range (1 to nmoduli)");
  if (batch == 0) return NFLHIP_OK;
  if (!ks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL multiplier array");
  for (size_t t = 0; t < terms; ++t)
    if ((ks[t] & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: the exponent k must be odd");
  if (!outs || !ins || !weights) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t t = 0; t < terms; ++t)
    if (!ins[t]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t o = 0; o < outputs; ++o) {
    if (!outs[o]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    if (addends && addends[o] && addends[o] != outs[o])
      return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: an addend is NULL or exactly its output");
  }
  const size_t row = ctx->shape.n * ctx->word, wb = rows * row;
  size_t ob;
  if (__builtin_mul_overflow(batch, wb, &ob)) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: the size overflows");
  for (size_t o = 0; o < outputs; ++o) {
    for (size_t t = 0; t < terms; ++t)
      if (ranges_overlap(outs[o], ob, ins[t], ob)) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: an output overlaps an input");
    for (size_t q = 0; q < outputs * terms; ++q)
      if (weights[q] && ranges_overlap(outs[o], ob, weights[q], wb)) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: an output overlaps a weight");
    for (size_t q = 0; q < o; ++q)
      if (ranges_overlap(outs[o], ob, outs[q], ob)) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism_mac_multi: two outputs overlap");
  }
  return NFLHIP_OK;
}
// nflhip_bsgs_ntt_dev / nflhip_bsgs_ntt: every argument check short of the tables, before any device use.  weights = [n2][n1], a NULL
// entry the zero diagonal; every giant step has a weight.  The operands have `level` rows, a weight is a whole polynomial of this
// context, and of a key the first ceil(level / alpha) digits are read.
inline int bsgs_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *c0, const void *c1, const void *const *bkeys,
                      const uint64_t *bks, size_t n1, const void *const *gkeys, const uint64_t *gks, size_t n2, const void *const *weights,
                      size_t batch, size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = keyswitch_family_check(ctx, "bsgs", flags, NFLHIP_BSGS_SEQUENCE | NFLHIP_BSGS_HOISTED, NFLHIP_BSGS_CENTERED | NFLHIP_BSGS_FLOOR,
                                  n1 == 0 || n1 > NFLHIP_BSGS_MAX_BABY   ? "bsgs: the number of baby steps is out of range (1 to 16)"
                                  : n2 == 0 || n2 > NFLHIP_BSGS_MAX_GIANT ? "bsgs: the number of giant steps is out of range (1 to 16)"
                                                                          : nullptr,
                                  k_special, alpha);
  if (!rc) rc = level_check(ctx, k_special, level, "bsgs");
  if (rc || batch == 0) return rc;
  const size_t nm = ctx->shape.nm, two_n = 2 * ctx->shape.n;
  if (!bks || !gks) return fail(ctx, NFLHIP_ERR_INVALID, "NULL multiplier array");
  if (!out0 || !out1 || !c1 || !bkeys || !gkeys || !weights) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  for (size_t m = 0; m < n1 + n2; ++m) {
    const uint64_t k = m < n1 ? bks[m] : gks[m - n1];
    const void *key = m < n1 ? bkeys[m] : gkeys[m - n1];
    if ((k & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: the exponent k must be odd");
    if (!key && (k & (two_n - 1)) != 1) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: a NULL key goes with k = 1 mod 2 degree only (the unrotated step)");
  }
  for (size_t j = 0; j < n2; ++j) {
    bool any = false;
    for (size_t i = 0; i < n1; ++i) any = any || weights[j * n1 + i];
    if (!any) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: a giant step has no diagonal");
  }
  const size_t row = ctx->shape.n * ctx->word, wb = nm * row, kd = (level + alpha - 1) / alpha, dnum = keyswitch_digits(ctx, k_special, alpha);
  size_t ob, sb, kb, polys;
  // (sb: beyond the largest scratch of either plan, in polynomials of nmoduli rows; kb: the digits that are read)
  if (__builtin_mul_overflow(batch, level * row, &ob) || __builtin_mul_overflow(batch, 8 * (dnum + 8) + 2 * n1 + n2, &polys) ||
      __builtin_mul_overflow(polys, wb, &sb) || __builtin_mul_overflow(2 * kd, wb, &kb))
    return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: the size overflows");
  if (ranges_overlap(out0, ob, out1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: the two outputs overlap");
  for (const void *o : {out0, out1}) {
    if ((c0 && ranges_overlap(o, ob, c0, ob)) || ranges_overlap(o, ob, c1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: an output overlaps c0 or c1");
    for (size_t m = 0; m < n1 + n2; ++m) {
      const void *key = m < n1 ? bkeys[m] : gkeys[m - n1];
      if (key && ranges_overlap(o, ob, key, kb)) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: an output overlaps a key");
    }
    for (size_t q = 0; q < n1 * n2; ++q)
      if (weights[q] && ranges_overlap(o, ob, weights[q], wb)) return fail(ctx, NFLHIP_ERR_INVALID, "bsgs: an output overlaps a weight");
  }
  return NFLHIP_OK;
}
// nflhip_tensor_ntt_dev / nflhip_tensor_ntt: every argument check, before any device use.  An output may be exactly an input (the
// same first byte); every other overlap of an output with an input or another output is refused.
inline int tensor_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *out2, const void *a0, const void *a1,
                        const void *b0, const void *b1, size_t batch, size_t rows, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: not on a cyclic row context");
  if (flags) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: unknown flag bits");
  if (rows == 0 || rows > ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: rows is out of range (1 to nmoduli)");
  if (ctx->shape.nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: more than 65535 rows");
  if (batch == 0) return NFLHIP_OK;
  if (!out0 || !out1 || !out2 || !a0 || !a1) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (!b0 != !b1) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: b0 and b1 are both given, or both NULL for the square");
  size_t ob;
  if (__builtin_mul_overflow(batch, rows * ctx->shape.n * ctx->word, &ob)) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: the size overflows");
  const void *const outs[3] = {out0, out1, out2}, *const ins[4] = {a0, a1, b0, b1};
  for (int o = 0; o < 3; ++o) {
    for (int q = 0; q < o; ++q)
      if (ranges_overlap(outs[o], ob, outs[q], ob)) return fail(ctx, NFLHIP_ERR_INVALID, "tensor: two outputs overlap");
    for (int i = 0; i < 4; ++i)
      if (ins[i] && ins[i] != outs[o] && ranges_overlap(outs[o], ob, ins[i], ob))
        return fail(ctx, NFLHIP_ERR_INVALID, "tensor: an output overlaps an input without being that input");
  }
  return NFLHIP_OK;
}
// nflhip_mulrelin_ntt_dev / nflhip_mulrelin_ntt: every argument check short of the tables (a repeated modulus is found by their
// builder, api.hip keyswitch_records), before any device use
inline int mulrelin_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *a0, const void *a1, const void *b0,
                          const void *b1, const void *key, size_t batch, size_t k_special, size_t alpha, int flags, size_t level = 0) {
  int rc = keyswitch_family_check(ctx, "mulrelin", flags, NFLHIP_MULRELIN_SEQUENCE | NFLHIP_MULRELIN_MERGED | NFLHIP_MULRELIN_FUSED,
                                  NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_FLOOR | NFLHIP_MULRELIN_RESCALE, nullptr, k_special, alpha);
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, dnum = keyswitch_digits(ctx, k_special, alpha);
  // (level: as keyswitch_check)
  const size_t row = ctx->shape.n * ctx->word, L = level ? level : nm - k_special, kd = level ? (level + alpha - 1) / alpha : dnum;
  if ((flags & NFLHIP_MULRELIN_RESCALE) && L < 2)
    return fail(ctx, NFLHIP_ERR_INVALID, level ? "mulrelin: the rescale needs two kept moduli at least (level >= 2)"
                                               : "mulrelin: the rescale needs two kept moduli at least (nmoduli - k_special >= 2)");
  if (batch == 0) return NFLHIP_OK;
  if (!out0 || !out1 || !a0 || !a1 || !key) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (!b0 != !b1) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin: b0 and b1 are both given, or both NULL for the square");
  size_t ib, ob, sb, kb, polys;
  // (sb: the largest scratch of either plan -- [batch][dnum + 12][nm][n] and a polynomial)
  if (__builtin_mul_overflow(batch, L * row, &ib) || __builtin_mul_overflow(batch, dnum + 13, &polys) || __builtin_mul_overflow(polys, nm * row, &sb) ||
      __builtin_mul_overflow(2 * kd, nm * row, &kb))  // (kb: the digits that are read)
    return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin: the size overflows");
  ob = (flags & NFLHIP_MULRELIN_RESCALE) ? ib - batch * row : ib;
  if (ranges_overlap(out0, ob, out1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin: the two outputs overlap");
  const void *const ins[4] = {a0, a1, b0, b1};
  for (const void *o : {out0, out1}) {
    if (ranges_overlap(o, ob, key, kb)) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin: an output overlaps the key");
    for (int i = 0; i < 4; ++i)
      if (ins[i] && ins[i] != o && ranges_overlap(o, ob, ins[i], ib))
        return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin: an output overlaps an input without being that input");
  }
  return NFLHIP_OK;
}
// nflhip_tensor_dot_ntt_dev / nflhip_mulrelin_dot_ntt_dev: the four operands (b0 == b1 == NULL: the squares) against `nouts` outputs
// of obytes each.  An operand's extent is that of dot_check over polynomials of pbytes.  `at_start`: an output may begin exactly at
// an operand's first byte (the multiplication: every read is enqueued before the mod-down writes).
inline int tensor_dot_operands_check(const nflhip_ctx *ctx, const std::string &w, const void *const *outs, int nouts, size_t obytes,
                                     const nflhip_dot_operand *const *ops, size_t groups, size_t terms, size_t pbytes, bool at_start) {
  for (int q = 0; q < 4; ++q) {
    const nflhip_dot_operand *x = ops[q];
    if (!x) continue;
    if (!x->ptr) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    size_t g, t, polys, bytes;
    if (__builtin_mul_overflow(groups - 1, x->group_stride, &g) || __builtin_mul_overflow(terms - 1, x->term_stride, &t) ||
        __builtin_add_overflow(g, t, &polys) || __builtin_add_overflow(polys, (size_t)1, &polys) || __builtin_mul_overflow(polys, pbytes, &bytes))
      return fail(ctx, NFLHIP_ERR_INVALID, w + ": an operand's extent overflows");
    for (int o = 0; o < nouts; ++o)
      if (!(at_start && outs[o] == x->ptr) && ranges_overlap(outs[o], obytes, x->ptr, bytes))
        return fail(ctx, NFLHIP_ERR_INVALID, w + (at_start ? ": an output overlaps an operand without beginning at its first byte" : ": an output overlaps an operand"));
  }
  return NFLHIP_OK;
}
// nflhip_tensor_dot_ntt_dev: every argument check, before any device use
inline int tensor_dot_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *out2, const nflhip_dot_operand *a0,
                            const nflhip_dot_operand *a1, const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, size_t groups, size_t terms,
                            size_t rows, int flags) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: not on a cyclic row context");
  if (flags) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: unknown flag bits");
  if (terms == 0 || terms > nflhip::kDotMaxTerms) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: the number of terms is out of range (1 to 2^31)");
  if (rows == 0 || rows > ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: rows is out of range (1 to nmoduli)");
  if (ctx->shape.nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: more than 65535 rows");
  if (!a0 || !a1) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (!b0 != !b1) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: b0 and b1 are both given, or both NULL for the squares");
  if (groups == 0) return NFLHIP_OK;
  if (!out0 || !out1 || !out2) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t pbytes = rows * ctx->shape.n * ctx->word;
  size_t ob;
  if (__builtin_mul_overflow(groups, pbytes, &ob)) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: the output size overflows");
  const void *const outs[3] = {out0, out1, out2};
  for (int o = 0; o < 3; ++o)
    for (int q = 0; q < o; ++q)
      if (ranges_overlap(outs[o], ob, outs[q], ob)) return fail(ctx, NFLHIP_ERR_INVALID, "tensor_dot: two outputs overlap");
  const nflhip_dot_operand *const ops[4] = {a0, a1, b0, b1};
  return tensor_dot_operands_check(ctx, "tensor_dot", outs, 3, ob, ops, groups, terms, pbytes, false);
}
// nflhip_mulrelin_dot_ntt_dev: every argument check short of the tables, before any device use; after level_check (1 <= level <= L)
inline int mulrelin_dot_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                              const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, const void *key, size_t groups, size_t terms,
                              size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = keyswitch_family_check(ctx, "mulrelin_dot", flags, NFLHIP_MULRELIN_SEQUENCE | NFLHIP_MULRELIN_MERGED | NFLHIP_MULRELIN_FUSED,
                                  NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_FLOOR | NFLHIP_MULRELIN_RESCALE, nullptr, k_special, alpha);
  if (rc) return rc;
  if (terms == 0 || terms > nflhip::kDotMaxTerms) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: the number of terms is out of range (1 to 2^31)");
  if ((flags & NFLHIP_MULRELIN_RESCALE) && level < 2) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: the rescale needs two kept moduli at least (level >= 2)");
  if (!a0 || !a1) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  if (!b0 != !b1) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: b0 and b1 are both given, or both NULL for the squares");
  if (groups == 0) return NFLHIP_OK;
  if (!out0 || !out1 || !key) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, dnum = keyswitch_digits(ctx, k_special, alpha), kd = (level + alpha - 1) / alpha;
  size_t ib, ob, sb, kb, polys;
  // (sb: the largest scratch of either plan, as mulrelin_check)
  if (__builtin_mul_overflow(groups, level * row, &ib) || __builtin_mul_overflow(groups, dnum + 13, &polys) || __builtin_mul_overflow(polys, nm * row, &sb) ||
      __builtin_mul_overflow(2 * kd, nm * row, &kb))  // (kb: the digits that are read)
    return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: the size overflows");
  ob = (flags & NFLHIP_MULRELIN_RESCALE) ? ib - groups * row : ib;
  if (ranges_overlap(out0, ob, out1, ob)) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: the two outputs overlap");
  for (const void *o : {out0, out1})
    if (ranges_overlap(o, ob, key, kb)) return fail(ctx, NFLHIP_ERR_INVALID, "mulrelin_dot: an output overlaps the key");
  const void *const outs[2] = {out0, out1};
  const nflhip_dot_operand *const ops[4] = {a0, a1, b0, b1};
  return tensor_dot_operands_check(ctx, "mulrelin_dot", outs, 2, ob, ops, groups, terms, level * row, true);
}
// nflhip_scale_round_dev / _ntt_dev / nflhip_scale_round / _ntt: every argument check short of the tables (a repeated modulus is found by
// their builder, api.hip scale_round_record), before any device use.  *obytes: the size of the output.
inline int scale_round_args(const nflhip_ctx *ctx, const char *what, size_t ks, uint64_t t, int flags, int allowed) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  const std::string w(what);
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, w + ": a cyclic row context has no modulus chain");
  if (flags & ~allowed) return fail(ctx, NFLHIP_ERR_INVALID, w + ": unknown flag bits");
  if (ks == 0 || ks >= ctx->shape.nm) return fail(ctx, NFLHIP_ERR_INVALID, w + ": ks is out of range (1 to nmoduli - 1)");
  if (t == 0 || t >> (ctx->shape.limb_bits - 3)) return fail(ctx, NFLHIP_ERR_INVALID, w + ": t is out of range (1 to 2^(limb_bits - 3) - 1)");
  if (ctx->shape.nm > 65535) return fail(ctx, NFLHIP_ERR_INVALID, w + ": more than 65535 rows");
  return NFLHIP_OK;
}
inline int scale_round_check(const nflhip_ctx *ctx, const void *out, const void *in, size_t batch, size_t ks, uint64_t t, int flags, size_t *obytes) {
  int rc = scale_round_args(ctx, "scale_round", ks, t, flags, NFLHIP_SCALE_ROUND_FLOOR | NFLHIP_SCALE_ROUND_KEEP | NFLHIP_SCALE_ROUND_TWO_PASS);
  if (rc || batch == 0) return rc;
  if (!out || !in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, orows = (flags & NFLHIP_SCALE_ROUND_KEEP) ? nm - ks : ks;
  size_t ib, ob;
  if (__builtin_mul_overflow(batch, nm * row, &ib) || __builtin_mul_overflow(batch, orows * row, &ob))
    return fail(ctx, NFLHIP_ERR_INVALID, "scale_round: the size overflows");
  if (ranges_overlap(out, ob, in, ib)) return fail(ctx, NFLHIP_ERR_INVALID, "scale_round: the output overlaps the input (the strides differ: never in place)");
  if (obytes) *obytes = ob;
  return NFLHIP_OK;
}
// nflhip_bfv_tensor_ntt_dev / nflhip_bfv_tensor_ntt: the scale-round's own arguments, then the tensor product's on ks rows
inline int bfv_tensor_check(const nflhip_ctx *ctx, const void *out0, const void *out1, const void *out2, const void *a0, const void *a1,
                            const void *b0, const void *b1, size_t batch, size_t ks, uint64_t t, int flags) {
  int rc = scale_round_args(ctx, "bfv_tensor", ks, t, flags, NFLHIP_SCALE_ROUND_FLOOR | NFLHIP_SCALE_ROUND_TWO_PASS);
  if (rc) return rc;
  size_t polys, sb;  // (the scratch: [4 + 3][batch] polynomials of nmoduli rows and the scaled components)
  if (__builtin_mul_overflow(batch, (size_t)10, &polys) || __builtin_mul_overflow(polys, poly_bytes(ctx, 1), &sb))
    return fail(ctx, NFLHIP_ERR_INVALID, "bfv_tensor: the size overflows");
  return tensor_check(ctx, out0, out1, out2, a0, a1, b0, b1, batch, ks, 0);
}
constexpr size_t kStageHostMax = (size_t)1 << 20;
inline void free_stage(nflhip_ctx *ctx, int slot) {
  if (ctx->stage[slot]) (void)(ctx->stage_host[slot] ? hipHostFree(ctx->stage[slot]) : hipFree(ctx->stage[slot]));
  ctx->stage[slot] = nullptr;
  ctx->stage_bytes[slot] = 0;
  ctx->stage_host[slot] = false;
}
inline int ensure_stage(nflhip_ctx *ctx, int slot, size_t bytes) {
  if (ctx->stage_bytes[slot] >= bytes) return NFLHIP_OK;
  free_stage(ctx, slot);
  if (bytes <= kStageHostMax && hipHostMalloc(&ctx->stage[slot], bytes, hipHostMallocDefault) == hipSuccess) {
    ctx->stage_host[slot] = true;
  } else {   // (also when the pinned allocation is refused -- a locked-memory limit: the copies take over)
    (void)hipGetLastError();
    ctx->stage[slot] = nullptr;
    HIPCHK(ctx, hipMalloc(&ctx->stage[slot], bytes));
  }
  ctx->stage_bytes[slot] = bytes;
  return NFLHIP_OK;
}
