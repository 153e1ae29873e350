// kernels.h -- internal launch interface between the C-ABI layer (api.hip) and
// the gfx950 kernels.  Not installed; the public boundary is include/nflhip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "table_types.h"  // ModConst<T>, RescConst<T>, Tw<T>: the records host_tables.cpp computes

namespace nflhip {

struct Shape {
  int limb_bits;
  int logn;
  size_t n, nm;
  size_t crt_L;      // limbs of a lifted coefficient
  size_t crt_Lacc;   // limbs of the accumulator (L+1)
  uint64_t crt_Q0;   // the moduli product when it is below 2^64 (crt_L == 1), else its low word
  int small_delta;   // every modulus is 2^(W-2) - delta with delta < 2^32 (delta-form butterflies)
  int nm_small;      // length of the PREFIX of moduli with delta < 2^32 (== nm when small_delta): at degree 4096 these rows keep the
                     // delta-form kernels in a context whose later moduli need the general family (params.hpp:82-119: #92 on)
  // configuration, read ONCE when the context is created (include/nflhip.h "environment"):
  int compiled_only; // NFLHIP_VARIANT=hipcc: the compiled (hipcc) kernels serve every call -- the independent cross-check
                     // of the generated assembly kernels (bit-identical results, tests/test_gpu_variants.py)
  int plan;          // NFLHIP_XCD: rows of 32768 / 65536 words -- -1 by batch size (default), 0 never / 1 always the
                     // one-launch plan of persistent workgroups
};

// Device-resident tables of one context.
struct DevTables {
  void *psi;        // [nm][n] Tw<T>
  void *psi_lm;     // 64-bit limbs, n >= 4096: the same with the last four stages lane-major (what the generated kernels read)
  void *mc;         // [nm] ModConst<T>
  void *mc_inc[2];  // 64-bit limbs, n = 4096, delta-form moduli: the records the incomplete-transform products read (level 1, 2:
                    // (n / 2^level)^-1 in the n^-1 fields, floor(2^127 / p) - 2^65 in mu2; tools/asmgen/incomplete.py), or nullptr
  uint64_t *qhat;   // [nm][crt_Lacc]  Q/p_cm, little-endian limbs
  uint64_t *qsh;    // [6][crt_Lacc]   Q << k, k = 0..5
  uint32_t *qparts; // [nm][3][72]     32-bit digits of (Q/p_cm) << 21 j   (carry-free lift), or nullptr
  uint32_t *bparts; // [proj_K][2][3][nm rounded up to 4] 21-bit parts of 2^(64k+32h) mod p_cm (project), or nullptr
  int proj_K;       // input words the project table covers
  double inv_qtop;  // 2^(32 (2 crt_L - 3)) / Q in double precision (quotient estimate of the lift)
  int *flag;        // kCmpSlots ints: result slots of any_eq / any_neq (one per concurrent call, see api.hip)
  // CRT lift beyond the register-resident kernels (more than 32 moduli / 36 limbs): limb-serial kernel, any size
  uint64_t *qhat_w; // [nm][crt_Lw]   Q/p_cm, little-endian limbs, or nullptr when the fast tables cover the shape
  uint64_t *qsh_w;  // [crt_nsh][crt_Lw]  Q << k
  int crt_Lw, crt_nsh;
  // CRT lift on the matrix cores (kernels_crt_mfma.hip): 64-bit limbs, many moduli
  void *crt_bfrag;  // [8 K-steps][8 N-tiles][64 lanes][16] int8: balanced base-256 digits of Q/p_cm in B-fragment order, or nullptr
  void *crt_bproj;  // the same for the projection: digit t of 256^k mod p_cm, k = 32 s + 16 (lane >> 5) + byte, cm = lane & 31, or nullptr
  uint64_t *crt_c2048; // [32][2] 2^2048 mod p_cm and its Shoup companion: how the residue of an input's upper 32 words joins the lower words'
  uint64_t *crt_coff; // [32][2] 2^18 p_cm + 128 sum_k (256^k mod p_cm in those digits), 128 bits: what the projection adds before reducing
  void *resc;       // [nm - 1] RescConst<T>: the rescale by the last modulus, or nullptr with a single modulus
};

// ---- launchers (kernels_generic.hip) ----
template <typename T>
hipError_t launch_ntt_fwd(const Shape &s, const DevTables &t, const T *src, T *dst, size_t batch, hipStream_t st);
// inverse of (src (.) mul) when mul != nullptr (fused point-wise product), else of src
template <typename T>
hipError_t launch_ntt_inv(const Shape &s, const DevTables &t, const T *src, const T *mul, T *dst, size_t batch,
                          hipStream_t st);
template <typename T>
hipError_t launch_pointwise(const Shape &s, const DevTables &t, int op, T *out, const T *a, const T *b, const T *bp,
                            size_t batch, hipStream_t st);
// postfix expression program (include/nflhip.h NFLHIP_EXPR_*) over up to 8 operands, one fused pass
template <typename T>
hipError_t launch_eval_expr(const Shape &s, const DevTables &t, T *out, const void *const *operands, int noperands,
                            const unsigned char *program, int len, size_t batch, hipStream_t st,
                            const unsigned *strides = nullptr, unsigned out_stride = 1);  // strides in polynomials (0 = shared)
template <typename T>
hipError_t launch_any_cmp(const Shape &s, const DevTables &t, const T *a, const T *b, size_t batch, int want_eq,
                          int *flag, int token, hipStream_t st);   // a hit stores `token` into *flag (no clearing, no atomic)
template <typename T>
hipError_t launch_check_range(const Shape &s, const DevTables &t, const T *d, size_t batch, int *flag, int token, hipStream_t st);
template <typename T>
hipError_t launch_fill_uniform(const Shape &s, const DevTables &t, T *d, size_t first_poly, size_t batch, uint64_t seed,
                               int operand, hipStream_t st);
// Galois automorphisms (kernels_automorph.hip): outs[m] = sigma_{ks[m]}(in) for m < count <= 16, every k odd; ntt_form selects the
// NTT-form map (a permutation of the stored words) over the coefficient-form one (a signed permutation).  No output may overlap
// the input or another output (api.hip checks).  hipErrorInvalidValue for an even k or a count out of range
template <typename T>
hipError_t launch_automorphism(const Shape &s, const DevTables &t, T *const *outs, const uint64_t *ks, int count, const T *in,
                               int ntt_form, size_t batch, hipStream_t st);
// RNS rescale by the last modulus (kernels_rescale.hip; include/nflhip.h "RNS rescale"): in = [batch][nm][n], out = the dense
// [batch][nm - 1][n]; nm >= 2 and out must not overlap in (api.hip checks).  _coeff: the coefficient form, one streaming pass.
// _ntt_fused: the NTT form in ONE launch, a workgroup per polynomial with two rows in LDS; hipErrorNotSupported when two rows
// exceed 64 KiB.  The composed NTT-form plan (api.hip rescale_composed) runs the transform launchers between _expand (out row i =
// (h - r) mod p_i from the inverse-transformed dropped rows t = [batch][n], r = (t + h) mod q) and _combine (out row i =
// (in row i + out row i) q^-1 mod p_i).
template <typename T>
hipError_t launch_rescale_coeff(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st);
template <typename T>
hipError_t launch_rescale_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st);
template <typename T>
hipError_t launch_rescale_expand(const Shape &s, const DevTables &t, T *out, const T *dropped, size_t batch, hipStream_t st);
template <typename T>
hipError_t launch_rescale_combine(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, hipStream_t st);
// sums of products across polynomials (kernels_dot.hip; include/nflhip.h "sums of products"): out[g] = addend[g] + sum_j a(g,j) b(g,j),
// a(g,j) the polynomial at a + (g a_gs + j a_ts) polynomials (b alike), out and addend dense [groups][nm][n], addend nullptr or
// possibly out itself; out must not overlap a or b (api.hip checks).  tiled: when one operand is shared by all groups (group
// stride 0) and groups > 1, a thread serves 4 groups per load of the shared words.  _ptrs: one group, terms <= kDotMaxPointers
// HOST arrays of device pointers, which travel in the kernel arguments.
constexpr int kDotMaxPointers = 16;
constexpr size_t kDotMaxTerms = (size_t)1 << 31;  // the kernel counts terms in 32 bits, a few ahead: j + 4 must not wrap
template <typename T>
hipError_t launch_dot(const Shape &s, const DevTables &t, T *out, const T *a, size_t a_gs, size_t a_ts, const T *b, size_t b_gs, size_t b_ts,
                      const T *addend, size_t groups, size_t terms, int tiled, hipStream_t st);
template <typename T>
hipError_t launch_dot_ptrs(const Shape &s, const DevTables &t, T *out, const T *const *a, const T *const *b, size_t terms, const T *addend,
                           hipStream_t st);
// several outputs against one first operand (kernels_dot_multi.hip; include/nflhip.h "sums of products, several outputs"):
// outs[o][g] = sum_j a(g,j) b_o(j), a(g,j) at a + (g a_gs + j a_ts) polynomials, b_o(j) at bs[o] + j b_ts polynomials, every outs[o]
// dense [groups][nm][n]; outs / bs are HOST arrays of `outputs` <= kDotMultiMaxOutputs device pointers, which travel in the kernel
// arguments.  No output may overlap an operand or another output (api.hip checks).  tiled: two groups per load of b's words.
constexpr int kDotMultiMaxOutputs = 32;
template <typename T>
hipError_t launch_dot_multi(const Shape &s, const DevTables &t, T *const *outs, const T *a, size_t a_gs, size_t a_ts, const T *const *bs,
                            size_t b_ts, size_t outputs, size_t groups, size_t terms, int tiled, hipStream_t st);
// the last step of a hoisted rotation (kernels_rotate.hip; include/nflhip.h "hoisted rotations"): outs[p] = sigma^NTT_{ks[p]}(ins[p]
// [+ c0 when bit p of add_mask is set]) for p < pairs <= kRotateMaxPairs, every block [batch][L][n] in the dense layout over the
// first L moduli of the context (the sum is mod p_(row mod L)); c0 may be nullptr.  HOST arrays of device pointers, which travel in
// the kernel arguments.  No output may overlap an input, c0 or another output (api.hip checks).  hipErrorInvalidValue for an even k
constexpr int kRotateMaxPairs = 32;
template <typename T>
hipError_t launch_permute_add_ntt(const Shape &s, const DevTables &t, T *const *outs, const T *const *ins, const uint64_t *ks, unsigned add_mask,
                                  int pairs, const T *c0, size_t L, size_t batch, hipStream_t st);
// the weighted sum of NTT-form automorphisms (kernels_lintrans.hip; include/nflhip.h "weighted sums of automorphisms"): for every
// component c < comps, out + c out_cs = (addend + c out_cs) + sum_{t < terms} weights[t] (.) sigma^NTT_{ks[t]}(ins[t] + c in_cs), every
// block [batch][R][n] in the dense layout over the first R moduli of the context, weights[t] = [>= R][n]; the strides in words;
// addend nullptr or out itself or apart from it.  HOST arrays of device pointers, which travel in the kernel arguments.  out may
// overlap no input and no weight (api.hip checks).  double_buffer: two staging buffers instead of one (the measured alternative).
// hipErrorInvalidValue for an even k
constexpr int kMacMaxTerms = 16;
template <typename T>
hipError_t launch_permute_mac_ntt(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const T *const *weights,
                                  const uint64_t *ks, int terms, size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs,
                                  int double_buffer, hipStream_t st);
// gadget decomposition (kernels_decompose.hip; include/nflhip.h "gadget decomposition"): in = [batch][nm][n] canonical words in
// coefficient form, digit width 1 <= w <= limb_bits - 3, l = ceil((limb_bits - 2) / w), terms = nm l; sgn: balanced digits.
// _words: out = [batch][terms][nm][n], the digit spread over every row (coefficient form).  _compact: out = [batch][terms][n] of
// int8 / int16 / int32 (format 1 / 2 / 3; w <= 7 / 15 / 31).  _ntt_fused: the words output forward-transformed, ONE launch, a
// workgroup per output polynomial with one row in LDS; hipErrorNotSupported for rows beyond 32 KiB (api.hip then runs _words and
// the forward launcher in place).  launch_gadget_mul: out[b][(m, t)][m'] = in[b][m] 2^(w t) mod p_m for m' = m, else 0.
// out must not overlap in (api.hip checks).
template <typename T>
hipError_t launch_decompose_words(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, int sgn, hipStream_t st);
template <typename T>
hipError_t launch_decompose_compact(const Shape &s, const DevTables &t, void *out, int format, const T *in, size_t batch, int w, int sgn,
                                    hipStream_t st);
template <typename T>
hipError_t launch_decompose_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, int sgn, hipStream_t st);
template <typename T>
hipError_t launch_gadget_mul(const Shape &s, const DevTables &t, T *out, const T *in, size_t batch, int w, hipStream_t st);
// RNS base conversion and mod-down (kernels_baseconv.hip; include/nflhip.h "RNS base conversion"): rows [s0, s0 + ks) of in =
// [batch][nm][n] converted to rows [d0, d0 + kd) of out, coefficient form.  rec: the device copy of the pair's record
// (host_tables.h build_baseconv_record).  moddown: s0 + ks = nm, d0 = 0, kd = s0, out is the dense [batch][kd][n] and must not
// overlap in; otherwise out = [batch][nm][n], the same buffer as in or apart from it (api.hip checks).
template <typename T>
hipError_t launch_baseconv(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t s0, size_t ks,
                           size_t d0, size_t kd, int centred, int moddown, hipStream_t st);
// the same kernels on an input of `inm` rows per polynomial whose rows [0, ks) are the sources (a gathered, inverse-transformed
// copy of rows S: the composed NTT-form plans of api.hip), written to rows [d0, d0 + kd) of out = [batch][onm][n]; rec is the record
// of the pair in the CONTEXT's numbering (destination row j reduces under the context's modulus d0 + j).  out never is in.
template <typename T>
hipError_t launch_baseconv_rows(const Shape &s, const DevTables &t, T *out, size_t onm, const T *in, size_t inm, const uint64_t *rec, size_t batch,
                                size_t ks, size_t d0, size_t kd, int centred, hipStream_t st);
// RNS scale-and-round by t/Q (kernels_scale_round.hip; include/nflhip.h "BFV multiplication"): in = [batch][nm][n] coefficient form, S
// the first ks rows; out = the dense [batch][ks][n], or with `keep` the dense [batch][nm - ks][n] of the words Y.  rec: the device copy
// of build_scale_round_record (host_tables.h).  centred: the first conversion (the second always is).  chunked = 0: the register
// plans, hipErrorNotSupported where neither holds the rows (scale_round_in_registers); chunked = 1: keep only, any shape.  out never
// overlaps in (api.hip checks).
inline bool scale_round_in_registers(size_t ks, size_t kd) { return ks <= 8 && kd <= 9; }
template <typename T>
hipError_t launch_scale_round(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t ks, int centred,
                              int keep, int chunked, hipStream_t st);
// NTT-form base conversion and mod-down (kernels_baseconv_ntt.hip; include/nflhip.h "RNS base conversion, NTT form").  _fused: ONE
// launch, a workgroup per polynomial with ks + 1 rows in LDS, one more in centred mode; hipErrorNotSupported when that exceeds 64 KiB
// or n < 4.  Operands as launch_baseconv.  _combine: the last pass of the composed mod-down, out row j = (in row j - out row j) P^-1
// mod p_j over the dense out = [batch][nm - k][n]; rec the mod-down's record.
static constexpr size_t kBaseconvNttLdsBytes = 65536;
inline size_t baseconv_ntt_fused_lds(size_t ks, size_t n, size_t word, int centred) { return (ks + 1 + (centred ? 1 : 0)) * n * word; }
template <typename T>
hipError_t launch_baseconv_ntt_fused(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *rec, size_t batch, size_t s0,
                                     size_t ks, size_t d0, size_t kd, int centred, int moddown, hipStream_t st);
template <typename T>
hipError_t launch_moddown_ntt_combine(const Shape &s, T *out, const T *in, const uint64_t *rec, size_t batch, size_t k, hipStream_t st);
// hybrid key switching, NTT form (kernels_keyswitch.hip; include/nflhip.h "hybrid key switching"): the mod-up of EVERY digit in one
// streaming pass.  in = [batch][L][n] coefficient form (the inverse-transformed input), digits of alpha rows (the last may be short),
// dnum = ceil(L / alpha); out = [batch][dnum][nm][n]: polynomial (b, d) holds the conversion of digit d to every row of the context,
// rows of the digit itself as the input has them.  recs: device array of the dnum device records of (d alpha, |S_d|) -> (0, nm).
// out never is in (api.hip: both are context-owned scratch).
template <typename T>
hipError_t launch_modup_digits(const Shape &s, const DevTables &t, T *out, const T *in, const uint64_t *const *recs, size_t batch, size_t L,
                               size_t alpha, int centred, hipStream_t st);
// the one-launch plan up to the two sums: in = [batch][L][n] NTT form, key = [dnum][2][nm][n], acc = [2][batch][nm][n] canonical
// (acc[c][b] = sum_d U_d key[d][c]).  A workgroup per polynomial; LDS: the L source rows, one work row and, in centred mode, the
// corrections v of every digit as 16-bit words (v <= alpha <= 1024) -- keyswitch_fused_lds.  hipErrorNotSupported beyond 64 KiB, for
// rows above 2048 words or below 4 (keyswitch_fused_fits).
inline size_t keyswitch_fused_lds(size_t L, size_t dnum, size_t n, size_t word, int centred) { return (L + 1) * n * word + (centred ? dnum * n * 2 : 0); }
inline bool keyswitch_fused_fits(size_t L, size_t dnum, size_t n, size_t word, int centred) {
  return n >= 4 && n <= 2048 && keyswitch_fused_lds(L, dnum, n, word, centred) <= kBaseconvNttLdsBytes;
}
template <typename T>
hipError_t launch_modup_dot_fused(const Shape &s, const DevTables &t, T *acc, const T *in, const T *key, const uint64_t *const *recs, size_t batch,
                                  size_t L, size_t alpha, int centred, hipStream_t st);
// the tensor product of two degree-1 ciphertexts (kernels_mulrelin.hip; include/nflhip.h "ciphertext multiplication"): out0 = a0 b0,
// out1 = a0 b1 + a1 b0, out2 = a1 b1 on the first `rows` moduli, inputs dense [batch][rows][n]; b0 == b1 == nullptr: the square.
// An output may be exactly an input.  pi == nullptr (the public entry): orows == rows, pitch01 == pitch2 == rows n.  pi = a device
// array of nm pairs (pi_m, Shoup companion): out0 / out1 are written as pi_m d_c over orows rows with the polynomial pitch pitch01,
// rows [rows, orows) as zeros, out2 with the pitch pitch2 (words).
template <typename T>
hipError_t launch_tensor_ntt(const Shape &s, const DevTables &t, T *out0, T *out1, T *out2, const T *a0, const T *a1, const T *b0, const T *b1,
                             size_t batch, size_t rows, size_t orows, size_t pitch01, size_t pitch2, const uint64_t *pi, hipStream_t st);
// the tensor product summed over terms (kernels_tensor_dot.hip; include/nflhip.h "sums of ciphertext products"): D0 = sum_j a0 b0,
// D1 = sum_j (a0 b1 + a1 b0), D2 = sum_j a1 b1 per group on the first `rows` moduli.  An operand's polynomial (g, j) lies
// g group_stride + j term_stride polynomials OF `rows` ROWS after its ptr (nflhip_dot_operand, field for field); b0 == b1 == nullptr:
// the squares.  The outputs must not overlap the operands (api.hip checks).  pi, orows and the pitches: as launch_tensor_ntt.
struct TensorDotOperand {
  const void *ptr;
  size_t group_stride, term_stride;
};
template <typename T>
hipError_t launch_tensor_dot_ntt(const Shape &s, const DevTables &t, T *out0, T *out1, T *out2, const TensorDotOperand *a0, const TensorDotOperand *a1,
                                 const TensorDotOperand *b0, const TensorDotOperand *b1, size_t groups, size_t terms, size_t rows, size_t orows,
                                 size_t pitch01, size_t pitch2, const uint64_t *pi, hipStream_t st);
// the multiplication's one-launch plan up to the two sums: a*, b* = [batch][L][n] NTT form (b0 == b1 == nullptr: the square), key =
// [dnum][2][nm][n], acc = [2][batch][nm][n] canonical, acc[c][b] = E(pi d_c) + sum_d U_d key[d][c] with U_d the mod-up of a1 (.) b1.
// The LDS and the bounds of launch_modup_dot_fused (keyswitch_fused_lds / keyswitch_fused_fits): hipErrorNotSupported beyond them.
template <typename T>
hipError_t launch_tensor_modup_dot_fused(const Shape &s, const DevTables &t, T *acc, const T *a0, const T *a1, const T *b0, const T *b1, const T *key,
                                         const uint64_t *const *recs, const uint64_t *pi, size_t batch, size_t L, size_t alpha, int centred,
                                         hipStream_t st);
// the key reads of a call below the top level (kernels_level.hip; include/nflhip.h "leveled key switching"): s, t are those of the
// level context C_l (split + K rows), the key stays in its PARENT's layout [dnum][2][knm][n] -- child row r of a key polynomial is the
// parent's row r for r < split and r + hole from there on, knm = s.nm + hole.  _dot_key_level: launch_dot with b = key + c knm n as the
// shared second operand, a term every two parent polynomials (key[d][c]).  The other two: the one-launch kernels above, L = split.
struct KeyLevel { size_t knm, split, hole; };
template <typename T>
hipError_t launch_dot_key_level(const Shape &s, const DevTables &t, T *out, const T *a, size_t a_gs, size_t a_ts, const T *key, const T *addend,
                                size_t groups, size_t terms, int tiled, const KeyLevel &kl, hipStream_t st);
template <typename T>
hipError_t launch_modup_dot_fused_level(const Shape &s, const DevTables &t, T *acc, const T *in, const T *key, const uint64_t *const *recs,
                                        size_t batch, size_t L, size_t alpha, int centred, const KeyLevel &kl, hipStream_t st);
template <typename T>
hipError_t launch_tensor_modup_dot_fused_level(const Shape &s, const DevTables &t, T *acc, const T *a0, const T *a1, const T *b0, const T *b1,
                                               const T *key, const uint64_t *const *recs, const uint64_t *pi, size_t batch, size_t L, size_t alpha,
                                               int centred, const KeyLevel &kl, hipStream_t st);
// the same layout for a hoisted rotation or a linear transform at a level (kernels_level_rotate.hip; include/nflhip.h "rotations and
// linear transforms at a level").  launch_dot_multi with bs[o] = component c of a key in the parent's layout, key + c knm n words,
// a term every 2 knm n words; launch_permute_mac_ntt (one staging buffer) on all rows of the level context with weights[t] = a
// diagonal [knm][n] in the parent's layout.  Everything else is the level context's dense layout.
template <typename T>
hipError_t launch_dot_multi_level(const Shape &s, const DevTables &t, T *const *outs, const T *a, size_t a_gs, size_t a_ts, const T *const *bs,
                                  size_t outputs, size_t groups, size_t terms, int tiled, const KeyLevel &kl, hipStream_t st);
template <typename T>
hipError_t launch_permute_mac_ntt_level(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const T *const *weights,
                                        const uint64_t *ks, int terms, size_t batch, size_t comps, size_t in_cs, size_t out_cs, const KeyLevel &kl,
                                        hipStream_t st);
// the kernels of the BSGS slot linear transform (kernels_bsgs.hip; include/nflhip.h "weighted sums of automorphisms into several
// outputs", "BSGS slot linear transforms").  launch_permute_mac_multi_ntt: launch_permute_mac_ntt for `outputs` outputs that share ins
// and ks -- outs[o] = addends[o] + sum_t weights[o terms + t] (.) sigma^NTT_{ks[t]}(ins[t]), a NULL weight skipped, addends NULL or
// addends[o] NULL or outs[o] --, one launch per kMacMultiJB outputs; _level: on all rows of a level context with the weights in the
// parent's layout.  launch_permute_sum_ntt: out = addend + sum_t sigma^NTT_{ks[t]}(ins[t]), no weights.  HOST arrays of device pointers.
template <typename T>
hipError_t launch_permute_mac_multi_ntt(const Shape &s, const DevTables &t, T *const *outs, const T *const *addends, const T *const *ins,
                                        const T *const *weights, const uint64_t *ks, int outputs, int terms, size_t batch, size_t R, size_t comps,
                                        size_t in_cs, size_t out_cs, hipStream_t st);
template <typename T>
hipError_t launch_permute_mac_multi_ntt_level(const Shape &s, const DevTables &t, T *const *outs, const T *const *addends, const T *const *ins,
                                              const T *const *weights, const uint64_t *ks, int outputs, int terms, size_t batch, size_t comps,
                                              size_t in_cs, size_t out_cs, const KeyLevel &kl, hipStream_t st);
template <typename T>
hipError_t launch_permute_sum_ntt(const Shape &s, const DevTables &t, T *out, const T *addend, const T *const *ins, const uint64_t *ks, int terms,
                                  size_t batch, size_t R, size_t comps, size_t in_cs, size_t out_cs, hipStream_t st);
// in-place bit reversal of every row (permut.hpp:86-117), and `count` copies of one polynomial
template <typename T> hipError_t launch_bitrev_rows(const Shape &s, T *d, size_t rows, hipStream_t st);
hipError_t launch_broadcast(void *dst, const void *one, size_t bytes_per_poly, size_t count, hipStream_t st);
template <typename T>
hipError_t launch_crt_lift(const Shape &s, const DevTables &t, uint64_t *limbs, const T *d, size_t batch, hipStream_t st);
template <typename T>
hipError_t launch_crt_project(const Shape &s, const DevTables &t, T *d, const uint64_t *limbs, size_t L_in, size_t batch,
                              hipStream_t st);
// any number of moduli: `scratch` = batch * n * t.crt_Lw words (the unreduced sums, limb-major)
template <typename T>
hipError_t launch_crt_lift_wide(const Shape &s, const DevTables &t, uint64_t *limbs, const T *d, size_t batch,
                                uint64_t *scratch, hipStream_t st);

// ---- samplers (kernels_sample.hip): ChaCha20 counter streams keyed by (key32, stream_id) ----
void set_gauss_tie_shift(int shift);  // debug entry point nflhip_debug_gauss_tie_shift (include/nflhip_debug.h)
hipError_t launch_random_words(uint64_t *out, uint64_t first_word, size_t nwords, const unsigned char *key32,
                               uint64_t stream_id, hipStream_t st);
// dist: 0 uniform | 1 bounded (p0 = upper bound, p1 = amplifier) | 2 zero/one (p0 = rho) | 3 hamming weight (p0 = h);
// | 0x100 reference words (zero/one, hamming weight) | 0x200 narrow draw (uniform: keystream lanes of the limb width)
template <typename T>
hipError_t launch_sample(const Shape &s, const DevTables &t, T *d, size_t first_poly, size_t batch, int dist, uint64_t p0,
                         uint64_t p1, const unsigned char *key32, uint64_t stream_id, hipStream_t st, int seq_on = 0,
                         uint64_t seq_stride = 0);  // seq_on: polynomial b = a one-polynomial call with stream id + b * seq_stride
hipError_t launch_inner_fwd_fast_u32(const Shape &s, const DevTables &t, const uint32_t *src, uint32_t *dst, size_t rows,
                                     hipStream_t st);
hipError_t launch_inner_inv_fast_u32(const Shape &s, const DevTables &t, const uint32_t *src, const uint32_t *mul,
                                     uint32_t *dst, size_t rows, hipStream_t st);
// narrow (every Gaussian launcher): the table's draw width is 32 bits (nflhip_gauss_set_draw_bits) -- domains 7 / 8 of the keystream
hipError_t launch_gauss_noise(long long *out, uint64_t first_sample, size_t count, const uint64_t *cdt, int words,
                              int entries, long long x_min, const unsigned char *key32, uint64_t stream_id, hipStream_t st,
                              int narrow = 0);
template <typename T>
hipError_t launch_sample_gauss(const Shape &s, const DevTables &t, T *d, size_t first_poly, size_t batch,
                               const uint64_t *cdt, int words, int entries, long long x_min, uint64_t amp,
                               const unsigned char *key32, uint64_t stream_id, hipStream_t st, int seq_on = 0,
                               uint64_t seq_stride = 0, int narrow = 0, const uint16_t *lut = nullptr);
// the narrow draw's bucket table (device copy passed as `lut` above and below; empty = the table does not fit LDS)
std::vector<uint16_t> gauss_bucket_table(const uint64_t *cdt, int words, size_t entries);

// compact Gaussian polynomials (one signed integer x * amp per coefficient; format 1 int8 | 2 int16 | 3 int32) and their
// expansion into residue words (format 0 = word rows: a strided gather); stride in polynomials, 0 = shared
hipError_t launch_gauss_small(const Shape &s, void *d, int format, size_t first_poly, size_t batch, const uint64_t *cdt,
                              int words, int entries, long long x_min, uint64_t amp, const unsigned char *key32,
                              uint64_t stream_id, hipStream_t st, int seq_on = 0, uint64_t seq_stride = 0, int narrow = 0,
                              const uint16_t *lut = nullptr);
hipError_t launch_gauss_small_multi(const Shape &s, void *const *d, size_t count, int format, size_t batch, const uint64_t *cdt, int words,
                                    int entries, long long x_min, const uint64_t *amp, const unsigned char *key32, const uint64_t *stream_id,
                                    const uint64_t *seq_stride, hipStream_t st, int narrow, const uint16_t *lut);
template <typename T>
hipError_t launch_expand_small(const Shape &s, const DevTables &t, T *dst, const void *src, int format, unsigned stride,
                               size_t batch, hipStream_t st);

// transform-fused pipelines at n = 4096, 64-bit limbs (tools/gen_polymul_asm.py build_fused): kind 0 enc2 | 1 fma_fwd |
// 2 fms_inv | 3 fma_inv; x: up to three operands with their formats (forward kinds) and strides, k: key rows with strides.
// hipErrorNotSupported for other shapes / the compiled-only variant (api.hip composes the same result from the plain kernels)
// INTT(b -+ a (.) key) in one pass on the wave-per-row kernels (kernels_wave.hip): rows of 1024 / 2048 words, 4096 for 32-bit limbs
// out0 = NTT(x) k0 + NTT(e0) [, out1 = NTT(x) k1 + NTT(e1)] on the wave-per-row kernels (kernels_wave.hip k_row_fwd_fma): rows of 1024 /
// 2048 words (4096 for 32-bit limbs), x / e0 / e1 of one format, strides 0 or 1; hipErrorNotSupported otherwise
hipError_t launch_row_fwd_fma_u32(const Shape &s, const DevTables &t, int format, uint32_t *out0, uint32_t *out1, const void *x, unsigned xs,
                                  const uint32_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint32_t *k1, unsigned k1s, const void *e1,
                                  unsigned e1s, size_t batch, hipStream_t st);
hipError_t launch_row_fwd_fma_u64(const Shape &s, const DevTables &t, int format, uint64_t *out0, uint64_t *out1, const void *x, unsigned xs,
                                  const uint64_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint64_t *k1, unsigned k1s, const void *e1,
                                  unsigned e1s, size_t batch, hipStream_t st);
hipError_t launch_row_fma_inv_u32(const Shape &s, const DevTables &t, int subtract, uint32_t *c, const uint32_t *a, const uint32_t *key,
                                  int kstride, const uint32_t *b, size_t batch, hipStream_t st);
hipError_t launch_row_fma_inv_u64(const Shape &s, const DevTables &t, int subtract, uint64_t *c, const uint64_t *a, const uint64_t *key,
                                  int kstride, const uint64_t *b, size_t batch, hipStream_t st);
// rows of 32768 words from a compact (int8) Gaussian polynomial: its forward transform, and NTT(x) k0 + e0' [, NTT(x) k1 + e1'] (e' words)
hipError_t launch_row32k_fwd_i8_u64(const Shape &s, const DevTables &t, uint64_t *dst, const void *x8, size_t batch, hipStream_t st);
hipError_t launch_row32k_fwd_fma_i8_u64(const Shape &s, const DevTables &t, uint64_t *out0, uint64_t *out1, const void *x8,
                                        const uint64_t *k0, const uint64_t *e0p, const uint64_t *k1, const uint64_t *e1p, size_t batch,
                                        hipStream_t st);
hipError_t launch_fused_asm_u64(const Shape &s, const DevTables &t, int kind, uint64_t *out0, uint64_t *out1,
                                const void *const *x, const unsigned *xstride, const int *xfmt, const void *const *k,
                                const unsigned *kstride, size_t batch, hipStream_t st);

// ---- fast paths (kernels_fast.hip); return hipErrorNotSupported when the shape has none ----
hipError_t launch_polymul_fast_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                                   int b_is_ntt, size_t batch, hipStream_t st);
hipError_t launch_ntt_fwd_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t batch,
                                   hipStream_t st);
hipError_t launch_ntt_inv_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t batch,
                                   hipStream_t st);

// 4096-word inner blocks of rows with logn >= 12 on the register-tiled kernels (rows = batch * nm);
// `mul` != nullptr fuses the point-wise product into the inverse's load.
hipError_t launch_inner_fwd_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t rows,
                                     hipStream_t st);
hipError_t launch_inner_inv_fast_u64(const Shape &s, const DevTables &t, const uint64_t *src, const uint64_t *mul,
                                     uint64_t *dst, size_t rows, hipStream_t st);

// streaming outer passes alone (rows with logn > 12): forward src -> dst, inverse in place
// (`logi` = log2 of the block the following fused kernel owns: global stages [0, logn - logi) run here)
hipError_t launch_outer_fwd_u64(const Shape &s, const DevTables &t, const uint64_t *src, uint64_t *dst, size_t rows,
                                hipStream_t st, int logi = 12);
hipError_t launch_outer_inv_u64(const Shape &s, const DevTables &t, uint64_t *data, size_t rows, hipStream_t st,
                                int logi = 12);
// fused NTT,NTT,(.),INTT over the 4096-word blocks of rows whose outer forward passes already ran
// (a_in, b_in) and whose outer inverse passes still have to run on c (logn > 12), or the whole
// polymul for logn == 12.  hipErrorNotSupported when the assembly code object is unavailable.
// b_is_ntt: b_in is the fully transformed operand (canonical words), only a_in went through the outer passes.
hipError_t launch_polymul_blocks_asm_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a_in,
                                         const uint64_t *b_in, size_t batch, hipStream_t st, bool b_is_ntt = false);

// 32768-word rows, ONE operand register-resident per 1024-thread workgroup: mode 1: c = INTT(NTT(a) (.) b) with b already
// transformed (streamed through the point-wise step), 2: c = NTT(a), 3: c = INTT(a); 4 / 5: modes 2 / 1 with the transformed
// operand in the layout [block][pair][thread] that only these two kernels share (the composed product's scratch: coalesced on
// both sides, no transposes); hipErrorNotSupported for other shapes
hipError_t launch_row32k_u64(const Shape &s, const DevTables &t, int mode, uint64_t *c, const uint64_t *a, const uint64_t *b,
                             size_t batch, hipStream_t st);
// n = 65536: one launch of the three-role pipeline kernel (block products of chunk j-1, forward streaming pass of
// chunk j, inverse streaming pass of chunk j-2); hipErrorNotSupported for other shapes
// one launch for the whole batch, rows pinned to an XCD (n = 65536 / 32768); xcd_plan_bytes() = 0 when the shape / batch
// 16-bit limbs, n = 128, fused product: the generated gfx950 assembly kernel (hipErrorNotSupported: composed plan)
hipError_t launch_row128_u16_asm(const Shape &s, const DevTables &t, int mode, uint16_t *c, const uint16_t *a,
                                 const uint16_t *b, size_t batch, hipStream_t st);
// 32-bit limbs, n = 1024, fused product: the generated gfx950 assembly kernel (hipErrorNotSupported: use k_row)
hipError_t launch_row1024_u32_asm(const Shape &s, const DevTables &t, int mode, uint32_t *c, const uint32_t *a,
                                  const uint32_t *b, size_t batch, hipStream_t st);
// ... their transform-fused pipelines (formats words / int8, strides 0 / 1; hipErrorNotSupported: the compiled kernels)
hipError_t launch_row_fwd_fma_u32_asm(const Shape &s, const DevTables &t, int format, uint32_t *out0, uint32_t *out1, const void *x, unsigned xs,
                                      const uint32_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint32_t *k1, unsigned k1s,
                                      const void *e1, unsigned e1s, size_t batch, hipStream_t st);
hipError_t launch_row_fma_inv_u32_asm(const Shape &s, const DevTables &t, int subtract, uint32_t *c, const uint32_t *a, const uint32_t *key,
                                      int kstride, const uint32_t *b, size_t batch, hipStream_t st);
hipError_t launch_row_fwd_fma_u64_asm(const Shape &s, const DevTables &t, int format, uint64_t *out0, uint64_t *out1, const void *x, unsigned xs,
                                      const uint64_t *k0, unsigned k0s, const void *e0, unsigned e0s, const uint64_t *k1, unsigned k1s,
                                      const void *e1, unsigned e1s, size_t batch, hipStream_t st);
hipError_t launch_row_fma_inv_u64_asm(const Shape &s, const DevTables &t, int subtract, uint64_t *c, const uint64_t *a, const uint64_t *key,
                                      int kstride, const uint64_t *b, size_t batch, hipStream_t st);
// 64-bit limbs, n = 1024 / 2048: the generated twins (modes 0, 2, 3; hipErrorNotSupported: use k_row)
hipError_t launch_row1024_u64_asm(const Shape &s, const DevTables &t, int mode, uint64_t *c, const uint64_t *a,
                                  const uint64_t *b, size_t batch, hipStream_t st);
// is not covered.  `work`: device memory of that many bytes, initialised by the call on `st`.
size_t xcd_plan_bytes(const Shape &s, size_t batch);
hipError_t launch_polymul_xcd_u64(const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                                  size_t batch, void *work, hipStream_t st, int level = 0);
// one empty launch per translation unit (+ the generated kernels' module): api.hip warm_up_device
hipError_t warm_generic(hipStream_t st);
hipError_t warm_fast(hipStream_t st);
hipError_t warm_crt(hipStream_t st);
hipError_t warm_crt_mfma(hipStream_t st);
hipError_t warm_sample(hipStream_t st);
hipError_t warm_wave(hipStream_t st);
hipError_t warm_automorph(hipStream_t st);
hipError_t warm_rescale(hipStream_t st);
hipError_t warm_dot(hipStream_t st);
hipError_t warm_dot_multi(hipStream_t st);
hipError_t warm_rotate(hipStream_t st);
hipError_t warm_lintrans(hipStream_t st);
hipError_t warm_mulrelin(hipStream_t st);
hipError_t warm_tensor_dot(hipStream_t st);
hipError_t warm_decompose(hipStream_t st);
hipError_t warm_baseconv(hipStream_t st);
hipError_t warm_baseconv_ntt(hipStream_t st);
hipError_t warm_scale_round(hipStream_t st);
hipError_t warm_keyswitch(hipStream_t st);
int polymul_level();   // 0 / 1 / 2: transforms of the coefficient-form products complete / incomplete (asm_launch.hip, nflhip_debug_polymul_level)
hipError_t launch_polymul_pipe64k_u64(const Shape &s, const DevTables &t, uint64_t *c_v, const uint64_t *a_v,
                                      const uint64_t *b_v, int cnt_v, const uint64_t *fa_src, uint64_t *fa_dst,
                                      const uint64_t *fb_src, uint64_t *fb_dst, int cnt_f, uint64_t *inv, int cnt_i,
                                      hipStream_t st, bool b_is_ntt = false, int level = 0);

// n = 1024, 32- and 64-bit limbs: one wave per row (kernels_wave.hip).  mode 0: c = INTT(NTT(a)(.)NTT(b)); 1: b already in
// NTT form; 2: c = NTT(a); 3: c = INTT(a).  hipErrorNotSupported for other shapes.
hipError_t launch_row1024_u32(const Shape &s, const DevTables &t, int mode, uint32_t *c, const uint32_t *a,
                              const uint32_t *b, size_t batch, hipStream_t st);
hipError_t launch_row1024_u64(const Shape &s, const DevTables &t, int mode, uint64_t *c, const uint64_t *a,
                              const uint64_t *b, size_t batch, hipStream_t st);

// register-resident CRT kernels for 64-bit limbs (kernels_crt.hip); hipErrorNotSupported otherwise
hipError_t launch_crt_lift_fast_u64(const Shape &s, const DevTables &t, uint64_t *limbs, const uint64_t *d, size_t batch,
                                    hipStream_t st);
// the lift as an int8 GEMM on v_mfma_i32_32x32x32_i8 (kernels_crt_mfma.hip): many moduli, batch * n a multiple of 64
hipError_t launch_crt_lift_mfma_u64(const Shape &s, const DevTables &t, uint64_t *limbs, const uint64_t *d, size_t batch,
                                    hipStream_t st);
hipError_t launch_crt_project_mfma_u64(const Shape &s, const DevTables &t, uint64_t *d, const uint64_t *limbs, size_t L_in,
                                       size_t batch, hipStream_t st);
hipError_t launch_crt_project_fast_u64(const Shape &s, const DevTables &t, uint64_t *d, const uint64_t *limbs, size_t L_in,
                                       size_t batch, hipStream_t st);

}  // namespace nflhip
