/* nflhip.h -- C ABI of the MI355X-native NTT polynomial-ring engine.
 *
 * This is the drop-in boundary for the ONE hot path of quarkslab/NFLlib that
 * this project accelerates: whole-polynomial / whole-batch
 * operations on the dense modulus-major coefficient block of
 * nfl::poly<T, Degree, NbModuli> (reference include/nfl/poly.hpp:82-88:
 * `T _data[NbModuli*Degree]`, element (cm,i) at `_data[cm*Degree+i]`).  A batch
 * is an array of polys, i.e. a dense [batch][NbModuli][Degree] tensor (how the
 * reference's tests allocate: tests/tools.h:6-17).
 *
 * Every entry point names the reference interface it replaces (file:line under
 * /root/reference).  All results are bit-identical to the reference's on the
 * same inputs.  Plain C types only; no exceptions cross this boundary: every
 * call returns an int status (0 = NFLHIP_OK) and nflhip_last_error() gives the
 * text.  The library is implemented in hand-written HIP for gfx950 and there
 * is NO CPU fallback: without a usable GPU every compute call fails with
 * NFLHIP_ERR_NO_DEVICE.
 *
 * Environment (all of it; every variable is read ONCE, when a context / communicator is created)
 *   NFLHIP_VARIANT=hipcc   the context serves every call with the compiled (hipcc) kernels instead of the generated
 *                          gfx950 assembly kernels: the independent cross-check the tests use (bit-identical results)
 *   NFLHIP_XCD=0|1         rows of 32768 / 65536 words: never / always the one-launch plan of persistent workgroups
 *                          (default: by batch size)
 *   NFLHIP_COMM_PIECE_BYTES  upper bound of one RCCL message of nflhip_scatter_dev / nflhip_gather_dev (default 1 GiB)
 * Test hooks are entry points of their own (include/nflhip_debug.h), not environment variables.
 *
 * Pointer conventions
 *   *_dev entry points take DEVICE pointers and a hipStream_t (passed as
 *   void*; NULL = the null stream) and are asynchronous on that stream.
 *   The un-suffixed entry points take HOST pointers, stage through
 *   context-owned device buffers and return after the result is in host
 *   memory (the per-poly calls of the header-only nfl::poly surface use them).
 *   `out` may alias any input of an element-wise op (the reference's
 *   evaluation loop is strictly element-wise: core.hpp:24-37).
 */
#ifndef NFLHIP_H
#define NFLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFLHIP_ABI_VERSION 6

typedef struct nflhip_ctx nflhip_ctx;

/* status codes */
enum {
  NFLHIP_OK = 0,
  NFLHIP_ERR_INVALID = 1,    /* bad argument (std::runtime_error / static_assert in the reference) */
  NFLHIP_ERR_NO_DEVICE = 2,  /* no usable HIP device: there is no CPU fallback */
  NFLHIP_ERR_HIP = 3,        /* a HIP runtime call failed */
  NFLHIP_ERR_UNSUPPORTED = 4,/* shape outside what the engine implements */
  NFLHIP_ERR_NOMEM = 5
};

/* element-wise operations (the functors poly::operator=(expr) evaluates) */
enum {
  NFLHIP_OP_ADD = 0,           /* ops::addmod        ops.hpp:124-135; operator+  poly.hpp:347 */
  NFLHIP_OP_SUB = 1,           /* ops::submod        ops.hpp:141-151; operator-  poly.hpp:346 */
  NFLHIP_OP_MUL = 2,           /* ops::mulmod        ops.hpp:183-219; operator*  poly.hpp:350 */
  NFLHIP_OP_MUL_SHOUP = 3,     /* ops::mulmod_shoup  ops.hpp:225-242; shoup(a*b,b') ops.hpp:267-277 */
  NFLHIP_OP_COMPUTE_SHOUP = 4  /* ops::compute_shoup ops.hpp:165-177; poly.hpp:352 */
};

/* tables readable through nflhip_get_table (reference-format views, for parity tests) */
enum {
  NFLHIP_TAB_PSI = 0,       /* engine layout: n pairs (psi^bitrev(k), Shoup companion), k=0..n-1 */
  NFLHIP_TAB_MODULUS = 1,   /* 1 word: params<T>::P[cm]                       params.hpp:21,55,97 */
  NFLHIP_TAB_INVDEGREE = 2, /* 1 word: core::invpolyDegree[cm]                core.hpp:664-665 */
  /* the reference's OWN table layouts (poly.hpp:228-237), rebuilt on the host from the same roots: what a caller that
   * reads core::base through the tests::poly_tests_proxy friend sees (tests/ntt_perfs.cpp:132-133).  No device needed. */
  NFLHIP_TAB_PHIS = 3,                 /* degree words: phi^i                          core.hpp:649-656 */
  NFLHIP_TAB_SHOUPPHIS = 4,            /* degree words: their Shoup companions */
  NFLHIP_TAB_INVPOLY_INVPHIS = 5,      /* degree words: n^-1 * phi^-i                  core.hpp:664-676 */
  NFLHIP_TAB_SHOUPINVPOLY_INVPHIS = 6, /* degree words */
  NFLHIP_TAB_OMEGAS = 7,               /* 2*degree words: stage-concatenated powers of omega = phi^2 (core::prep_wtab,
                                          core.hpp:564-581), then their Shoup companions at offset degree (shoupomegas) */
  NFLHIP_TAB_INVOMEGAS = 8             /* 2*degree words: the same for omega^-1 (invomegas / shoupinvomegas) */
};

int nflhip_abi_version(void);
/* Text of the last error any nflhip call raised ON THE CALLING THREAD (errno
 * style, so host threads sharing one context never race on it; ctx may be NULL,
 * e.g. after a failed nflhip_ctx_create). Never NULL. */
const char *nflhip_last_error(const nflhip_ctx *ctx);
int nflhip_device_count(int *count);

/* ---- context: replaces the static tables of poly::core / poly::GMP ----------
 * core::initialize (core.hpp:625-686), core::prep_wtab (core.hpp:564-581) and
 * GMP::GMP (gmp.hpp:113-155).  Built lazily by the caller (never at static-init
 * time, unlike poly.hpp:247).  limb_bits in {16,32,64}; P / primitive_roots /
 * invkmax point at nmoduli words of that width taken from params<T>
 * (params.hpp:21-36, 55-76, 97-113); kmax_log2 = log2(params<T>::kMaxPolyDegree).
 * The context is immutable after creation: entry points may be called from
 * several host threads with distinct streams.  One context per device.
 * The *_dev entry points only enqueue work on the caller's stream (no host
 * synchronisation, no allocation after the first call of a given size), so a
 * sequence of them can be captured into a hipGraph and replayed; the exceptions
 * are nflhip_any_eq_dev / nflhip_any_neq_dev, which return a host value. */
int nflhip_ctx_create(nflhip_ctx **out, int device, int limb_bits, size_t degree, size_t nmoduli,
                      const void *P, const void *primitive_roots, const void *invkmax, int kmax_log2);
int nflhip_ctx_destroy(nflhip_ctx *ctx);

size_t nflhip_degree(const nflhip_ctx *ctx);
size_t nflhip_nmoduli(const nflhip_ctx *ctx);
int nflhip_limb_bits(const nflhip_ctx *ctx);
/* L = ceil(bits(prod p_cm)/64): 64-bit limbs per lifted coefficient (gmp.hpp:121-122) */
size_t nflhip_crt_limbs(const nflhip_ctx *ctx);
int nflhip_get_table(const nflhip_ctx *ctx, int which, size_t cm, void *host_out, size_t host_bytes);
/* CRT constants as little-endian 64-bit limbs; what: 0 = moduli_product, 1 = lifting_integers[cm]
 * (gmp.hpp:115-151). Returns the number of significant limbs through *nlimbs. */
int nflhip_get_crt_constant(const nflhip_ctx *ctx, int what, size_t cm, uint64_t *host_out, size_t cap,
                            size_t *nlimbs);

/* ---- transforms ------------------------------------------------------------
 * poly::ntt_pow_phi()       poly.hpp:167 -> core::ntt_pow_phi        core.hpp:594-600
 * poly::invntt_pow_invphi() poly.hpp:168 -> core::invntt_pow_invphi  core.hpp:608-614
 * In place on [batch][nmoduli][degree]; forward output is in the reference's
 * order (out[cm][bitrev(k)] = a_cm(phi^(2k+1))) and every output word is the
 * canonical representative in [0,p) (core.hpp:523-529, ops.hpp:240). */
int nflhip_ntt_fwd_dev(nflhip_ctx *ctx, void *d_data, size_t batch, void *stream);
int nflhip_ntt_inv_dev(nflhip_ctx *ctx, void *d_data, size_t batch, void *stream);
int nflhip_ntt_fwd(nflhip_ctx *ctx, void *h_data, size_t batch);
int nflhip_ntt_inv(nflhip_ctx *ctx, void *h_data, size_t batch);

/* ---- the cyclic transform of single rows ------------------------------------------
 * core::ntt(x, wtab, winvtab, p)   core.hpp:455-532 (Harvey DIF, algos.hpp:47-73): in-place CYCLIC transform of
 * `rows` contiguous rows of `degree` words, all of modulus `cm`: natural order in, bit-reversed order out,
 * out[bitrev(k)] = sum_j x[j] w^(jk), every word in [0,p).  mode bit NFLHIP_ROW_INVERSE_TABLES selects
 * w = omega^-1 (the reference's invomegas tables) instead of omega = phi^2; bit NFLHIP_ROW_BITREV_IO bit-reverses
 * the row before and after, i.e. core::inv_ntt (core.hpp:539-557) when combined with the inverse tables.
 * This is what tests/ntt_perfs.cpp:155-171 times through the poly_tests_proxy friend (BASELINE configs[0]). */
#define NFLHIP_ROW_INVERSE_TABLES 1
#define NFLHIP_ROW_BITREV_IO 2
int nflhip_ntt_row_dev(nflhip_ctx *ctx, void *d_rows, size_t cm, int mode, size_t rows, void *stream);
int nflhip_ntt_row(nflhip_ctx *ctx, void *h_rows, size_t cm, int mode, size_t rows);

/* ---- Galois automorphisms ------------------------------------------------------------
 * sigma_k : a(X) -> a(X^k) mod (X^n + 1) for odd k, taken mod 2n, on every row of [batch][nmoduli][degree] (the primitive
 * behind slot rotations, conjugation (k = 2n - 1), traces and key switching to a Galois key).  n = degree, p = the row's modulus.
 *   NFLHIP_FORM_COEFF  coefficient form, canonical words in [0,p) in and out: for i in [0,n), e = i k mod 2n,
 *                      out[e] = in[i] when e < n, else out[e - n] = (p - in[i]) mod p (0 stays 0).
 *   NFLHIP_FORM_NTT    the order nflhip_ntt_fwd_dev produces (slot j holds a(phi^(2 rev(j) + 1)), rev = the log2(n)-bit
 *                      reversal): out[j] = in[j'] where 2 rev(j') + 1 = k (2 rev(j) + 1) mod 2n.  The stored words move
 *                      unchanged, so ntt_inv(sigma_ntt(ntt_fwd(x))) == sigma_coeff(x) word for word.
 * The multi form writes d_outs[m] = sigma_{ks[m]}(d_in) for m < count <= NFLHIP_AUTOMORPHISM_MAX_OUTPUTS and reads d_in
 * once (hoisted rotations).  NFLHIP_ERR_INVALID: an even k, an unknown form, a count of 0 or above the maximum, a NULL
 * pointer, or an output that overlaps the input or another output (the device entries never work in place).  The host
 * variant stages both sides and accepts h_out == h_in (but no other overlap).  The _dev entries allocate nothing and do
 * not synchronise: they can be captured into a hipGraph (the multi form's pointers and multipliers travel as kernel
 * arguments). */
#define NFLHIP_FORM_COEFF 0
#define NFLHIP_FORM_NTT 1
#define NFLHIP_AUTOMORPHISM_MAX_OUTPUTS 16
int nflhip_automorphism_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, uint64_t k, int form, void *stream);
int nflhip_automorphism(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, uint64_t k, int form);
int nflhip_automorphism_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const uint64_t *ks, size_t count, const void *d_in,
                                  size_t batch, int form, void *stream);

/* ---- RNS rescale: exact division with rounding by the last modulus -----------------------
 * The primitive behind CKKS rescaling, BGV / BFV modulus switching and the mod-down step of key switching.  Context: nmoduli >= 2
 * moduli p_0 .. p_L (L = nmoduli - 1), q = p_L, Q = their product, Q' = Q / q, h = (q - 1) / 2.  For every coefficient position
 * X in [0, Q) is the integer whose residues are the input words; the output holds the residues mod p_0 .. p_(L-1) of
 *     Y = floor((X + h) / q) mod Q'
 * -- X / q rounded to nearest (and the centred representative of X rounded correctly) -- as canonical words in [0, p_i).  In RNS
 * arithmetic r = (x_L + h) mod q and y_i = (x_i + h - r) q^-1 mod p_i; no multi-precision integer is formed.
 *   input   [batch][nmoduli][degree]
 *   output  [batch][nmoduli - 1][degree], dense: the layout of the context over the first nmoduli - 1 moduli (callers chain
 *           through that context to drop further moduli)
 *   NFLHIP_FORM_COEFF  the formula word by word, one streaming pass.
 *   NFLHIP_FORM_NTT    input and output in the order nflhip_ntt_fwd_dev produces: the dropped row is inverse-transformed under q,
 *                      d_i = (h - r) mod p_i forward-transformed under p_i, y_i = (x_i + NTT_i(d_i)) q^-1 mod p_i, so that
 *                      ntt_inv'(rescale_ntt(ntt_fwd(x))) == rescale_coeff(x) word for word (ntt_inv' of the smaller context).
 *                      Rows below 32 KiB run in one launch with no scratch (it can be captured into a hipGraph); longer rows,
 *                      and contexts created under NFLHIP_VARIANT=hipcc, compose the transform launchers around context-owned
 *                      scratch (allocated on first use and when the batch grows).  NFLHIP_FORM_NTT | NFLHIP_RESCALE_COMPOSED
 *                      selects the composed plan whatever the shape, NFLHIP_FORM_NTT | NFLHIP_RESCALE_FUSED the one-launch
 *                      kernel (rows up to 32 KiB, NFLHIP_ERR_UNSUPPORTED beyond): each is the other's cross-check, same words.
 * NFLHIP_ERR_INVALID: fewer than two moduli, a NULL pointer, an unknown form, an output that overlaps the input (the strides
 * differ, so neither variant works in place), or a cyclic row context.  Every argument is checked before the device is touched. */
#define NFLHIP_RESCALE_COMPOSED 0x100
#define NFLHIP_RESCALE_FUSED 0x200
int nflhip_rescale_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, int form, void *stream);
int nflhip_rescale(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, int form);   /* staged host variant */

/* ---- sums of products across polynomials: dot and matrix-vector forms ----------------------
 * The inner step of an XPIR reply (out[r] = sum_j db[r][j] (.) query[j]), of key switching (sum_j digit_j (.) key_j), of
 * relinearisation and of any linear layer over ciphertexts.  For every group g < groups, row m and position i
 *     out[g][m][i] = (addend[g][m][i] + sum_{j < terms} a(g,j)[m][i] * b(g,j)[m][i]) mod p_m
 * as the canonical word in [0, p_m); the inputs are canonical words (the contract of the element-wise MUL).  The operation does not
 * look at the form: callers pass NTT-form data.  One pass: the products are accumulated unreduced in a double-width word and
 * reduced once per 16 terms, the accumulator never touches memory, and every input word is read once (a shared operand once per
 * four groups, below).
 *   operand  polynomial (g, j) starts (g * group_stride + j * term_stride) polynomials after ptr; group_stride 0 = shared by all
 *            groups.  A plain dot: {A, terms, 1} against {B, terms, 1}; a matrix times a shared vector: b = {V, 0, 1}; a key laid
 *            out [term][component]: b = {K + c, 0, 2}; one shared polynomial: both strides 0.
 *   out      dense [groups][nmoduli][degree]
 *   addend   NULL, or dense like out; it may be out itself (the same first byte): out += sum
 *   flags    0, or NFLHIP_DOT_UNTILED.  When one operand is shared (group_stride 0) and groups > 1 a thread serves four consecutive
 *            groups per load of the shared words; NFLHIP_DOT_UNTILED forces one group per pass -- each plan is the other's
 *            cross-check, same words.
 * The pointer form computes ONE output polynomial from terms <= NFLHIP_DOT_MAX_POINTERS polynomials anywhere in device memory:
 * d_a / d_b are HOST arrays of device pointers, which travel to the kernel by value (longer sums chain through the addend).
 * The _dev entries allocate nothing, use no scratch and do not synchronise: they can be captured into a hipGraph.
 * The host variant takes a dense as [groups][terms] and b as [groups][terms], or as [terms] when b_shared is non-zero.
 * NFLHIP_ERR_INVALID: a NULL context or pointer, terms == 0 or terms > 2^31 (terms > 16 in the pointer form), unknown flag bits, an output that
 * overlaps any byte of an operand's extent -- the (groups - 1) * group_stride + (terms - 1) * term_stride + 1 polynomials from its
 * ptr --, an addend that overlaps the output other than exactly, or a cyclic row context.  groups == 0 returns NFLHIP_OK and
 * touches nothing.  Every argument is checked before the device is touched. */
typedef struct nflhip_dot_operand {
  const void *ptr;      /* device pointer to element (0,0) */
  size_t group_stride;  /* polynomials from (g,j) to (g+1,j); 0 = shared by all groups */
  size_t term_stride;   /* polynomials from (g,j) to (g,j+1) */
} nflhip_dot_operand;
#define NFLHIP_DOT_UNTILED 0x100
#define NFLHIP_DOT_MAX_POINTERS 16
int nflhip_dot_dev(nflhip_ctx *ctx, void *d_out, const nflhip_dot_operand *a, const nflhip_dot_operand *b, const void *d_addend,
                   size_t groups, size_t terms, int flags, void *stream);
int nflhip_dot_ptrs_dev(nflhip_ctx *ctx, void *d_out, const void *const *d_a, const void *const *d_b, size_t terms,
                        const void *d_addend, void *stream);
int nflhip_dot(nflhip_ctx *ctx, void *h_out, const void *h_a, const void *h_b, size_t groups, size_t terms, int b_shared);   /* staged host variant */

/* ---- sums of products, several outputs: a small matrix product over polynomials ---------------
 * One first operand against `outputs` second operands, each shared by every group:
 *     d_outs[o][g][m][i] = (sum_{j < terms} a(g,j)[m][i] * b_o(j)[m][i]) mod p_m          o < outputs <= NFLHIP_DOT_MULTI_MAX_OUTPUTS
 * as the canonical word; b_o(j) starts j * b_term_stride polynomials after d_bs[o]; every d_outs[o] is dense
 * [groups][nmoduli][degree].  Word for word nflhip_dot_dev(d_outs[o], a, {d_bs[o], 0, b_term_stride}, NULL, groups, terms) for
 * every o, in ONE launch: replies to several XPIR queries, a linear layer with several output channels, the inner products of a
 * hoisted rotation (a = the digits, b_o = a component of a Galois key).  Up to 8 terms a thread loads its words of `a` once and
 * walks the outputs, so `a` is read once per call and b_o once per two groups; with more terms the terms are walked per output
 * as nflhip_dot_dev does.  d_outs and d_bs are HOST arrays of device pointers, which travel to the kernel by value: nothing is
 * allocated, no scratch, no synchronisation, and the call can be captured into a hipGraph.
 *   flags    0, or NFLHIP_DOT_UNTILED: one group per pass instead of two -- each plan is the other's cross-check, same words.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context or pointer, outputs == 0 or > 32, terms == 0 or > 2^31, unknown flag bits,
 * an extent that overflows, an output that overlaps any byte of the extent of `a`, of ANY b_o -- the (terms - 1) * b_term_stride
 * + 1 polynomials from d_bs[o] -- or of another output, or a cyclic row context.  The b pointers may alias each other.
 * groups == 0 returns NFLHIP_OK and touches nothing. */
#define NFLHIP_DOT_MULTI_MAX_OUTPUTS 32
int nflhip_dot_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const nflhip_dot_operand *a, const void *const *d_bs,
                         size_t b_term_stride, size_t outputs, size_t groups, size_t terms, int flags, void *stream);

/* ---- gadget decomposition: base-2^w digits of RNS rows ---------------------------------------
 * The first step of every key switch (relinearisation, a rotation's Galois key, an XPIR / SealPIR reply): a coefficient-form
 * polynomial is split into small "digit" polynomials whose sum of products against a key is what nflhip_dot_dev computes.
 * Context with nm = nmoduli moduli of `bits` = limb_bits - 2 bits (2^(bits-1) < p < 2^bits); digit width w, B = 2^w,
 * l = ceil(bits / w) digits per word, terms = nm * l (nflhip_decompose_terms).  Term j = m * l + t is digit t of row m.  For the
 * canonical word x = in[b][m][i]:
 *   unsigned (default)     d_t = (x >> w t) & (B - 1)
 *   NFLHIP_DECOMP_SIGNED   c = x if x <= (p_m - 1) / 2 else x - p_m;  r_0 = c;  for t < l - 1: d_t = ((r_t + B/2) mod B) - B/2 in
 *                          [-B/2, B/2), r_(t+1) = (r_t - d_t) / B;  the top digit d_(l-1) = r_(l-1) takes the carry and is not
 *                          reduced: |d_(l-1)| <= B/2 (derived in nfllib_amd/csrc/kernels_decompose.hip)
 * so that sum_t d_t B^t = x (unsigned) or c (signed), congruent to x mod p_m; B^t = 2^(w t) < p_m is its own residue.
 *   input    [batch][nmoduli][degree] canonical words, always in COEFFICIENT form
 *   output   NFLHIP_FMT_WORDS            dense [batch][terms][nmoduli][degree]: word (b, j, m', i) = d if d >= 0 else p_m' + d -- the
 *                                        digit spread over every row as nflhip_expand_small_dev spreads a compact value; what
 *                                        nflhip_dot_dev reads with {D, terms, 1}.  1 <= w <= bits - 1.
 *            NFLHIP_FMT_I8 / I16 / I32   dense [batch][terms][degree], one signed integer per coefficient (the compact format of
 *                                        nflhip_operand); additionally w <= 7 / 15 / 31, which holds the signed top digit +B/2 too
 *   flags    NFLHIP_FORM_COEFF or NFLHIP_FORM_NTT, | NFLHIP_DECOMP_SIGNED, | one plan flag (NTT form only).
 *            NFLHIP_FORM_NTT (words output only): each of the batch * terms digit polynomials is forward-transformed -- word for
 *            word what nflhip_ntt_fwd_dev makes of the coefficient-form output.  Rows of up to 2048 words run in ONE launch (a workgroup
 *            per digit polynomial, one row in LDS, 1x the output of traffic); longer rows, and contexts created under
 *            NFLHIP_VARIANT=hipcc, write the digits and run the context's forward transform over them in place.
 *            NFLHIP_DECOMP_COMPOSED selects the latter whatever the shape, NFLHIP_DECOMP_FUSED the one-launch kernel (rows up to
 *            32 KiB, NFLHIP_ERR_UNSUPPORTED beyond): each is the other's cross-check, same words.
 * nflhip_gadget_mul_dev is the key-generation companion: out[b][j = (m, t)][m'][i] = in[b][m][i] 2^(w t) mod p_m for m' = m, 0
 * elsewhere; dense [batch][terms][nmoduli][degree].  A row-wise scalar: it does not look at the form of its input.  Per row m' of the
 * ring product sum_j D_j(x) G_j(y) = sum_t d_t B^t y = x y, so
 *     ntt_inv(dot(decompose(x, NTT), ntt_fwd(gadget_mul(y)), terms)) == polymul(x, y)     bit for bit.
 * nflhip_decompose_terms returns 0 for an invalid w or context.  NFLHIP_ERR_INVALID: a NULL context or pointer, w outside the limits
 * above, an unknown format or flag bit, the NTT form with a compact format, a plan flag without the NTT form or both plan flags, an
 * output that overlaps the input, a size that overflows size_t, more than 65535 terms, or a cyclic row context; every argument is
 * checked before the device is touched.  batch == 0 returns NFLHIP_OK and touches nothing.  The _dev entries allocate nothing and do
 * not synchronise: they can be captured into a hipGraph wherever nflhip_ntt_fwd_dev can; the coefficient form and the one-launch
 * kernel always can. */
#define NFLHIP_DECOMP_COMPOSED 0x100
#define NFLHIP_DECOMP_FUSED 0x200
#define NFLHIP_DECOMP_SIGNED 0x400
size_t nflhip_decompose_terms(const nflhip_ctx *ctx, int w);       /* nmoduli * ceil(bits / w); 0 for an invalid w or ctx */
int nflhip_decompose_dev(nflhip_ctx *ctx, void *d_out, int out_format, const void *d_in, size_t batch, int w, int flags, void *stream);
int nflhip_decompose(nflhip_ctx *ctx, void *h_out, int out_format, const void *h_in, size_t batch, int w, int flags);  /* staged host variant */
int nflhip_gadget_mul_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, int w, void *stream);

/* ---- RNS base conversion and mod-down by the last k moduli ------------------------------------
 * Base conversion carries a value from one set of RNS rows to another without forming it: the mod-up of hybrid key switching, BFV
 * multiplication, the scale-down by a special modulus, bootstrapping.  Coefficient form only (re-reading a residue mod p_i as an
 * integer mod p_j does not commute with the transforms).  Source rows S = [s0, s0 + ks), destination rows D = [d0, d0 + kd), both
 * inside [0, nmoduli), overlapping or not; Q = prod_{i in S} p_i, the source moduli pairwise distinct.  Per coefficient position,
 * x in [0, Q) the integer behind the canonical source words x_i:
 *     y_i = x_i (Q/p_i)^-1 mod p_i,   c_ij = (Q/p_i) mod p_j,   Q_j = Q mod p_j,   u = floor(sum_i y_i / p_i) in [0, ks)
 *   fast (flags 0)             out_j = (sum_i y_i c_ij) mod p_j = (x + u Q) mod p_j          -- x_j itself for j in S
 *   NFLHIP_BASECONV_CENTERED   out_j = (sum_i y_i c_ij - v Q_j) mod p_j,  v = floor((sum_i f_i + 2^59) / 2^60), f_i the fixed-point
 *                              image of y_i / p_i with 60 fraction bits: f_i = floor(y_i floor(2^124 / p_i) / 2^64) for 64-bit limbs,
 *                              f_i = y_i floor(2^60 / p_i) for 32- and 16-bit limbs.  v - u is 0 or 1: the output is the centred
 *                              representative of x (x below Q/2, x - Q from there on) reduced mod p_j, except that an x with
 *                              x/Q in [1/2, 1/2 + ks e / 2^60), e = 5/4 (64-bit limbs) or 2^(limb_bits - 2), may come out as x
 *                              itself.
 *   input, output   [batch][nmoduli][degree] both; only rows S are read, only rows D are written.  d_out == d_in is allowed (the
 *                   normal mod-up: every source word is read before a word of its position is written); any other overlap is refused.
 * nflhip_moddown_dev divides and rounds by P = the product of the LAST k moduli, 1 <= k <= nmoduli - 1: X in [0, Q_all) the integer
 * behind all rows, conv_j the conversion of the last k rows to row j,
 *     Y_j = (x_j - conv_j) P^-1 mod p_j        for j < nmoduli - k
 *   default               the centred conversion: Y = X / P rounded to nearest, except that a fraction in [1/2, 1/2 + k e / 2^60) may
 *                         round down.  For k = 1 this is nflhip_rescale_dev (coefficient form) wherever the fraction is outside that band.
 *   NFLHIP_MODDOWN_FLOOR  the fast conversion: Y = floor(X / P) - u, the approximate mod-down of the literature.
 *   input [batch][nmoduli][degree]; output the dense [batch][nmoduli - k][degree], the layout of the context over the first
 *   nmoduli - k moduli; the output never overlaps the input.  One pass: nmoduli rows read, nmoduli - k written.
 * The tables of a pair of ranges are built and uploaded on the FIRST call that names it (that call allocates and synchronises: make
 * it before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED); later calls allocate nothing, do not
 * synchronise and can be captured.  NFLHIP_ERR_INVALID: a NULL context or pointer, an empty range or one outside the context, k out
 * of range, unknown flag bits, a repeated source modulus (for the mod-down also a kept modulus that repeats a dropped one), a
 * refused overlap, a size that overflows size_t, or a cyclic row context; every argument is checked before the device is touched.
 * batch == 0 returns NFLHIP_OK and touches nothing (it builds no tables: the warm-up before a capture is a call with batch >= 1).
 * The host variants stage both sides.  nflhip_baseconv accepts h_out == h_in; with h_out != h_in it writes EVERY row of h_out --
 * rows D converted, the other rows copied from h_in -- unlike the device entry, which leaves the rows of d_out outside D as they are. */
#define NFLHIP_BASECONV_CENTERED 0x100
#define NFLHIP_MODDOWN_FLOOR 0x100
int nflhip_baseconv_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd,
                        int flags, void *stream);
int nflhip_baseconv(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags);   /* staged host variant */
int nflhip_moddown_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t k, int flags, void *stream);
int nflhip_moddown(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags);   /* staged host variant */

/* ---- RNS base conversion and mod-down, NTT form ------------------------------------------------
 * The same two maps on NTT-form data, so that a hybrid key switch never leaves the NTT form: the mod-up of a digit and the final
 * mod-down are one call each, around nflhip_dot_dev.  Input and output words are in the order nflhip_ntt_fwd_dev produces; the
 * semantics are those of the coefficient-form entries above, word for word (same ranges, same `flags` = NFLHIP_BASECONV_CENTERED /
 * NFLHIP_MODDOWN_FLOOR, same rounding band, same first-call table upload, same errors):
 *   nflhip_baseconv_ntt_dev   out row j = NTT_j(conv_j(INTT_i(in row i), i in S)) for j in D, conv the fast or the centred map of
 *                             nflhip_baseconv_dev.  For j in D and S this is the input row itself (the words are canonical): in
 *                             place (d_out == d_in, allowed; any other overlap is refused) the final words of those rows are the
 *                             input's, out of place they are copied.  Rows of d_out outside D stay as they are.
 *                                 ntt_inv(baseconv_ntt(ntt_fwd(x))) == baseconv(x)   on rows D, when D is the whole context;
 *                             in general every written row is the forward transform of the coefficient-form entry's row.
 *   nflhip_moddown_ntt_dev    Y_j = (x_j - NTT_j(conv_j(INTT(last k rows)))) P^-1 mod p_j, dense [batch][nmoduli - k][degree]:
 *                                 ntt_inv'(moddown_ntt(ntt_fwd(x))) == moddown(x),   ntt_inv' of the context over the first
 *                             nmoduli - k moduli.  For k = 1, outside the band, it equals nflhip_rescale_dev(..., NFLHIP_FORM_NTT).
 * Two plans compute the same words, each the other's cross-check; `flags` may carry at most one plan flag:
 *   NFLHIP_BASECONV_NTT_FUSED     ONE launch: a workgroup per polynomial keeps the ks inverse-transformed source rows, one work row
 *                                 and (centred conversion, i.e. NFLHIP_BASECONV_CENTERED or the mod-down without
 *                                 NFLHIP_MODDOWN_FLOOR) one row of corrections in LDS.  It needs
 *                                     (ks + 1 + c) * degree * (limb_bits / 8) <= 65536 bytes,   c = 1 centred, 0 otherwise;
 *                                 beyond that the flag gives NFLHIP_ERR_UNSUPPORTED.  ks rows read, the rows of D outside S written.
 *   NFLHIP_BASECONV_NTT_COMPOSED  the source rows are gathered into context-owned scratch and inverse-transformed, the coefficient-
 *                                 form kernel converts them, the result is forward-transformed (and, for the mod-down, combined
 *                                 with the kept rows in one more pass): every shape, any transform launcher of the project.  In
 *                                 place with D the whole context, the rows of S pass through their coefficient form on the way.
 *   neither                       the one-launch kernel when it fits and a row has up to 2048 words, the composed plan otherwise
 *                                 and for contexts created under NFLHIP_VARIANT=hipcc.
 * Both plans can be captured into a hipGraph after a warm-up call: the first call for a pair of ranges uploads its tables, and the
 * composed plan allocates its scratch and its child contexts on first use and whenever the batch grows -- while capturing each of
 * these is NFLHIP_ERR_UNSUPPORTED and the stream stays usable.  A graph that replays the composed plan must not run concurrently
 * with other composed calls on the same context (the scratch is shared; outside a capture calls on different streams are ordered by
 * events).  NFLHIP_ERR_INVALID additionally for both plan flags at once.  batch == 0 returns NFLHIP_OK and touches nothing. */
#define NFLHIP_BASECONV_NTT_COMPOSED 0x200
#define NFLHIP_BASECONV_NTT_FUSED 0x400
int nflhip_baseconv_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd,
                            int flags, void *stream);
int nflhip_baseconv_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags);   /* staged host variant */
int nflhip_moddown_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t k, int flags, void *stream);
int nflhip_moddown_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags);   /* staged host variant */

/* ---- hybrid (RNS-digit) key switching, NTT form -------------------------------------------------
 * The whole key switch around the entries above as ONE call: mod-up of every digit, the two inner products against the key, the
 * mod-down of both sums.  The context has nm = nmoduli moduli of which the LAST k_special are the special ones, 1 <= k_special <=
 * nm - 1; L = nm - k_special.  The digits are contiguous groups of alpha rows of the first L rows, 1 <= alpha <= L:
 * dnum = ceil(L / alpha) (nflhip_keyswitch_digits), S_d = [d alpha, min((d + 1) alpha, L)) -- the last digit may be short.
 *   in           [batch][L][degree], NTT form, the dense layout of the context over the first L moduli (what nflhip_moddown_ntt_dev returns)
 *   key          [dnum][2][nmoduli][degree], NTT form over the full context, shared by the batch ([term][component])
 *   out0, out1   [batch][L][degree], NTT form
 * Definition, word for word: X = in embedded into the first L rows of an nm-row polynomial;
 *     U_d   = nflhip_baseconv_ntt_dev(X, s0 = d alpha, ks = |S_d|, d0 = 0, kd = nm)       fast, or centred with NFLHIP_KEYSWITCH_CENTERED
 *     acc_c = sum_d U_d (.) key[d][c]   row by row mod p_j                                what nflhip_dot_dev gives
 *     out_c = nflhip_moddown_ntt_dev(acc_c, k_special)                                    rounding, or NFLHIP_KEYSWITCH_FLOOR
 * including the centred band and the rescale-band behaviour of those entries: no new rounding rule.  Three plans give the same
 * words, each the others' cross-check; `flags` may carry at most one plan flag:
 *   NFLHIP_KEYSWITCH_SEQUENCE  the definition itself, run through the entries above over context-owned scratch: dnum base
 *                              conversions, two inner products, one mod-down of 2 batch polynomials.  No kernel of its own.
 *   NFLHIP_KEYSWITCH_COMPOSED  ONE inverse transform over the L rows, one streaming pass that writes every row of every U_d in
 *                              coefficient form, one forward transform over batch dnum polynomials, then the inner products and
 *                              the mod-down as above.  Every shape.
 *   NFLHIP_KEYSWITCH_FUSED     ONE launch up to the two sums: a workgroup per polynomial keeps the L inverse-transformed rows and
 *                              one work row in LDS and accumulates both components in registers; then the mod-down.  It needs
 *                                  (L + 1) * degree * (limb_bits / 8) [+ 2 * dnum * degree, centred] <= 65536 bytes
 *                              and rows of at most 2048 words; beyond that the flag gives NFLHIP_ERR_UNSUPPORTED.
 *   none                       the one-launch kernel where it fits (not for contexts created under NFLHIP_VARIANT=hipcc); past it the
 *                              composed plan for rows above 2048 words, the sequence for shorter ones.
 * The first call for a (k_special, alpha), or for a larger batch, builds tables and allocates scratch (it synchronises): make it
 * before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED and the stream stays usable.  Calls on different
 * streams are ordered on the scratch by an event; a replaying graph must not run concurrently with other key switches of the context.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0, k_special or alpha out of range, unknown
 * flag bits or two plan flags, a size that overflows size_t, any overlap among out0, out1, in and key, a cyclic row context, a
 * repeated modulus inside a digit or among the special rows.  batch == 0 returns NFLHIP_OK and touches nothing.
 * The host variant stages in, key and both outputs. */
#define NFLHIP_KEYSWITCH_CENTERED 0x100
#define NFLHIP_KEYSWITCH_FLOOR 0x200
#define NFLHIP_KEYSWITCH_COMPOSED 0x400
#define NFLHIP_KEYSWITCH_FUSED 0x800
#define NFLHIP_KEYSWITCH_SEQUENCE 0x1000
size_t nflhip_keyswitch_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha);   /* dnum; 0 for invalid arguments */
int nflhip_keyswitch_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch,
                             size_t k_special, size_t alpha, int flags, void *stream);
int nflhip_keyswitch_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch,
                         size_t k_special, size_t alpha, int flags);   /* staged host variant */

/* ---- hoisted rotations: one mod-up shared by many Galois key switches ---------------------------
 * A ciphertext (c0, c1) rotated by `count` amounts in one call -- the linear transforms over slots (matrix-vector products, the
 * baby steps of BSGS, traces, CoeffToSlot) rotate one ciphertext many times, and every key switch of c1 repeats the same mod-up.
 * The context is that of the key switch above: nm moduli, the last k_special special, L = nm - k_special, digits of alpha rows,
 * dnum = nflhip_keyswitch_digits.
 *   c0, c1        [batch][L][degree], NTT form; c0 may be NULL
 *   keys[m]       [dnum][2][nmoduli][degree], NTT form, shared by the batch; one device pointer per rotation (a HOST array)
 *   ks[m]         odd, taken mod 2 degree (a HOST array); m < count <= NFLHIP_ROTATE_MAX_OUTPUTS
 *   out0s[m], out1s[m]   [batch][L][degree], NTT form (HOST arrays of device pointers)
 * Definition, word for word, for every m:
 *     (d0, d1) = nflhip_keyswitch_ntt_dev(c1, keys[m], k_special, alpha)    NFLHIP_ROTATE_CENTERED / _FLOOR as NFLHIP_KEYSWITCH_*
 *     y0       = d0 + c0   row by row mod p_j, canonical                    (y0 = d0 when c0 is NULL)
 *     out0s[m] = sigma^NTT_ks[m](y0),   out1s[m] = sigma^NTT_ks[m](d1)      nflhip_automorphism_dev, NFLHIP_FORM_NTT
 * THE PERMUTATION COMES LAST, after the mod-down: the mod-up U_d of c1 then does not depend on m, so it is computed once, every
 * plan gives the same words as the sequence, and only 2 L rows per rotation are permuted instead of dnum nm.
 * The key convention that goes with it: keys[m] switches from s to sigma_(k^-1)(s),
 *     key[d][0] = -a_d sigma_(k^-1)(s) + e_d + P g_d s,   key[d][1] = a_d       (g_d, P as for the key switch),
 * which is the usual Galois key for k with the NTT-form automorphism by k^-1 mod 2 degree applied to both components of every
 * term, once at key generation.  Then out0 + out1 s ~ sigma_k(c0 + c1 s), with the noise of one key switch.
 * Plans, same words; `flags` may carry at most one plan flag:
 *   NFLHIP_ROTATE_SEQUENCE  the definition itself per rotation: nflhip_keyswitch_ntt_dev (its default plan) into scratch, the
 *                           element-wise ADD of c0 (nflhip_pointwise_dev; for buffers off 16 bytes or of no whole number of
 *                           16-byte groups nflhip_dot_dev as c0 + d0 (.) 1), two nflhip_automorphism_dev.  No kernel of its own.
 *   NFLHIP_ROTATE_HOISTED   the mod-up ONCE (per-digit nflhip_baseconv_ntt_dev for rows up to 2048 words; above that, or for a
 *                           context created under NFLHIP_VARIANT=hipcc, one inverse transform, the all-digit mod-up pass and one
 *                           forward transform); ONE nflhip_dot_multi_dev-style launch for the 2 count inner products, the digits
 *                           read once; ONE nflhip_moddown_ntt_dev of 2 count batch polynomials; ONE launch that adds c0 and permutes.
 *   none                    hoisted for count >= 2, the sequence for count == 1.
 * Scratch of the hoisted plan, context-owned, in polynomials of nm rows (p) and of L rows (q):
 *     batch (1 p | 1 q) [the embedded | inverse-transformed c1]  +  batch dnum p [U]  +  2 count batch p [S]  +  2 count batch q [Y];
 * of the sequence 3 batch q + 1 q, besides the key switch's own.
 * The first call for a (k_special, alpha, plan, modes), or for a larger batch or count * batch, builds tables and allocates (it
 * synchronises): make it before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED and the stream stays
 * usable.  Calls on different streams are ordered on the scratch by an event; a replaying graph must not run concurrently with
 * other rotations or key switches of the context.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0 (except c0), count == 0 or > 16, an even k,
 * k_special or alpha out of range, unknown flag bits or two plan flags, a size that overflows size_t, any overlap among the
 * 2 count outputs or of an output with c0, c1 or a key, a cyclic row context, a repeated modulus inside a digit or among the
 * special rows.  Keys may repeat, a k may repeat, k = 1 is allowed.  batch == 0 returns NFLHIP_OK and touches nothing.
 * The host variant stages c0, c1, every key and every output. */
#define NFLHIP_ROTATE_MAX_OUTPUTS 16
#define NFLHIP_ROTATE_CENTERED 0x100
#define NFLHIP_ROTATE_FLOOR 0x200
#define NFLHIP_ROTATE_SEQUENCE 0x1000
#define NFLHIP_ROTATE_HOISTED 0x2000
int nflhip_rotate_hoisted_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                  const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special,
                                  size_t alpha, int flags, void *stream);
int nflhip_rotate_hoisted_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                              const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special,
                              size_t alpha, int flags);   /* staged host variant */

/* ---- weighted sums of automorphisms: several permuted inputs, each times a weight, into ONE output -------------
 * The primitive behind linear transforms over slots (a matrix-vector product by diagonals, the inner sums of BSGS, CoeffToSlot):
 *     out[g][j][i] = addend[g][j][i] + sum_{t < terms} w_t[j][i] * in_t[g][j][src_{k_t}(i)]      mod p_j, canonical,
 * where in_t[..][src_k(i)] is what nflhip_automorphism_dev with NFLHIP_FORM_NTT writes at i (2 rev(src_k(i)) + 1 =
 * k (2 rev(i) + 1) mod 2 degree), g < batch, j < rows, i < degree.
 *   rows          the number of leading moduli the layout covers, 1 <= rows <= nmoduli
 *   ins[t], out, addend   [batch][rows][degree], canonical words
 *   weights[t]    [>= rows][degree] with row stride degree, shared by the batch; rows past `rows` are not read
 *   ins, weights, ks      HOST arrays; 1 <= terms <= NFLHIP_MAC_MAX_TERMS; every ks[t] odd, taken mod 2 degree; k = 1 is allowed;
 *                 ins may repeat, weights may repeat
 *   addend        may be NULL, and may be `out` exactly (accumulation in place)
 * The products are accumulated unreduced in a double-width word and reduced once (16 terms never wrap it, see "sums of
 * products"); the result is exact.  One launch; the pointers travel by value in the kernel arguments, nothing is allocated and
 * the call can be captured into a hipGraph.  flags: 0, or NFLHIP_MAC_DOUBLE_BUFFER (two staging buffers, the next term's loads in
 * flight while a term is consumed, instead of one: the alternative the default was measured against and ahead of; same words).
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context or pointer with batch != 0 (except addend), terms == 0 or > 16, rows == 0
 * or > nmoduli, an even k, unknown flag bits, a size that overflows size_t, a cyclic row context, the addend overlapping `out`
 * without being `out`, `out` overlapping an input or a weight.  batch == 0 returns NFLHIP_OK and touches nothing.
 * The host variant stages every input, every weight, the addend and the output. */
#define NFLHIP_MAC_MAX_TERMS 16
#define NFLHIP_MAC_DOUBLE_BUFFER 0x1
int nflhip_automorphism_mac_dev(nflhip_ctx *ctx, void *d_out, const void *d_addend, const void *const *d_ins,
                                const void *const *d_weights, const uint64_t *ks, size_t terms, size_t batch, size_t rows,
                                int flags, void *stream);
int nflhip_automorphism_mac(nflhip_ctx *ctx, void *h_out, const void *h_addend, const void *const *h_ins,
                            const void *const *h_weights, const uint64_t *ks, size_t terms, size_t batch, size_t rows,
                            int flags);   /* staged host variant */

/* ---- slot linear transforms: weighted sums of rotations, one mod-down ---------------------------
 * sum_m pt_m (.) sigma_{k_m}(ct) for plaintext diagonals pt_m in one call: what the callers of hoisted rotations want, without
 * the rotations themselves.  The key-switch sums are multiplied by the diagonals and added up while they are still in the
 * extended basis (all nmoduli rows), then modded down ONCE ("double hoisting"): 2 batch polynomials for any count.
 * The context, k_special, L = nmoduli - k_special, the digits of alpha rows and dnum are those of the key switch above.
 *   c0, c1, out0, out1   [batch][L][degree], NTT form; c0 may be NULL
 *   keys[m]       [dnum][2][nmoduli][degree], the key convention of the hoisted rotations (from s to sigma_(k^-1)(s)); NULL if
 *                 and only if ks[m] = 1 mod 2 degree is meant as the unrotated diagonal, which needs no key switch (a HOST array)
 *   weights[m]    [nmoduli][degree], the diagonal in NTT form over ALL nmoduli moduli, shared by the batch (a HOST array)
 *   ks[m]         odd, taken mod 2 degree (a HOST array); m < count <= NFLHIP_LINTRANS_MAX_TERMS
 * Definition, word for word ("keyed": keys[m] != NULL):
 *     U_d     as nflhip_keyswitch_ntt_dev forms it from c1                                 (nmoduli rows)
 *     S_{m,c} = sum_d U_d (.) keys[m][d][c]                 for keyed m                    nflhip_dot_dev, nmoduli rows
 *     A_c     = sum_{keyed m} w_m (.) sigma^NTT_{k_m}(S_{m,c})                             nflhip_automorphism_mac_dev, rows = nmoduli
 *     Y_c     = nflhip_moddown_ntt_dev(A_c, k_special)      (zero when no m is keyed)      NFLHIP_LINTRANS_FLOOR as NFLHIP_MODDOWN_FLOOR
 *     out0    = Y_0 + sum_{all m} w_m (.) sigma^NTT_{k_m}(c0)     (the sum absent when c0 is NULL)      rows = L
 *     out1    = Y_1 + sum_{unkeyed m} w_m (.) c1                                           rows = L
 * THESE ARE NOT THE WORDS OF sum_m w_m (.) nflhip_rotate_hoisted_ntt_dev(...): one rounding of the sum replaces `count`
 * roundings of its terms.  It is the same function of the plaintext with less noise: out0 + out1 s = sum_m pt_m sigma_{k_m}(c0 +
 * c1 s) + e with |e| at most keyed * degree * |pt|_inf times the bound of one key switch (tests/test_lintrans_cpu.py).
 * Plans, same words; `flags` may carry at most one plan flag:
 *   NFLHIP_LINTRANS_SEQUENCE  the definition through existing entries: per-digit nflhip_baseconv_ntt_dev; per keyed (m, c)
 *                             nflhip_dot_dev, nflhip_automorphism_dev on the nmoduli-row sum, nflhip_dot_dev of one term against
 *                             the weight with the addend in place; the mod-down; nflhip_automorphism_dev and nflhip_dot_dev with
 *                             the addend in place on the L-row child context.  No kernel of its own: the cross-check.
 *   NFLHIP_LINTRANS_HOISTED   the mod-up once (the two routes of the hoisted rotations); ONE nflhip_dot_multi_dev-style launch into
 *                             S = [2 keyed][batch][nmoduli][degree]; ONE launch of the weighted-sum kernel for both A_c; ONE
 *                             nflhip_moddown_ntt_dev of 2 batch polynomials straight into out0 / out1 when out1 follows out0 in
 *                             memory, else two; the weighted-sum kernel on L rows with the addend in place, once for out0 (the
 *                             c0 terms) and once for out1 (the unkeyed terms), where there are any.
 *   none                      hoisted (measured ahead of the sequence for any number of keyed terms).
 * Scratch, context-owned, in polynomials of nmoduli rows (p) and of L rows (q): hoisted
 *     batch (1 p | 1 q) [the embedded | inverse-transformed c1]  +  batch dnum p [U]  +  2 keyed batch p [S]  +  2 batch p [A];
 * the sequence batch (1 + dnum + 2 + 2) p + batch q; nothing when no term is keyed (the sequence: batch q when c0 is given).
 * The first call for a (k_special, alpha, plan, modes), or for a larger batch, keyed * batch or mod-down, builds tables and
 * allocates (it synchronises): make it before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED, nothing
 * is enqueued and the stream stays usable.  Calls on different streams are ordered on the scratch by an event; a replaying graph
 * must not run concurrently with other linear transforms, rotations or key switches of the context.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0 (except c0, and keys[m] where ks[m] = 1
 * mod 2 degree), a NULL key with another k, a NULL weight, count == 0 or > 16, an even k, k_special or alpha out of range, unknown
 * flag bits or two plan flags, a size that overflows size_t, out0 overlapping out1, an output overlapping c0, c1, a key or a
 * weight, a cyclic row context, a repeated modulus inside a digit or among the special rows.  Keys, weights and ks may repeat.
 * batch == 0 returns NFLHIP_OK and touches nothing.  The host variant stages c0, c1, every key, every weight and both outputs. */
#define NFLHIP_LINTRANS_MAX_TERMS 16
#define NFLHIP_LINTRANS_CENTERED 0x100
#define NFLHIP_LINTRANS_FLOOR 0x200
#define NFLHIP_LINTRANS_SEQUENCE 0x1000
#define NFLHIP_LINTRANS_HOISTED 0x2000
int nflhip_lintrans_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1,
                            const void *const *d_keys, const void *const *d_weights, const uint64_t *ks, size_t count,
                            size_t batch, size_t k_special, size_t alpha, int flags, void *stream);
int nflhip_lintrans_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1,
                        const void *const *h_keys, const void *const *h_weights, const uint64_t *ks, size_t count,
                        size_t batch, size_t k_special, size_t alpha, int flags);   /* staged host variant */

/* ---- ciphertext multiplication: the tensor product, and the product with relinearisation --------
 * THE TENSOR PRODUCT of two degree-1 ciphertexts (a0, a1), (b0, b1), row by row mod p_j on the `rows` leading moduli of the context,
 * 1 <= rows <= nmoduli:
 *     out0 = a0 (.) b0,     out1 = a0 (.) b1 + a1 (.) b0,     out2 = a1 (.) b1          every block [batch][rows][degree], canonical
 * One streaming pass, nothing allocated, capturable.  out1 is accumulated unreduced in a double-width word and reduced once.  It
 * does not look at the form (the product of NTT-form operands is the NTT form of the negacyclic product).  b0 == b1 == NULL: the
 * SQUARE, a0^2, 2 a0 a1, a1^2, with two reads instead of four.  An output may be exactly an input (the same first byte); any
 * other overlap of an output with an input or with another output is NFLHIP_ERR_INVALID.  Buffers off 16 bytes and rows shorter
 * than 16 bytes take a word variant of the kernel.  flags: 0.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0 (b0 and b1 both NULL is the square, one of
 * them NULL is an error), rows out of range, flag bits, a size that overflows size_t, such an overlap, a cyclic row context.
 * batch == 0 returns NFLHIP_OK and touches nothing.  The host variant stages the inputs and the three outputs.
 *
 * THE PRODUCT WITH RELINEARISATION.  The context, k_special, L = nmoduli - k_special, the digits of alpha rows and dnum are those
 * of the key switch above.
 *   a0, a1, b0, b1   [batch][L][degree], NTT form; b0 == b1 == NULL: the square of (a0, a1)
 *   key              [dnum][2][nmoduli][degree] exactly as nflhip_keyswitch_ntt_dev takes it: the key from s^2 to s
 *   out0, out1       [batch][L][degree], NTT form; with NFLHIP_MULRELIN_RESCALE [batch][L - 1][degree]
 * Definition, word for word, with pi_j = P mod p_j, P the product of the special moduli:
 *     d0, d1, d2 = the tensor product of (a0, a1) and (b0, b1) on L rows
 *     U_d   as nflhip_keyswitch_ntt_dev forms it from d2                                        NFLHIP_MULRELIN_CENTERED as NFLHIP_KEYSWITCH_CENTERED
 *     A_c   = E(pi (.) d_c) + sum_d U_d (.) key[d][c]       E: the L rows embedded in nmoduli rows, the special rows 0; nflhip_dot_dev with addend
 *     out_c = nflhip_moddown_ntt_dev(A_c, k_special)                                            NFLHIP_MULRELIN_FLOOR as NFLHIP_MODDOWN_FLOOR
 *             with NFLHIP_MULRELIN_RESCALE: nflhip_moddown_ntt_dev(A_c, k_special + 1);  needs L >= 2
 * Without RESCALE these are the words of d_c + nflhip_keyswitch_ntt_dev(d2)_c: the mod-down computes (x_j - conv_j(special
 * rows)) P^-1 mod p_j, the special rows of A_c are those of the key-switch sum, and pi_j d_c P^-1 = d_c mod p_j, in both rounding
 * modes.  With RESCALE the sum is divided by P q_(L-1) in ONE rounding, (d_c + ks_c) / q_(L-1) rounded: the same
 * function of the plaintext as the product followed by two nflhip_rescale_dev, with less noise and K + L row transforms per
 * component instead of K + 2L -- not the words of the two-step way.  The result is a ciphertext over the first L - 1 moduli.
 * Plans, same words; `flags` may carry at most one plan flag:
 *   NFLHIP_MULRELIN_SEQUENCE  the definition through existing entries: the tensor product by nflhip_dot_dev on the context over the
 *                             first L moduli, the scaling by pi as a one-term nflhip_dot_dev against a constant polynomial, per-digit
 *                             nflhip_baseconv_ntt_dev, nflhip_dot_dev with the addend in place, the mod-down.  No kernel of its own:
 *                             the cross-check.
 *   NFLHIP_MULRELIN_MERGED    ONE launch of the tensor kernel that writes d2 straight into the mod-up's source buffer and pi d_c into
 *                             the two sums; the mod-up by the two routes of the hoisted rotations; nflhip_dot_dev twice with the
 *                             addend in place; ONE mod-down of 2 batch polynomials when out1 follows out0 in memory, else two.
 *   NFLHIP_MULRELIN_FUSED     ONE launch from the four inputs up to the two sums: the key switch's one-launch kernel with the source
 *                             rows formed as a1 (.) b1 at the load and pi d_c as the accumulators' carry-in; d0, d1, d2 never touch
 *                             memory.  The LDS bound of NFLHIP_KEYSWITCH_FUSED, unchanged; beyond it the flag gives
 *                             NFLHIP_ERR_UNSUPPORTED.
 *   none                      the one-launch kernel where it fits (not for contexts created under NFLHIP_VARIANT=hipcc), else merged
 *                             (DESIGN.md 5.19).
 * Scratch, context-owned, in polynomials of nmoduli rows (p) and of L rows (q): merged batch (1 p | 1 q) + batch dnum p + 2 batch p;
 * fused 2 batch p; the sequence batch (7 q + 3 p + dnum p + 2 p).
 * The first call for a (k_special, alpha, plan, modes), or for a larger batch, builds tables and allocates (it synchronises): make
 * it before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED, nothing is enqueued and the stream stays
 * usable.  Calls on different streams are ordered on the scratch by an event; a replaying graph must not run concurrently with
 * other multiplications of the context.  An output may be exactly an input: every read of the inputs precedes the mod-down that
 * writes the outputs.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0 (b0 and b1 both NULL is the square, one of
 * them NULL is an error), k_special or alpha out of range, RESCALE with L == 1, unknown flag bits or two plan flags, a size that
 * overflows size_t, out0 overlapping out1, an output overlapping the key, an output overlapping an input without being it, a
 * cyclic row context, a repeated modulus.  batch == 0 returns NFLHIP_OK and touches nothing.
 * The host variant stages the inputs, the key and both outputs. */
#define NFLHIP_MULRELIN_CENTERED 0x100
#define NFLHIP_MULRELIN_FLOOR 0x200
#define NFLHIP_MULRELIN_RESCALE 0x400
#define NFLHIP_MULRELIN_FUSED 0x800
#define NFLHIP_MULRELIN_SEQUENCE 0x1000
#define NFLHIP_MULRELIN_MERGED 0x2000
int nflhip_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1,
                          const void *d_b0, const void *d_b1, size_t batch, size_t rows, int flags, void *stream);
int nflhip_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1,
                      const void *h_b0, const void *h_b1, size_t batch, size_t rows, int flags);   /* staged host variant */
int nflhip_mulrelin_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0,
                            const void *d_b1, const void *d_key, size_t batch, size_t k_special, size_t alpha, int flags,
                            void *stream);
int nflhip_mulrelin_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0,
                        const void *h_b1, const void *h_key, size_t batch, size_t k_special, size_t alpha, int flags);   /* staged host variant */

/* ---- BFV multiplication: RNS scale-and-round by t/Q, the scale-invariant tensor product ---------
 * The scale-invariant product of BFV needs Y = round(t X / Q) carried from the rows Q u B onto the rows Q without forming the
 * integer (Halevi-Polyakov-Shoup).  The mod-down above cannot stand in: it divides by the LAST k rows and returns the leading ones;
 * here the leading rows are divided out, the value is multiplied by t first, and the result comes back onto the rows divided out.
 * The context has nm moduli p_0 ... p_{nm-1}, pairwise distinct over the rows used (anything else is NFLHIP_ERR_INVALID, as
 * nflhip_baseconv_dev refuses a repeated source modulus).  1 <= ks <= nm - 1.  S = [0, ks), Q = prod_S p_i.  D = [ks, nm),
 * kd = nm - ks, B = prod_D p_j.  t is a uint64_t with 1 <= t < 2^(limb_bits - 3): it is below every modulus, so coprime to all.
 * Per coefficient position, from canonical words x_r:
 *     z_r  = t * x_r mod p_r                                   every row r
 *     r_j  = conv_{S->j}(z)          the CENTRED conversion of nflhip_baseconv_dev (same f_i, same v, same band), j in D
 *                                   with NFLHIP_SCALE_ROUND_FLOOR the fast conversion (x + uQ) instead
 *     Y_j  = (z_j - r_j) * Q^-1 mod p_j                        j in D
 *     out_i = conv_{D->i}(Y)         the CENTRED conversion again, i in S      -> dense [batch][ks][degree]
 *     NFLHIP_SCALE_ROUND_KEEP:      stop at Y: output the kd rows Y_j, dense [batch][kd][degree]
 * With X_c the centred integer behind all nm rows, Y = round(t X_c / Q) mod B, whatever representative the rows hold (t B m = 0 on
 * D); a fraction inside [1/2, 1/2 + ks e / 2^60) may round down, and under FLOOR it is floor(t X / Q) - u.  out is the centred
 * representative of Y mod B reduced mod p_i, with the band of the second conversion at |Y| ~ B/2.  A BFV caller keeps
 * n Q^2 / 2 < Q B / 2 and t n Q / 2 + 1 < B / 2: then neither representation wraps and the second band is never reached (with
 * kd = L + 1 moduli of one width, roughly 2^(limb_bits - 3 - L) > t n).  The entries do not check the bound: they are defined for
 * every input.
 *   nflhip_scale_round_dev      coefficient form.  in [batch][nm][degree]; the output never overlaps the input.
 *   nflhip_scale_round_ntt_dev  NTT form in and out: out = NTT_S(scale_round(INTT(in))), under KEEP NTT_D of Y, the transforms of the
 *                               contexts over those moduli.  A composed plan: the input is copied into context-owned scratch and
 *                               inverse-transformed, the result is forward-transformed by the child context over the rows written.
 * Plans, same words: by default ONE kernel reads the nm rows, keeps the kd words Y in registers and writes the ks rows, where
 * ks <= 8 and kd <= 9; NFLHIP_SCALE_ROUND_TWO_PASS -- and every larger shape -- writes Y into context-owned scratch and converts it
 * with the kernel of nflhip_baseconv_dev (the cross-check).  With KEEP the flag changes nothing.
 * The tables of a (ks, t) are built and uploaded on the FIRST call that names it (that call allocates and synchronises: make it
 * before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED); the scratch of the two-pass plan and of the NTT
 * form, and the NTT form's child contexts, are allocated on first use and whenever the batch grows, likewise refused while
 * capturing.  A replaying graph must not run concurrently with other such calls of the context.  batch == 0 returns NFLHIP_OK and
 * touches nothing.  NFLHIP_ERR_INVALID, before the device is touched: a NULL context or pointer, ks or t out of range, unknown
 * flag bits, a repeated modulus, the output overlapping the input, a size that overflows size_t, a cyclic row context.
 *
 * nflhip_bfv_tensor_ntt_dev on the context over the first L + kb moduli, ks = L: the scale-invariant tensor product of two BFV
 * ciphertexts.  a0, a1, b0, b1 and out0, out1, out2 are [batch][L][degree], NTT form; b0 == b1 == NULL is the square.  Definition,
 * word for word:
 *     1. each input embedded in nm rows;  2. nflhip_baseconv_ntt_dev(S = [0, L), D = [0, nm), NFLHIP_BASECONV_CENTERED);
 *     3. nflhip_tensor_ntt_dev on nm rows;  4. nflhip_scale_round_ntt_dev on each component.
 * The four (or two) inputs go through the base extension as ONE batch, the three components through the scale-round as ONE batch of
 * 3 batch, in scratch the context owns.  An output may be exactly an input; flags are NFLHIP_SCALE_ROUND_FLOOR and
 * NFLHIP_SCALE_ROUND_TWO_PASS, passed through; the overlap and argument rules are those of nflhip_tensor_ntt_dev, every argument is
 * checked before the device is touched.  The relinearisation is an ordinary nflhip_keyswitch_ntt_dev of out2 on the context over
 * the first L + k_special moduli.  The host variants stage both sides. */
#define NFLHIP_SCALE_ROUND_FLOOR 0x100
#define NFLHIP_SCALE_ROUND_KEEP 0x200
#define NFLHIP_SCALE_ROUND_TWO_PASS 0x400
int nflhip_scale_round_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream);
int nflhip_scale_round(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags);   /* staged host variant */
int nflhip_scale_round_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream);
int nflhip_scale_round_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags);   /* staged host variant */
int nflhip_bfv_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1,
                              const void *d_b0, const void *d_b1, size_t batch, size_t ks, uint64_t t, int flags, void *stream);
int nflhip_bfv_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1,
                          const void *h_b0, const void *h_b1, size_t batch, size_t ks, uint64_t t, int flags);   /* staged host variant */

/* ---- leveled key switching and multiplication: one key for every level --------------------------
 * The two entries above on a ciphertext BELOW the context's top level -- what nflhip_mulrelin_ntt_dev with NFLHIP_MULRELIN_RESCALE
 * returns -- with the ONE top-level key: no context and no copy of the keys per level.  The context has nm = nmoduli moduli, the
 * last k_special of them special, L = nm - k_special, as above.  A level is l with 1 <= l <= L.
 *   live rows    A_l = [0, l) and [L, nm): l + k_special rows;  phys(r) = r for r < l, r + (L - l) from there on
 *   digits       S_d = [d alpha, min((d + 1) alpha, l)), dnum_l = ceil(l / alpha) (nflhip_keyswitch_level_digits); the last live digit
 *                may be shorter than it is at the top level, and alpha may exceed l (one short digit)
 *   key          unchanged: [dnum_L][2][nmoduli][degree], NTT form over the full context.  Only key[d][c][phys(r)] is read, for
 *                d < dnum_l and r < l + k_special: rows [l, L) of the key and digits >= dnum_l are never read
 *   in, a*, b*   [batch][l][degree], NTT form, the dense layout over the first l moduli
 *   out0, out1   [batch][l][degree]; nflhip_mulrelin_level_* with NFLHIP_MULRELIN_RESCALE [batch][l - 1][degree]
 * Definition, word for word: let C_l be the context over the moduli (p_j : j in A_l), in that order, and key_l[d][c][r] =
 * key[d][c][phys(r)].  A level-l call returns the words of nflhip_keyswitch_ntt_dev / nflhip_mulrelin_ntt_dev on C_l with key_l,
 * k_special and min(alpha, l).  For l = L it is that entry on this context itself.  The mod-down drops the k_special special rows
 * onto rows [0, l); with RESCALE the multiplication drops rows {l - 1} and [L, nm), the last k_special + 1 rows of C_l (it needs
 * l >= 2); the tensor product runs on l rows; pi_j = P mod p_j is unchanged.  No new rounding rule.
 * Flags, plans, modes and the overlap rules are those of the two entries above with L read as l throughout -- the one-launch
 * kernels need (l + 1) * degree * (limb_bits / 8) [+ 2 * dnum_l * degree, centred] <= 65536 bytes, so a top level that does not
 * fit may fit lower down.  The level context C_l is created at the first call for a (k_special, l) and lives with this context;
 * tables and scratch are per (k_special, alpha, l, plan, modes) and sized by l + k_special rows.  The first-call, larger-batch and
 * while-capturing rules are those of the key switch: the first call for a level while capturing is NFLHIP_ERR_UNSUPPORTED, nothing
 * is enqueued and the stream stays usable.  The key is read where it lies: the kernels that read it (the inner products and the two
 * one-launch kernels) have instances that know the parent's pitch and the hole of L - l rows.
 * NFLHIP_ERR_INVALID, nothing enqueued: what the two entries above refuse, and level == 0, level > L, RESCALE with level == 1.
 * The host variants stage the operands and the 2 dnum_l key polynomials that are read. */
size_t nflhip_keyswitch_level_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha, size_t level);   /* dnum at that level; 0 for invalid arguments */
int nflhip_keyswitch_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch,
                                   size_t k_special, size_t alpha, size_t level, int flags, void *stream);
int nflhip_keyswitch_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch,
                               size_t k_special, size_t alpha, size_t level, int flags);   /* staged host variant */
int nflhip_mulrelin_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0,
                                  const void *d_b1, const void *d_key, size_t batch, size_t k_special, size_t alpha, size_t level,
                                  int flags, void *stream);
int nflhip_mulrelin_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0,
                              const void *h_b1, const void *h_key, size_t batch, size_t k_special, size_t alpha, size_t level,
                              int flags);   /* staged host variant */

/* ---- sums of ciphertext products: one relinearisation for many products --------------------------
 * sum_j ct_a[j] * ct_b[j] per group -- an encrypted matrix times an encrypted vector, an inner product, a sum of squares -- with
 * the tensor products summed BEFORE the one key switch (lazy relinearisation): one mod-up, one key-switch inner product, one
 * mod-down and one key-switch noise term for `terms` products.
 *
 * nflhip_tensor_dot_ntt_dev: for every group g < groups, on the first `rows` moduli, row by row mod p_m,
 *     D0[g] = sum_{j < terms} a0(g,j) (.) b0(g,j)
 *     D1[g] = sum_{j < terms} (a0(g,j) (.) b1(g,j) + a1(g,j) (.) b0(g,j))
 *     D2[g] = sum_{j < terms} a1(g,j) (.) b1(g,j)                                  b0 == b1 == NULL: the squares, b = a
 *   a0, a1, b0, b1   nflhip_dot_operand, exactly as nflhip_dot_dev reads them, EXCEPT that a polynomial has `rows` rows: polynomial
 *                    (g, j) lies (g group_stride + j term_stride) * rows * degree words after ptr; group_stride 0: shared by all groups.
 *                    Canonical words; the form is not looked at (callers pass NTT form)
 *   d_out0..2        dense [groups][rows][degree], canonical
 *   One launch: the three sums stay unreduced in registers, D1 reduced every 8 terms, D0 and D2 every 16; the words
 *   are the canonical residues of the exact sums.  Allocates nothing, uses no scratch, does not synchronise, can be captured.
 *   NFLHIP_ERR_INVALID, before the device is touched: a NULL pointer; exactly one of b0 / b1 NULL; terms == 0 or above 2^31; rows
 *   outside [1, nmoduli]; flag bits; an extent that overflows size_t; an output that overlaps another output or any byte of an
 *   operand's extent (the (groups - 1) group_stride + (terms - 1) term_stride + 1 polynomials from its ptr); a cyclic row context.
 *   groups == 0: NFLHIP_OK, nothing touched.
 *   The host variant takes a0, a1 dense [groups][terms][rows][degree] and b0, b1 alike, or [terms][rows][degree] with b_shared.
 *
 * nflhip_mulrelin_dot_ntt_dev: nflhip_mulrelin_level_ntt_dev with (d0, d1, d2) replaced by (D0, D1, D2) and the batch by `groups`:
 *     A_c = E(pi (.) D_c) + sum_d U_d (.) key[d][c],  U_d the mod-up of D2;   out_c = the mod-down of A_c (RESCALE: one row more)
 *   operands         polynomials of `level` rows, strides in such polynomials; level == nmoduli - k_special is the top level
 *   d_key            the ONE top-level key [dnum_L][2][nmoduli][degree], read as at a level
 *   d_out0, d_out1   [groups][level][degree]; with NFLHIP_MULRELIN_RESCALE [groups][level - 1][degree]
 *   Without the rescale the words are D_c + nflhip_keyswitch_level_ntt_dev(D2)_c, in both mod-up modes and both roundings.
 *   Plans: NFLHIP_MULRELIN_SEQUENCE -- existing entries only (nflhip_dot_dev on the kept rows: D0 = dot(a0, b0), D1 = dot(a0, b1)
 *   then dot(a1, b0) with D1 as the addend, D2 = dot(a1, b1); the rest as the multiplication's sequence); NFLHIP_MULRELIN_MERGED,
 *   the default -- one launch of the kernel above in the scaled layout, then as the multiplication's merged plan;
 *   NFLHIP_MULRELIN_FUSED -- NFLHIP_ERR_UNSUPPORTED: the one-launch kernel re-forms a1 (.) b1 per digit from global memory.
 *   terms == 1 with every operand dense over the groups (group_stride 1, or groups == 1) IS nflhip_mulrelin_level_ntt_dev: the call
 *   forwards, every plan included.
 *   Scratch, tables, the level context, the first-call, larger-batch and while-capturing rules are the multiplication's, with
 *   `groups` as the batch (the terms size no scratch).
 *   NFLHIP_ERR_INVALID, nothing enqueued: what nflhip_mulrelin_level_ntt_dev refuses, terms == 0 or above 2^31, an extent that
 *   overflows, and an output that overlaps an operand's extent without beginning at that operand's first byte (every read is
 *   enqueued before the mod-down writes), the other output, or the key.
 *   The host variant stages a0, a1 dense [groups][terms], b0, b1 alike or [terms] with b_shared, and the key's digits that are read. */
int nflhip_tensor_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const nflhip_dot_operand *a0,
                              const nflhip_dot_operand *a1, const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, size_t groups,
                              size_t terms, size_t rows, int flags /* 0 */, void *stream);
int nflhip_tensor_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1,
                          const void *h_b0, const void *h_b1, size_t groups, size_t terms, int b_shared, size_t rows,
                          int flags);   /* staged host variant */
int nflhip_mulrelin_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                                const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, const void *d_key, size_t groups,
                                size_t terms, size_t k_special, size_t alpha, size_t level, int flags /* NFLHIP_MULRELIN_* */,
                                void *stream);
int nflhip_mulrelin_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0,
                            const void *h_b1, const void *h_key, size_t groups, size_t terms, int b_shared, size_t k_special,
                            size_t alpha, size_t level, int flags);   /* staged host variant */

/* ---- rotations and linear transforms at a level: one Galois key and one diagonal for every level ----
 * nflhip_rotate_hoisted_ntt_dev and nflhip_lintrans_ntt_dev on a ciphertext below the context's top level, with the ONE top-level
 * Galois key per rotation and the ONE top-level diagonal per term.  Levels, live rows A_l, phys(r) and the digits are those of
 * "leveled key switching" above.
 *   c0, c1, outputs  [batch][l][degree], NTT form, the dense layout over the first l moduli
 *   keys[m]          unchanged: [dnum_L][2][nmoduli][degree], the convention of "hoisted rotations" (from s to sigma_(k^-1)(s)).
 *                    Only keys[m][d][c][phys(r)] is read, for d < dnum_l and r < l + k_special
 *   weights[m]       (linear transform) unchanged: [nmoduli][degree], the diagonal in NTT form over the full context.  Rows A_l are
 *                    read in the pass on l + k_special rows and rows [0, l) in the passes on the kept rows; rows [l, L) are never
 *                    read.  Row j of an encoded diagonal is its residue mod p_j whatever the level, so one diagonal serves every level
 * Definition, word for word: with C_l and key_l as above and weight_l[m][r] = weights[m][phys(r)], a level-l call returns the words
 * of nflhip_rotate_hoisted_ntt_dev / nflhip_lintrans_ntt_dev on C_l with those keys and weights, k_special and min(alpha, l).  For
 * l = L it is that entry on this context itself.  ks, flags, plans, modes, the limits (16 rotations / terms), the NULL-key terms and
 * the overlap rules are those of the two entries with L read as l; the extent of a key that may not overlap an output is its first
 * dnum_l digits.  The level context is the one of the key switch at that (k_special, l); records, scratch and the first-call,
 * larger-batch and while-capturing rules are per level as there.  The kernels that read a key or a diagonal on l + k_special rows
 * (k_dot_multi, k_permute_mac_ntt) have instances that know the parent's pitch and the hole of L - l rows.
 * NFLHIP_ERR_INVALID, nothing enqueued: what the two entries refuse, and level == 0, level > L.
 * The host variants stage the operands, the 2 dnum_l key polynomials per rotation that are read and the whole diagonals. */
int nflhip_rotate_hoisted_level_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                        const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special,
                                        size_t alpha, size_t level, int flags, void *stream);
int nflhip_rotate_hoisted_level_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                                    const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special,
                                    size_t alpha, size_t level, int flags);   /* staged host variant */
int nflhip_lintrans_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1,
                                  const void *const *d_keys, const void *const *d_weights, const uint64_t *ks, size_t count, size_t batch,
                                  size_t k_special, size_t alpha, size_t level, int flags, void *stream);
int nflhip_lintrans_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1,
                              const void *const *h_keys, const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch,
                              size_t k_special, size_t alpha, size_t level, int flags);   /* staged host variant */

/* ---- weighted sums of automorphisms into several outputs --------------------------------------
 * nflhip_automorphism_mac_dev for `outputs` outputs that share the inputs and the multipliers -- the inner sums of the giant steps of
 * a BSGS matrix-vector product, which all read the same permuted baby-step sums:
 *     out_o[g][r][x] = addend_o[g][r][x] + sum_{t < terms} w_{o,t}[r][x] * in_t[g][r][src_{k_t}(x)]      mod p_r, canonical,
 * o < outputs <= NFLHIP_MAC_MULTI_MAX_OUTPUTS, terms <= NFLHIP_MAC_MAX_TERMS, g < batch, r < rows <= nmoduli.
 *   ins[t], ks[t]             shared by every output, as nflhip_automorphism_mac_dev takes them
 *   weights[o * terms + t]    [>= rows][degree], or NULL: the zero weight, for which nothing is read
 *   addends                   NULL, or addends[o] NULL or exactly outs[o]
 * All four arrays are HOST arrays; the pointers travel by value in the kernel arguments, nothing is allocated and the call can be
 * captured.  By definition the words are those of `outputs` calls of nflhip_automorphism_mac_dev (an output whose weights are all
 * NULL is its addend, or zero).  A term's source chunk is staged and read permuted ONCE for the outputs of a launch.  flags: 0.
 * NFLHIP_ERR_INVALID, nothing enqueued: what nflhip_automorphism_mac_dev refuses, outputs == 0 or > 16, an addend that is neither
 * NULL nor its output, ANY overlap of an output with an input, a weight or another output.  batch == 0 returns NFLHIP_OK.
 * The host variant stages every input, every weight, the addends and the outputs. */
#define NFLHIP_MAC_MULTI_MAX_OUTPUTS 16
int nflhip_automorphism_mac_multi_dev(nflhip_ctx *ctx, void *const *d_outs, const void *const *d_addends, const void *const *d_ins,
                                      const void *const *d_weights, const uint64_t *ks, size_t outputs, size_t terms, size_t batch,
                                      size_t rows, int flags, void *stream);
int nflhip_automorphism_mac_multi(nflhip_ctx *ctx, void *const *h_outs, const void *const *h_addends, const void *const *h_ins,
                                  const void *const *h_weights, const uint64_t *ks, size_t outputs, size_t terms, size_t batch,
                                  size_t rows, int flags);   /* staged host variant */

/* ---- BSGS slot linear transforms: giant steps before the one mod-down ---------------------------
 * sum_j sigma_{g_j}( sum_i pt_{j,i} (.) sigma_{b_i}(ct) ) for n1 baby steps b_i and n2 giant steps g_j in one call: a matrix-vector
 * product by n1 n2 diagonals with n1 + n2 Galois keys.  The babies' key-switch sums do not depend on the giant step, the giant step's
 * key switch acts on sums that are still on all rows, and ONE mod-down of two polynomials closes the call (double hoisting taken to
 * its end).  The context, K = k_special, alpha, the digit rule and the level rule are those of "hybrid key switching" and "leveled key
 * switching"; nm_l = level + K rows are live.
 *   level         l, 1 <= l <= L = nmoduli - K; l = L is the top level
 *   c0, c1, out0, out1   [batch][l][degree], NTT form; c0 may be NULL
 *   bkeys[i], bks[i]     i < n1 <= NFLHIP_BSGS_MAX_BABY: bks[i] odd; bkeys[i] the top-level Galois key [dnum_L][2][nmoduli][degree] by the
 *                 convention of the hoisted rotations (from s to sigma_(k^-1)(s), the permutation last), or NULL for the unrotated
 *                 baby step, which requires bks[i] = 1 mod 2 degree
 *   gkeys[j], gks[j]     j < n2 <= NFLHIP_BSGS_MAX_GIANT: likewise; NULL is the unrotated giant step
 *   weights[j n1 + i]    the top-level diagonal [nmoduli][degree] in NTT form, pre-rotated by sigma_{g_j}^-1 by the caller as every BSGS
 *                 does; NULL is the zero diagonal and nothing is read for it.  Every j has at least one non-NULL weight
 * Keys and weights are read as the level entries read them: rows phys(r) of the live rows and the first dnum_l digits only.
 * Definition, word for word ("mod-down": nflhip_moddown_ntt_dev(., K) on the level context, rounding or NFLHIP_BSGS_FLOOR; "mod-up" and
 * the key-switch sums: those of nflhip_keyswitch_ntt_dev, fast or NFLHIP_BSGS_CENTERED):
 *     U_d      the mod-up of c1, every digit                                               (nm_l rows)   once
 *     S_{i,c}  = sum_d U_d (.) bkeys[i][d][c]                        keyed i, c = 0, 1          (nm_l rows)
 *     per giant step j:
 *       V_{j,c} = sum_{keyed i} w_{j,i} (.) sigma^NTT_{b_i}(S_{i,c})                                (nm_l rows; zero with no keyed i)
 *       W_{j,0} = sum_{all i}   w_{j,i} (.) sigma^NTT_{b_i}(c0)            (absent when c0 is NULL)  (l rows)
 *       W_{j,1} = sum_{unkeyed i} w_{j,i} (.) c1                                                 (l rows)
 *       gkeys[j] non-NULL:
 *         v_j     = mod-down(V_{j,1}) + W_{j,1}                     (the mod-down skipped with no keyed i)   (l rows)
 *         T_{j,c} = sum_d mod-up(v_j)_d (.) gkeys[j][d][c]                                       (nm_l rows)
 *         A_0 += sigma^NTT_{g_j}(V_{j,0} + T_{j,0});   A_1 += sigma^NTT_{g_j}(T_{j,1});   O_0 += sigma^NTT_{g_j}(W_{j,0})
 *       gkeys[j] NULL:
 *         A_c += V_{j,c};   O_0 += W_{j,0};   O_1 += W_{j,1}
 *     out_c = mod-down(A_c) + O_c                                   canonical, row by row mod p_r
 * Every sum is exact mod p_r, so the order of the additions does not matter and both plans give the same words.
 * It is a BSGS product: out0 + out1 s = sum_j sigma_{g_j}(sum_i pt_{j,i} sigma_{b_i}(c0 + c1 s)) + e with |e| at most
 * n2 kb n T B + kg B + (kg + 1)(n + 1), B the bound of one key switch, kb / kg the keyed babies / giants, T = |pt|_inf
 * (tests/test_bsgs_cpu.py).
 * Plans, same words; `flags` may carry at most one plan flag:
 *   NFLHIP_BSGS_SEQUENCE  the map through existing entries only: nflhip_baseconv_ntt_dev per digit, nflhip_dot_dev,
 *                         nflhip_automorphism_dev, nflhip_automorphism_mac_dev, the element-wise addition (nflhip_pointwise_dev),
 *                         nflhip_moddown_ntt_dev; out_c is a device copy of the sum.  No kernel of its own: the cross-check.
 *                         NFLHIP_ERR_UNSUPPORTED, nothing enqueued, where batch polynomials are no whole number of 16-byte groups
 *                         (rows under 16 bytes), which the element-wise addition does not serve.
 *   NFLHIP_BSGS_HOISTED   the mod-up of c1 once; ONE k_dot_multi launch for every S; the giant steps in groups of 4: the several-output
 *                         weighted-sum kernel for the group's V (both components in one grid), ONE mod-down over the group's V_{.,1},
 *                         W_{.,1} added on l rows, ONE mod-up over group * batch polynomials, the inner products with V_{j,0} as the
 *                         addend of T_{j,0}, one weightless permute-and-accumulate into A_c; after the last group one mod-down of A
 *                         into out0 / out1 and the passes on l rows.  Whatever has no term is skipped.
 *   none                  hoisted.
 * Scratch, context-owned (per level), in polynomials of nm_l rows (p) and of l rows (q), G = min(4, giants of one kind): hoisted
 *     batch (1 p | 1 q) + batch dnum p [U] + 2 kb batch p [S] + 2 batch p [A] + 2 G batch p [V, T] + G batch q [v]
 *     + G batch (1 p | 1 q) + G batch dnum p [the giants' mod-up] + n2 batch q [W_{.,0}];
 * the sequence batch (2 dnum + 2 kb + 9) p + 7 batch q at most.  G = 4 bounds the giants' share of the scratch at four
 * ciphertexts' worth of digits whatever n2 is, and is a whole number of the several-output kernel's launches.
 * The first call for a (k_special, alpha, level, plan, modes) and kinds of steps (keyed babies or none, keyed giants or none, c0 or
 * none), or for a larger batch, more keyed babies or more giants, builds tables and allocates (it synchronises): make
 * it before capturing into a hipGraph; while capturing it is NFLHIP_ERR_UNSUPPORTED, nothing is enqueued and the stream stays usable.
 * Calls on different streams are ordered on the scratch by an event.
 * NFLHIP_ERR_INVALID, nothing enqueued: a NULL context, a NULL pointer with batch != 0 (except c0, a key with k = 1 mod 2 degree and a
 * weight), n1 or n2 of 0 or above 16, an even k, a NULL key with another k, a giant step without a weight, k_special, alpha or level out
 * of range, unknown flag bits or two plan flags, a size that overflows, out0 overlapping out1, an output overlapping c0, c1, the live
 * digits of a key or a weight, a cyclic row context, a repeated modulus inside a digit or among the special rows.
 * batch == 0 returns NFLHIP_OK and touches nothing.  The host variant stages c0, c1, the live digits of every key, every weight and
 * both outputs. */
#define NFLHIP_BSGS_MAX_BABY 16
#define NFLHIP_BSGS_MAX_GIANT 16
#define NFLHIP_BSGS_CENTERED 0x100
#define NFLHIP_BSGS_FLOOR 0x200
#define NFLHIP_BSGS_SEQUENCE 0x1000
#define NFLHIP_BSGS_HOISTED 0x2000
int nflhip_bsgs_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_bkeys,
                        const uint64_t *bks, size_t n1, const void *const *d_gkeys, const uint64_t *gks, size_t n2,
                        const void *const *d_weights, size_t batch, size_t k_special, size_t alpha, size_t level, int flags,
                        void *stream);
int nflhip_bsgs_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_bkeys,
                    const uint64_t *bks, size_t n1, const void *const *h_gkeys, const uint64_t *gks, size_t n2,
                    const void *const *h_weights, size_t batch, size_t k_special, size_t alpha, size_t level,
                    int flags);   /* staged host variant */

/* ---- element-wise ops: poly::operator=(expr) core.hpp:24-37 ------------------
 * op in NFLHIP_OP_*; b is ignored for COMPUTE_SHOUP, bprime only used by
 * MUL_SHOUP.  Input contract as the reference's (operands < p; ops.hpp:131,148,211). */
int nflhip_pointwise_dev(nflhip_ctx *ctx, int op, void *d_out, const void *d_a, const void *d_b,
                         const void *d_bprime, size_t batch, void *stream);
int nflhip_pointwise(nflhip_ctx *ctx, int op, void *h_out, const void *h_a, const void *h_b,
                     const void *h_bprime, size_t batch);

/* ---- fused expression trees -------------------------------------------------------
 * poly::operator=(expr) evaluates a whole expression tree (e.g. `a + b*add`, tests/poly_p.cpp:62-66;
 * `resb - resa*s`, tests/nfllib_demo_main_op.cpp:51) in one pass without temporaries
 * (core.hpp:24-37, ops.hpp:52-79).  Here the tree is a postfix program executed per word on the
 * device: byte k < 8 pushes operand k; NFLHIP_EXPR_ADD/SUB/MUL pop two values and push the result
 * (`x op y` with y on top); NFLHIP_EXPR_MUL_SHOUP pops b', b, a and pushes mulmod_shoup(a,b,b');
 * NFLHIP_EXPR_COMPUTE_SHOUP replaces the top.  At most 8 operands, 24 program bytes, stack depth 4;
 * exactly one value must remain.  `out` may alias any operand.  The host-pointer variant stages at
 * most 4 distinct operands (4: `c = c + shoup(a * b, b')`, the result is formed over the first one's staging buffer). */
#define NFLHIP_EXPR_ADD 0x10
#define NFLHIP_EXPR_SUB 0x11
#define NFLHIP_EXPR_MUL 0x12
#define NFLHIP_EXPR_MUL_SHOUP 0x13
#define NFLHIP_EXPR_COMPUTE_SHOUP 0x14
#define NFLHIP_EXPR_MAX_OPERANDS 8
#define NFLHIP_EXPR_MAX_LEN 24
int nflhip_eval_dev(nflhip_ctx *ctx, void *d_out, const void *const *d_operands, size_t noperands,
                    const unsigned char *program, size_t proglen, size_t batch, void *stream);
int nflhip_eval(nflhip_ctx *ctx, void *h_out, const void *const *h_operands, size_t noperands,
                const unsigned char *program, size_t proglen, size_t batch);
/* The same over operands that advance by their own stride (in polynomials) from one batch element to the next:
 * 1 = a dense array of polynomials, 0 = ONE polynomial shared by the whole batch (a key), k = every k-th polynomial of
 * an interleaved array.  Element i reads operand j at d_operands[j] + i*strides[j] polynomials and writes
 * d_out + i*out_stride polynomials (out_stride >= 1).  What the header's deferred per-polynomial operations are
 * coalesced into (one launch for a loop of `r[i] = u[i] * key + e[i]`). */
int nflhip_eval_strided_dev(nflhip_ctx *ctx, void *d_out, size_t out_stride, const void *const *d_operands,
                            const size_t *strides, size_t noperands, const unsigned char *program, size_t proglen,
                            size_t batch, void *stream);

/* ---- the metric path ---------------------------------------------------------
 * c = INTT( NTT(a) (.) NTT(b) ): the reference sequence
 *   a.ntt_pow_phi(); b.ntt_pow_phi(); c = a*b; c.invntt_pow_invphi();
 * (poly.hpp:167-168, 350) as one fused device pass.  a, b, c in coefficient
 * form; a and b are not modified; c may alias a or b.
 * Rows of up to 16384 words are ONE launch that touches nothing but its operands: calls on distinct streams run
 * concurrently.  Longer rows (32768 words: b' = NTT(b) into a scratch, then the product kernel; 65536 and beyond: streaming
 * passes around block products) go through ONE context-owned scratch area: calls on different streams of one context are
 * ordered one after the other by events (no host synchronisation); use one context per stream to overlap them. */
int nflhip_polymul_dev(nflhip_ctx *ctx, void *d_c, const void *d_a, const void *d_b, size_t batch,
                       void *stream);
int nflhip_polymul(nflhip_ctx *ctx, void *h_c, const void *h_a, const void *h_b, size_t batch);
/* "one operand pre-transformed": c = INTT( NTT(a) (.) b_ntt ), b_ntt already in
 * NTT form (keys kept in NTT form as in tests/nfllib_demo_main_op.cpp:26-46). */
int nflhip_polymul_ntt_dev(nflhip_ctx *ctx, void *d_c, const void *d_a, const void *d_bntt, size_t batch,
                           void *stream);

/* ---- transform-fused pipelines ------------------------------------------------------
 * What the reference's callers run AROUND the transforms, as one device pass per batch.  The reference's only
 * end-to-end ring code is the LWE demo (tests/nfllib_demo_main_op.cpp:26-58):
 *   encrypt():  u.ntt_pow_phi(); e1.ntt_pow_phi(); e2.ntt_pow_phi(); resa = u * pka + e1; resb = u * pkb + e2;
 *   decrypt():  tmp = resb - resa * s; tmp.invntt_pow_invphi();
 * (poly.hpp:167-168 + the evaluation loop core.hpp:24-37).  Run operator by operator that is 8 + 2 launches and ~17 + 5
 * polynomial passes over HBM; here the transformed operands never leave the registers of the workgroup that owns the row:
 *   nflhip_fwd_fma_dev    out  = NTT(x) * k + NTT(e)
 *   nflhip_fwd_fma2_dev   out0 = NTT(x) * k0 + NTT(e0),  out1 = NTT(x) * k1 + NTT(e1)       (x is transformed once)
 *   nflhip_fma_inv_dev    out  = INTT(b + a * k)   or   INTT(b - a * k)  (subtract != 0)
 * Results are bit-identical to the operator-by-operator sequence.  Every operand names its own stride (in polynomials
 * from one batch element to the next: 1 = dense array, 0 = ONE polynomial for the whole batch -- a key) and, for the
 * inputs of the forward entries, its format: NFLHIP_FMT_WORDS = residue words [nmoduli][degree] in coefficient form, or
 * one SIGNED integer per coefficient shared by all moduli (int8 / int16 / int32; v < 0 stands for p + v; |v| must be
 * below every modulus) -- what the samplers produce before they spread a value over the moduli (core.hpp:230-277); see
 * nflhip_sample_gauss_small_dev.  k operands and the operands of nflhip_fma_inv_dev are words in NTT form (canonical,
 * ops.hpp:131,211).  Results are dense; a result may alias a DENSE (stride 1) input of the same call
 * exactly (same first byte), or lie over one in any way when it is out0 over e1 / k1 (then a plan that reads every input before it
 * stores is taken); a result that overlaps an operand shared by the batch (stride 0, batch > 1) is refused with NFLHIP_ERR_INVALID.  u64 limbs at degree 4096,
 * 8192 and 16384 run one generated gfx950 kernel per call (at degree 32768 nflhip_fma_inv_dev does for dense a / b, and the forward
 * entries run three for int8 polynomials with keys of stride 0); rows of 1024 / 2048 words -- 4096 for 32-bit limbs -- run every
 * entry as ONE pass of the wave-per-row kernels (forward: inputs of one format, strides 0 / 1); every other shape composes the same
 * result from the plain kernels through the context's scratch (calls on different streams of one context are then ordered by
 * events, as for nflhip_polymul_dev). */
#define NFLHIP_FMT_WORDS 0
#define NFLHIP_FMT_I8 1
#define NFLHIP_FMT_I16 2
#define NFLHIP_FMT_I32 3
typedef struct nflhip_operand {
  const void *ptr; /* device pointer */
  size_t stride;   /* polynomials (of the operand's own format) between consecutive batch elements */
  int format;      /* NFLHIP_FMT_* */
} nflhip_operand;
int nflhip_fwd_fma_dev(nflhip_ctx *ctx, void *d_out, const nflhip_operand *x, const nflhip_operand *k,
                       const nflhip_operand *e, size_t batch, void *stream);
int nflhip_fwd_fma2_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const nflhip_operand *x, const nflhip_operand *k0,
                        const nflhip_operand *e0, const nflhip_operand *k1, const nflhip_operand *e1, size_t batch,
                        void *stream);
int nflhip_fma_inv_dev(nflhip_ctx *ctx, void *d_out, const nflhip_operand *a, const nflhip_operand *k,
                       const nflhip_operand *b, int subtract, size_t batch, void *stream);
/* 1 when the three entries above run as one-pass kernels on this context (the default kernel variant; u64 limbs: ONE kernel each
 * at degree 1024 / 2048 -- the wave-per-row kernels -- and 4096 / 8192 / 16384 -- generated; at degree 32768 one kernel for
 * nflhip_fma_inv_dev and, for int8 polynomials with keys shared by the batch, one per noise polynomial + one for the results;
 * u32 limbs: ONE kernel each at degree 1024 / 2048 / 4096), 0 when they compose the result from the plain kernels: what a caller
 * that can choose between its own operator sequence and these entries asks (the header's deferred queue only rewrites sequences
 * when it gains a pass) */
int nflhip_has_fused_kernels(const nflhip_ctx *ctx);
/* compact polynomial(s) -> residue words: d_data[b][cm][i] = v < 0 ? p_cm + v : v, v = element i of src's polynomial
 * b * stride (format NFLHIP_FMT_WORDS: a strided gather of word rows) */
int nflhip_expand_small_dev(nflhip_ctx *ctx, void *d_data, const nflhip_operand *src, size_t batch, void *stream);

/* ---- comparisons: expr::operator bool over eqmod / neqmod (ops.hpp:81-117) ----
 * *result = 1 iff ANY word of a equals (any_eq) / differs from (any_neq) the
 * matching word of b -- the reference's semantics for `a == b` / `a != b`.
 * These synchronise the stream. */
int nflhip_any_eq_dev(nflhip_ctx *ctx, const void *d_a, const void *d_b, size_t batch, int *result,
                      void *stream);
int nflhip_any_neq_dev(nflhip_ctx *ctx, const void *d_a, const void *d_b, size_t batch, int *result,
                       void *stream);
int nflhip_any_eq(nflhip_ctx *ctx, const void *h_a, const void *h_b, size_t batch, int *result);
int nflhip_any_neq(nflhip_ctx *ctx, const void *h_a, const void *h_b, size_t batch, int *result);

/* ---- range assertion: CHECK_STRICTMOD ---------------------------------------------
 * The reference's tests are compiled with CHECK_STRICTMOD (tests/CMakeLists.txt:10): ASSERT_STRICTMOD (debug.hpp:33-37)
 * then asserts that every operand word is the canonical representative, x < p -- at the entry of the transforms
 * (core.hpp:457-462), in addmod / submod / mulmod / mulmod_shoup (ops.hpp:131,148,190,211,235) and after the samplers
 * (core.hpp:179-185, 275-281, 319-325).  *bad = 1 iff some word of the batch is >= its row's modulus.  The _dev form is one
 * streaming compare on the device and synchronises the stream; the host form reads host words against the context's
 * copy of the moduli (no device needed).  include/nfl_hip/nfl.hpp calls them under -DCHECK_STRICTMOD (without NDEBUG) on
 * the operands of transforms and expressions and throws std::runtime_error where the reference's assert would fire. */
int nflhip_check_range_dev(nflhip_ctx *ctx, const void *d_data, size_t batch, int *bad, void *stream);
int nflhip_check_range(const nflhip_ctx *ctx, const void *h_data, size_t batch, int *bad);

/* ---- CRT ---------------------------------------------------------------------
 * lift:    GMP::poly2mpz gmp.hpp:183-209 -- limbs[b][i][0..L) = little-endian
 *          64-bit limbs (the mpz_export(order=-1) image) of
 *          X_i = sum_cm lifting[cm]*x(cm,i) mod Q, in [0,Q).
 * project: GMP::mpz2poly gmp.hpp:211-219 / poly::set_mpz gmp.hpp:73-108 --
 *          x(cm,i) = X_i mod p_cm for non-negative X_i given as L_in limbs.
 * Any number of moduli.  With 62-bit moduli the lift runs on the matrix cores (an int8 GEMM over balanced base-256 digits,
 * nfllib_amd/csrc/kernels_crt_mfma.hip) for 21..32 of them, the projection for 17..32 and inputs of 5..64 limbs, when
 * batch * degree is a multiple of 64; register-resident VALU kernels up to 32 moduli otherwise, a limb-serial kernel
 * beyond.  The results do not depend on which kernel ran. */
int nflhip_crt_lift_dev(nflhip_ctx *ctx, uint64_t *d_limbs, const void *d_data, size_t batch, void *stream);
int nflhip_crt_project_dev(nflhip_ctx *ctx, void *d_data, const uint64_t *d_limbs, size_t L_in, size_t batch,
                           void *stream);
int nflhip_crt_lift(nflhip_ctx *ctx, uint64_t *h_limbs, const void *h_data, size_t batch);
int nflhip_crt_project(nflhip_ctx *ctx, void *h_data, const uint64_t *h_limbs, size_t L_in, size_t batch);

/* ---- harness helpers ---------------------------------------------------------
 * Seeded synthetic operands generated in place on the device: word (b,cm,i) of
 * operand s = splitmix64 counter stream masked to floor(log2 p)+1 bits with one
 * conditional subtract of p -- the distribution rule of nfl::uniform
 * (core.hpp:165-176).  first_poly offsets the counter so shards of one logical
 * batch can be generated independently on several GPUs. */
int nflhip_fill_uniform_dev(nflhip_ctx *ctx, void *d_data, size_t first_poly, size_t batch, uint64_t seed,
                            int operand, void *stream);

/* ---- samplers ------------------------------------------------------------------
 * Device versions of the reference's random constructors (core.hpp:146-391):
 *   poly(uniform) / poly(non_uniform(ub[,amp])) / poly(ZO_dist(rho)) / poly(hwt_dist(h)) /
 *   poly(gaussian(&fg_prng[,amp])).
 * The reference draws from a process-global Salsa20 stream keyed from /dev/urandom
 * (lib/prng/fastrandombytes.cpp:17-37); here every call names its stream: a 32-byte key
 * and a 64-bit stream id select a ChaCha20 keystream that is read by position (word w of
 * the stream belongs to one fixed coefficient), so a call is reproducible and a batch can
 * be generated in shards (first_poly) with the same result.  Callers that want the
 * reference's behaviour draw the key from the OS once and increment stream_id per call
 * (what include/nfl_hip/nfl.hpp does).  The map from random words to coefficients is the
 * reference's (mask-and-subtract, no rejection), so the distributions are identical. */
enum {
  NFLHIP_DIST_UNIFORM = 0, /* core.hpp:152-188   one word per residue word */
  NFLHIP_DIST_BOUNDED = 1, /* core.hpp:195-277   param0 = upper_bound, param1 = amplifier; one word per coefficient */
  NFLHIP_DIST_ZO = 2,      /* core.hpp:330-340   param0 = rho (0..255) */
  NFLHIP_DIST_HWT = 3,     /* core.hpp:347-391   param0 = hamming weight (1..degree) */
  /* OR into NFLHIP_DIST_ZO / NFLHIP_DIST_HWT: store +1 exactly as the reference does, as the non-canonical word
   * p + 1 (`pm + (rnd & 2)`, core.hpp:341,387), so that raw _data images diff clean against the CPU library.
   * Default (flag absent): the canonical 1, which the engine's own operators require (ops.hpp:131,148). */
  NFLHIP_DIST_REFERENCE_WORDS = 0x100,
  /* OR into NFLHIP_DIST_UNIFORM: the NARROW draw -- residue word g reads the limb-width LANE g of the keystream (bytes
   * [g w, (g + 1) w), little endian, w = limb bytes) instead of one 64-bit word, in a keystream domain of its own.  Same map
   * from the lane to the residue (mask, one conditional subtraction), so the distribution is the reference's -- and so is the
   * consumption: the reference fills _data with fastrandombytes and reduces every limb-width word in place (core.hpp:152-188),
   * i.e. residue word g is made from bytes [g w, (g + 1) w) of ITS stream (tests/test_samplers_cpu.py pins exactly that); a u16 / u32
   * polynomial costs a quarter / half of the ChaCha20 rounds (measured: profiles/r05_sampler_rates.txt).  The values differ
   * from the wide rule's for the same (key, stream_id) -- a different domain, by design: what the wide rule produces, and
   * every digest recorded from it, keeps its meaning. */
  NFLHIP_DIST_NARROW = 0x200
};
/* KEYSTREAM DISCIPLINE.  A (key, stream_id, distribution) triple names one keystream: two calls that share all
 * three produce the same values.  Different distributions never share keystream words even for the same
 * (key, stream_id) -- the distribution's tag is part of the ChaCha20 block counter -- so a public uniform polynomial
 * never reveals the noise drawn next to it; but two draws of the SAME distribution that must be independent (the
 * secret and the error of an LWE sample) need distinct stream ids.  Callers that want the reference's behaviour draw
 * the key from the OS once and take a fresh stream id per call (what include/nfl_hip/nfl.hpp does). */
int nflhip_sample_dev(nflhip_ctx *ctx, void *d_data, size_t first_poly, size_t batch, int dist, uint64_t param0,
                      uint64_t param1, const unsigned char key[32], uint64_t stream_id, void *stream);
int nflhip_sample(nflhip_ctx *ctx, void *h_data, size_t batch, int dist, uint64_t param0, uint64_t param1,
                  const unsigned char key[32], uint64_t stream_id);
/* SEQUENCE forms: polynomial b of the dense batch at d is exactly what the one-polynomial call
 * nflhip_sample_dev(ctx, d_b, 0, 1, dist, param0, param1, key, first_stream_id + b*stream_id_stride, stream) produces
 * (one keystream per polynomial instead of one keystream per batch) -- so a loop of per-polynomial constructor calls
 * and ONE batched launch give the same polynomials.  Needs degree >= 8 (NFLHIP_ERR_UNSUPPORTED otherwise). */
int nflhip_sample_seq_dev(nflhip_ctx *ctx, void *d_data, size_t batch, int dist, uint64_t param0, uint64_t param1,
                          const unsigned char key[32], uint64_t first_stream_id, uint64_t stream_id_stride, void *stream);
/* raw keystream words [first_word, first_word + nwords) of (key, stream_id) -- what the samplers consume */
int nflhip_random_words_dev(nflhip_ctx *ctx, uint64_t *d_out, uint64_t first_word, size_t nwords,
                            const unsigned char key[32], uint64_t stream_id, void *stream);

/* Discrete Gaussian (FastGaussianNoise<in,out,lu>(sigma, security, samples, center),
 * FastGaussianNoise.hpp:163-290): cumulative table with the reference's tail bound and bit precision
 * (<= 384 bits: security parameters up to ~ 360), sampled by inversion.  The table lives on the context's device.
 * Keystream use: the top 64 bits of coefficient g's uniform number are word g of stream (key, stream_id)
 * (g = (first_poly + poly) * degree + i); its lower words -- words (W-1)*g .. of the same stream counted from
 * block 2^63 -- are only generated when the top word ties with a table entry; the sample is exactly the
 * full-precision inversion x = x_min + #{k : table[k] <= r}. */
typedef struct nflhip_gauss nflhip_gauss;
int nflhip_gauss_create(nflhip_ctx *ctx, nflhip_gauss **out, double sigma, unsigned security, unsigned samples,
                        double center);
int nflhip_gauss_destroy(nflhip_ctx *ctx, nflhip_gauss *g);
/* DRAW WIDTH of every sampler that takes this table: 64 (default, the rule above) or 32 -- the narrow draw: the top 32 bits
 * of coefficient g's uniform number are the 32-bit lane g of the stream (key, stream_id) in the Gaussian samplers' narrow
 * domain, the next 32 bits lane g of a second domain that is only generated when the first lane ties with the top half of
 * a table entry the search meets (~entries x 2^-32 per sample), the lower words as above.  The sample is still EXACTLY the
 * full-precision inversion of that number; it costs half the ChaCha20 rounds and 32-bit compares.  Values differ from the
 * 64-bit draw's for the same (key, stream_id): other keystream domains.  Sequence forms then need degree >= 16.  Set it
 * before the table is used by concurrent calls (it is a plain field). */
int nflhip_gauss_set_draw_bits(nflhip_gauss *g, int bits);
int nflhip_gauss_draw_bits(const nflhip_gauss *g);
/* the same table without a device (host arithmetic only: what nflhip_gauss_create uploads); h_table may be NULL to
 * query the sizes first, cap_words = capacity of h_table in 64-bit words */
int nflhip_gauss_table(double sigma, unsigned security, unsigned samples, double center, long long *x_min, size_t *entries,
                       int *words, unsigned *bit_precision, double *tail, uint64_t *h_table, size_t cap_words);
/* introspection: support [x_min, x_min + entries), words per entry, the reference's bit_precision and tail bound;
 * h_table (may be NULL) receives entries*words 64-bit words, most significant word of an entry first */
int nflhip_gauss_info(const nflhip_gauss *g, long long *x_min, size_t *entries, int *words, unsigned *bit_precision,
                      double *tail, uint64_t *h_table);
int nflhip_sample_gauss_dev(nflhip_ctx *ctx, void *d_data, size_t first_poly, size_t batch, const nflhip_gauss *g,
                            uint64_t amplifier, const unsigned char key[32], uint64_t stream_id, void *stream);
int nflhip_sample_gauss(nflhip_ctx *ctx, void *h_data, size_t batch, const nflhip_gauss *g, uint64_t amplifier,
                        const unsigned char key[32], uint64_t stream_id);
/* sequence form, see nflhip_sample_seq_dev */
int nflhip_sample_gauss_seq_dev(nflhip_ctx *ctx, void *d_data, size_t batch, const nflhip_gauss *g, uint64_t amplifier,
                                const unsigned char key[32], uint64_t first_stream_id, uint64_t stream_id_stride,
                                void *stream);
/* COMPACT forms (format NFLHIP_FMT_I8 / I16 / I32): d_out[b][i] = x * amplifier as ONE signed integer per coefficient,
 * x exactly the sample nflhip_sample_gauss_dev / nflhip_sample_gauss_seq_dev would spread over the moduli for the same
 * arguments -- so nflhip_expand_small_dev (or the forward entries above, which expand in their prologue) reproduce those
 * calls' words bit for bit at 1/32 (int8, 4 moduli of 64 bits) of the bytes.  NFLHIP_ERR_INVALID when a possible sample
 * does not fit the format or is not below every modulus. */
int nflhip_sample_gauss_small_dev(nflhip_ctx *ctx, void *d_out, int format, size_t first_poly, size_t batch,
                                  const nflhip_gauss *g, uint64_t amplifier, const unsigned char key[32], uint64_t stream_id,
                                  void *stream);
int nflhip_sample_gauss_small_seq_dev(nflhip_ctx *ctx, void *d_out, int format, size_t batch, const nflhip_gauss *g,
                                      uint64_t amplifier, const unsigned char key[32], uint64_t first_stream_id,
                                      uint64_t stream_id_stride, void *stream);
/* `count` (1..4) compact draws from ONE table in ONE launch: draw j writes `batch` polynomials to d_out[j] with amplifier[j] and is,
 * byte for byte, nflhip_sample_gauss_small_seq_dev(..., stream_id[j], stream_id_stride[j], ...) when stream_id_stride is given and
 * nflhip_sample_gauss_small_dev(..., first_poly 0, ..., stream_id[j], ...) when it is NULL.  What an LWE encryption draws per
 * ciphertext (FastGaussianNoise.hpp:477-595 through tests/nfllib_demo_main_op.cpp:33-35: x, e0, e1 with their own amplifiers):
 * three launches of a few hundred polynomials each leave wave slots empty in their last round and pay three ramps. */
int nflhip_sample_gauss_small_multi_dev(nflhip_ctx *ctx, void *const *d_out, size_t count, int format, size_t batch,
                                        const nflhip_gauss *g, const uint64_t *amplifier, const unsigned char key[32],
                                        const uint64_t *stream_id, const uint64_t *stream_id_stride, void *stream);
/* FastGaussianNoise::getNoise(out, rlen) (FastGaussianNoise.hpp:477-595): `count` raw signed samples; sample j is the
 * integer that coefficient first_sample + j of a polynomial batch gets from the same (key, stream_id) */
int nflhip_gauss_noise_dev(nflhip_ctx *ctx, int64_t *d_out, uint64_t first_sample, size_t count, const nflhip_gauss *g,
                           const unsigned char key[32], uint64_t stream_id, void *stream);
int nflhip_gauss_noise(nflhip_ctx *ctx, int64_t *h_out, size_t count, const nflhip_gauss *g,
                       const unsigned char key[32], uint64_t stream_id);

/* nfl::fastrandombytes(r, rlen) (nfl/prng/fastrandombytes.h:12): rlen raw keystream bytes of (key, stream_id) -- the
 * bytes of nflhip_random_words_dev's words 0.. in little-endian order -- generated on `device`, copied to the host */
int nflhip_random_bytes(int device, unsigned char *h_out, size_t nbytes, const unsigned char key[32], uint64_t stream_id);

/* plain device-memory helpers so a C caller needs no HIP headers */
int nflhip_malloc(nflhip_ctx *ctx, void **d_ptr, size_t bytes);
int nflhip_free(nflhip_ctx *ctx, void *d_ptr);
int nflhip_memcpy_h2d(nflhip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, void *stream);
int nflhip_memcpy_d2h(nflhip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, void *stream);
int nflhip_memcpy_d2d(nflhip_ctx *ctx, void *d_dst, const void *d_src, size_t bytes, void *stream);
int nflhip_memset_dev(nflhip_ctx *ctx, void *d_dst, int byte, size_t bytes, void *stream);
int nflhip_stream_sync(nflhip_ctx *ctx, void *stream);
/* never blocks: *idle = 1 when everything enqueued on `stream` so far has completed, else 0 (hipStreamQuery).  What the
 * header's deferred queue asks before it starts a run early (a short loop's records would otherwise wait for the loop's
 * end with the device idle).  Not for a stream that is being captured into a hipGraph (a query ends the capture). */
int nflhip_stream_idle(nflhip_ctx *ctx, void *stream, int *idle);
/* a non-blocking stream of the context's device (what the header's resident handles enqueue on) */
int nflhip_stream_create(nflhip_ctx *ctx, void **stream);
int nflhip_stream_destroy(nflhip_ctx *ctx, void *stream);
/* d_dst[k] = *d_one for k < count: one polynomial replicated over a resident batch (one kernel, no host copies) */
int nflhip_broadcast_dev(nflhip_ctx *ctx, void *d_dst, const void *d_one, size_t count, void *stream);

/* ---- multi-GPU: the batch split --------------------------------------------------------
 * The reference has no distributed layer; its callers hold dense arrays of independent polynomials
 * (tests/tools.h:6-17: alloc_aligned<poly_t, 32>(N)) and loop over them (tests/nfl_mul_main.cpp, nfllib_demo_main_op.cpp).
 * Across the GPUs of one node that array is cut into contiguous shards: device r of n owns polynomials
 * [first, first + count) of `total` as nflhip_shard_range says, every device builds identical tables locally (one
 * context per device: nflhip_ctx_create's `device` argument) and there is NO data-path collective: operands are generated
 * in place (the `first_poly` argument of nflhip_fill_uniform_dev / nflhip_sample*_dev) or scattered once.  Two ways to
 * drive it:
 *   ONE PROCESS, n devices  -- n contexts, one stream each; nflhip_scatter_local_dev / nflhip_gather_local_dev move
 *                              shards with peer-to-peer copies (hipMemcpyPeerAsync), one per peer, each on that peer's
 *                              stream so that every xGMI link is busy at once;
 *   ONE PROCESS PER DEVICE  -- an nflhip_comm on RCCL: nflhip_scatter_dev / nflhip_gather_dev are grouped
 *                              ncclSend / ncclRecv of contiguous shards (one message per peer and group, <= 1 GiB each).
 * RCCL is bound at run time (librccl.so.1 is opened by the first nflhip_comm_* call), so single-GPU callers do not
 * depend on it. */
int nflhip_ctx_device(const nflhip_ctx *ctx);
/* contiguous, balanced split: the first (total mod nranks) ranks own one polynomial more */
int nflhip_shard_range(size_t total, int nranks, int rank, size_t *first, size_t *count);
/* 64-bit digest of `batch` resident polynomials that COMPOSES over shards: sum over words of
 * (g + 1) * mix(word) mod 2^64, g = the word's index in the whole logical batch (first_poly offsets it), so the sum of
 * the shards' digests equals the digest of the whole batch ("checksum of checksums").  Synchronises `stream`. */
int nflhip_digest_dev(nflhip_ctx *ctx, const void *d_data, size_t first_poly, size_t batch, uint64_t *h_digest,
                      void *stream);
/* copy between the devices of two contexts of this process, asynchronous on `stream` (a stream of dst_ctx's device) */
int nflhip_memcpy_peer_dev(nflhip_ctx *dst_ctx, void *d_dst, nflhip_ctx *src_ctx, const void *d_src, size_t bytes,
                           void *stream);
/* ONE PROCESS: ctxs[r] / d_shards[r] / streams[r] belong to device r of n (same shape everywhere); d_full holds `total`
 * polynomials on ctxs[root]'s device.  scatter: shard r <- full[first_r, first_r + count_r); gather: the inverse.
 * Each peer's copy runs on that peer's stream after everything enqueued so far on the root's stream (scatter) / on the
 * peer's stream (gather), and the root's stream waits for all of them: no host synchronisation. */
int nflhip_scatter_local_dev(nflhip_ctx *const *ctxs, int n, void *const *d_shards, int root, const void *d_full,
                             size_t total, void *const *streams);
int nflhip_gather_local_dev(nflhip_ctx *const *ctxs, int n, void *d_full, int root, const void *const *d_shards,
                            size_t total, void *const *streams);
/* ONE PROCESS PER DEVICE: a communicator over RCCL (ncclCommInitRank).  Rank 0 draws the id (ncclGetUniqueId) and hands
 * it to the other ranks out of band (a file, MPI, a key-value store ...).  nranks = 1 is legal (and what a
 * single-GPU box can run). */
typedef struct nflhip_comm nflhip_comm;
#define NFLHIP_COMM_ID_BYTES 128
int nflhip_comm_unique_id(unsigned char id[NFLHIP_COMM_ID_BYTES]);
int nflhip_comm_create(nflhip_comm **out, nflhip_ctx *ctx, int nranks, int rank, const unsigned char id[NFLHIP_COMM_ID_BYTES]);
int nflhip_comm_destroy(nflhip_comm *comm);
int nflhip_comm_rank(const nflhip_comm *comm);
int nflhip_comm_size(const nflhip_comm *comm);
/* scatter: rank `root` holds d_full (`total` polynomials, ignored elsewhere); every rank receives its shard_range slice
 * in d_shard.  gather: the inverse.  Asynchronous on `stream`; every rank must call with the same total and root. */
int nflhip_scatter_dev(nflhip_comm *comm, void *d_shard, const void *d_full, size_t total, int root, void *stream);
int nflhip_gather_dev(nflhip_comm *comm, void *d_full, const void *d_shard, size_t total, int root, void *stream);
/* control plane: a barrier (one-word all-reduce) and an all-gather of one 64-bit word per rank (shard digests, clocks).
 * Both synchronise `stream`. */
int nflhip_comm_barrier(nflhip_comm *comm, void *stream);
int nflhip_comm_allgather_u64(nflhip_comm *comm, uint64_t mine, uint64_t *h_all, void *stream);

/* ---- in-library timing of the metric kernel (HIP events on `stream`) -----------
 * Runs `iters` back-to-back polymul passes over the batch and returns the mean
 * milliseconds per pass measured with hipEvents recorded on the same stream the
 * kernels are launched on (bench.py's roofline leg). */
int nflhip_time_polymul_dev(nflhip_ctx *ctx, void *d_c, const void *d_a, const void *d_b, size_t batch,
                            int iters, void *stream, float *ms_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* NFLHIP_H */
