/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_tensor_dot_ntt_dev / nflhip_tensor_dot_ntt / nflhip_mulrelin_dot_ntt_dev /
 * nflhip_mulrelin_dot_ntt over plain host memory, linked INTO the program tests/cpp_mulrelin_dot/mulrelin_dot_main.cpp when it runs
 * against the CPU stand-in of tests/cpp/mock (whose generated versions of these entries only fail), next to the toy entries of
 * tests/cpp_level, tests/cpp_mulrelin, tests/cpp_keyswitch, tests/cpp_baseconv_ntt and tests/cpp_baseconv.  The toy sum of tensor
 * products is the toy tensor product of every (group, term) added up in term order by the stand-in's element-wise ADD (its operations
 * do not commute); the toy multiplication is (D0, D1) + the toy level key switch of D2, and with NFLHIP_MULRELIN_RESCALE the first
 * level - 1 rows of that.  So what it keeps of the real entries is what the header layer relies on: which operand is which, the
 * strides (in polynomials of `rows` rows, group stride 0 = shared), the number of terms, K and the level, the key in the parent's
 * layout, the rescaled outputs' rows and, through the stand-in's own device copy, that every buffer belongs to the device of the
 * context the call is made on and is as long as the call reads. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }
static int own_operand(nflhip_ctx *ctx, const nflhip_dot_operand *x, size_t groups, size_t terms, size_t pbytes, void *stream) {
  return x ? own(ctx, x->ptr, ((groups - 1) * x->group_stride + (terms - 1) * x->term_stride + 1) * pbytes, stream) : NFLHIP_OK;
}
static const char *at(const nflhip_dot_operand *x, size_t g, size_t j, size_t pbytes) {
  return (const char *)x->ptr + (g * x->group_stride + j * x->term_stride) * pbytes;
}

/* D[c] = [groups][rows][n], c < 3, into three buffers */
static int toy_tensor_dot(nflhip_ctx *ctx, char *const D[3], const nflhip_dot_operand *a0, const nflhip_dot_operand *a1, const nflhip_dot_operand *b0,
                          const nflhip_dot_operand *b1, size_t groups, size_t terms, size_t rows) {
  const size_t n = nflhip_degree(ctx), pbytes = rows * n * ((size_t)nflhip_limb_bits(ctx) / 8);
  nflhip_ctx *one = NULL;
  int rc = nflhip_ctx_create(&one, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, 1, NULL, NULL, NULL, 0);
  if (rc) return rc;
  char *t = (char *)malloc(6 * pbytes);
  if (!t) rc = NFLHIP_ERR_NOMEM;
  for (size_t g = 0; g < groups && !rc; ++g)
    for (size_t j = 0; j < terms && !rc; ++j) {
      char *const d[3] = {j ? t : t + 3 * pbytes, j ? t + pbytes : t + 4 * pbytes, j ? t + 2 * pbytes : t + 5 * pbytes};   /* term 0 starts the sums */
      rc = nflhip_tensor_ntt(ctx, d[0], d[1], d[2], at(a0, g, j, pbytes), at(a1, g, j, pbytes), b0 ? at(b0, g, j, pbytes) : NULL,
                             b1 ? at(b1, g, j, pbytes) : NULL, 1, rows, 0);
      for (int c = 0; c < 3 && !rc && j; ++c) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, t + (3 + c) * pbytes, t + (3 + c) * pbytes, d[c], NULL, rows);
      if (j + 1 == terms)
        for (int c = 0; c < 3 && !rc; ++c) memcpy(D[c] + g * pbytes, t + (3 + c) * pbytes, pbytes);
    }
  free(t);
  nflhip_ctx_destroy(one);
  return rc;
}

static int tensor_dot_args(nflhip_ctx *ctx, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1, const nflhip_dot_operand *b0,
                           const nflhip_dot_operand *b1, size_t terms, size_t rows, int flags) {
  return !ctx || flags || terms == 0 || rows == 0 || rows > nflhip_nmoduli(ctx) || !a0 || !a1 || !b0 != !b1;
}
int nflhip_tensor_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                              const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, size_t groups, size_t terms, size_t rows, int flags,
                              void *stream) {
  if (tensor_dot_args(ctx, a0, a1, b0, b1, terms, rows, flags)) return NFLHIP_ERR_INVALID;
  if (groups == 0) return NFLHIP_OK;
  const size_t pbytes = rows * nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8);
  void *const outs[3] = {d_out0, d_out1, d_out2};
  const nflhip_dot_operand *const ops[4] = {a0, a1, b0, b1};
  int rc = NFLHIP_OK;
  for (int k = 0; k < 3 && !rc; ++k) rc = outs[k] ? own(ctx, outs[k], groups * pbytes, stream) : NFLHIP_ERR_INVALID;
  for (int k = 0; k < 4 && !rc; ++k) rc = own_operand(ctx, ops[k], groups, terms, pbytes, stream);
  if (rc) return rc;
  char *const D[3] = {(char *)d_out0, (char *)d_out1, (char *)d_out2};
  return toy_tensor_dot(ctx, D, a0, a1, b0, b1, groups, terms, rows);
}
int nflhip_tensor_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0,
                          const void *h_b1, size_t groups, size_t terms, int b_shared, size_t rows, int flags) {
  const nflhip_dot_operand a0 = {h_a0, terms, 1}, a1 = {h_a1, terms, 1}, b0 = {h_b0, b_shared ? 0 : terms, 1}, b1 = {h_b1, b_shared ? 0 : terms, 1};
  if (tensor_dot_args(ctx, &a0, &a1, h_b0 ? &b0 : NULL, h_b1 ? &b1 : NULL, terms, rows, flags)) return NFLHIP_ERR_INVALID;
  if (groups == 0) return NFLHIP_OK;
  char *const D[3] = {(char *)h_out0, (char *)h_out1, (char *)h_out2};
  return toy_tensor_dot(ctx, D, &a0, &a1, h_b0 ? &b0 : NULL, h_b1 ? &b1 : NULL, groups, terms, rows);
}

static int toy_mulrelin_dot(nflhip_ctx *ctx, void *out0, void *out1, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                            const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, const void *key, size_t groups, size_t terms, size_t K,
                            size_t alpha, size_t level, int flags, void *stream, int device_ptrs) {
  const size_t dl = ctx ? nflhip_keyswitch_level_digits(ctx, K, alpha, level) : 0;
  const int plans = NFLHIP_MULRELIN_SEQUENCE | NFLHIP_MULRELIN_MERGED | NFLHIP_MULRELIN_FUSED, plan = flags & plans;
  if (dl == 0 || terms == 0 || !a0 || !a1 || !b0 != !b1 || (plan & (plan - 1)) ||
      (flags & ~(plans | NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_FLOOR | NFLHIP_MULRELIN_RESCALE)) || ((flags & NFLHIP_MULRELIN_RESCALE) && level < 2))
    return NFLHIP_ERR_INVALID;
  if (groups == 0) return NFLHIP_OK;
  const size_t n = nflhip_degree(ctx), row = n * ((size_t)nflhip_limb_bits(ctx) / 8), pbytes = level * row, ib = groups * pbytes;
  const size_t orows = (flags & NFLHIP_MULRELIN_RESCALE) ? level - 1 : level;
  int rc = NFLHIP_OK;
  if (device_ptrs) {
    const nflhip_dot_operand *const ops[4] = {a0, a1, b0, b1};
    for (int k = 0; k < 4 && !rc; ++k) rc = own_operand(ctx, ops[k], groups, terms, pbytes, stream);
    if (!rc) rc = own(ctx, out0, groups * orows * row, stream);
    if (!rc) rc = own(ctx, out1, groups * orows * row, stream);
    if (!rc) rc = own(ctx, key, 2 * dl * nflhip_nmoduli(ctx) * row, stream);
    if (rc) return rc;
  }
  nflhip_ctx *one = NULL;
  char *d = (char *)malloc(5 * ib);
  if (!d) return NFLHIP_ERR_NOMEM;
  char *const D[3] = {d, d + ib, d + 2 * ib}, *k0 = d + 3 * ib, *k1 = d + 4 * ib;
  rc = toy_tensor_dot(ctx, D, a0, a1, b0, b1, groups, terms, level);
  const int ksflags = (flags & NFLHIP_MULRELIN_CENTERED ? NFLHIP_KEYSWITCH_CENTERED : 0) | (flags & NFLHIP_MULRELIN_FLOOR ? NFLHIP_KEYSWITCH_FLOOR : 0);
  if (!rc) rc = nflhip_keyswitch_level_ntt(ctx, k0, k1, D[2], key, groups, K, alpha, level, ksflags);
  if (!rc) rc = nflhip_ctx_create(&one, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, 1, NULL, NULL, NULL, 0);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, D[0], D[0], k0, NULL, groups * level);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, D[1], D[1], k1, NULL, groups * level);
  for (size_t g = 0; g < groups && !rc; ++g) {   /* the kept rows of every polynomial */
    memcpy((char *)out0 + g * orows * row, D[0] + g * pbytes, orows * row);
    memcpy((char *)out1 + g * orows * row, D[1] + g * pbytes, orows * row);
  }
  if (one) nflhip_ctx_destroy(one);
  free(d);
  return rc;
}
int nflhip_mulrelin_dot_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const nflhip_dot_operand *a0, const nflhip_dot_operand *a1,
                                const nflhip_dot_operand *b0, const nflhip_dot_operand *b1, const void *d_key, size_t groups, size_t terms,
                                size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  return toy_mulrelin_dot(ctx, d_out0, d_out1, a0, a1, b0, b1, d_key, groups, terms, k_special, alpha, level, flags, stream, 1);
}
int nflhip_mulrelin_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                            const void *h_key, size_t groups, size_t terms, int b_shared, size_t k_special, size_t alpha, size_t level, int flags) {
  const nflhip_dot_operand a0 = {h_a0, terms, 1}, a1 = {h_a1, terms, 1}, b0 = {h_b0, b_shared ? 0 : terms, 1}, b1 = {h_b1, b_shared ? 0 : terms, 1};
  if (!h_a0 || !h_a1) return NFLHIP_ERR_INVALID;
  return toy_mulrelin_dot(ctx, h_out0, h_out1, &a0, &a1, h_b0 ? &b0 : NULL, h_b1 ? &b1 : NULL, h_key, groups, terms, k_special, alpha, level, flags, NULL, 0);
}
