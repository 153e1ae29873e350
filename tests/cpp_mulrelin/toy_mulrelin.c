/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_tensor_ntt_dev / nflhip_tensor_ntt / nflhip_mulrelin_ntt_dev / nflhip_mulrelin_ntt over
 * plain host memory, linked INTO the program tests/cpp_mulrelin/mulrelin_main.cpp when it runs against the CPU stand-in of tests/cpp/mock
 * (whose generated versions of these entries only fail), next to the toy key switch of tests/cpp_keyswitch and the toy base conversions
 * under it.  The toy tensor product is the stand-in's element-wise MUL and ADD in the order a0 b0, a0 b1 + a1 b0, a1 b1 (the stand-in's
 * operations do not commute); the toy multiplication is (d0, d1) + the toy key switch of d2, and with NFLHIP_MULRELIN_RESCALE the first
 * L - 1 rows of that.  So what it keeps of the real entries is what the header layer relies on: which operand is which, the layouts
 * ([batch][L][n] in, [batch][L or L - 1][n] out, the key as the key switch takes it), the square as b = a, a batched call equal to a
 * loop of single calls, the host variant equal to the device variant and, through the stand-in's own device copy, that every buffer
 * belongs to the device of the context the call is made on. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }

/* the three components over `rows` rows of `batch` polynomials, through the stand-in's element-wise entry on a one-row context */
static int toy_tensor(nflhip_ctx *ctx, void *o0, void *o1, void *o2, const void *a0, const void *a1, const void *b0, const void *b1, size_t batch,
                      size_t rows) {
  const size_t n = nflhip_degree(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, bytes = batch * rows * n * wb;
  nflhip_ctx *one = NULL;
  int rc = nflhip_ctx_create(&one, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, 1, NULL, NULL, NULL, 0);
  if (rc) return rc;
  if (!b0) b0 = a0, b1 = a1;
  char *t = (char *)malloc(5 * (bytes ? bytes : 1)), *d0 = t, *d1 = d0 + bytes, *d2 = d1 + bytes, *x = d2 + bytes, *y = x + bytes;
  if (!t) rc = NFLHIP_ERR_NOMEM;
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_MUL, d0, a0, b0, NULL, batch * rows);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_MUL, x, a0, b1, NULL, batch * rows);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_MUL, y, a1, b0, NULL, batch * rows);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, d1, x, y, NULL, batch * rows);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_MUL, d2, a1, b1, NULL, batch * rows);
  if (!rc) memcpy(o0, d0, bytes), memcpy(o1, d1, bytes), memcpy(o2, d2, bytes);   /* (an output may be an input) */
  free(t);
  nflhip_ctx_destroy(one);
  return rc;
}

int nflhip_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1, const void *d_b0,
                          const void *d_b1, size_t batch, size_t rows, int flags, void *stream) {
  if (!ctx || flags || rows == 0 || rows > nflhip_nmoduli(ctx) || !d_b0 != !d_b1) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t bytes = batch * rows * nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8);
  const void *const all[7] = {d_out0, d_out1, d_out2, d_a0, d_a1, d_b0, d_b1};
  for (int k = 0; k < 7; ++k) {
    const int rc = own(ctx, all[k], bytes, stream);
    if (rc) return rc;
  }
  return toy_tensor(ctx, d_out0, d_out1, d_out2, d_a0, d_a1, d_b0, d_b1, batch, rows);
}
int nflhip_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                      size_t batch, size_t rows, int flags) {
  if (!ctx || flags || rows == 0 || rows > nflhip_nmoduli(ctx) || !h_b0 != !h_b1) return NFLHIP_ERR_INVALID;
  return batch ? toy_tensor(ctx, h_out0, h_out1, h_out2, h_a0, h_a1, h_b0, h_b1, batch, rows) : NFLHIP_OK;
}

static int toy_mulrelin(nflhip_ctx *ctx, void *out0, void *out1, const void *a0, const void *a1, const void *b0, const void *b1, const void *key,
                        size_t batch, size_t k_special, size_t alpha, int flags, void *stream, int device_ptrs) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, dnum = nflhip_keyswitch_digits(ctx, k_special, alpha);
  const int plans = NFLHIP_MULRELIN_SEQUENCE | NFLHIP_MULRELIN_MERGED | NFLHIP_MULRELIN_FUSED, plan = flags & plans;
  if (dnum == 0 || (flags & ~(plans | NFLHIP_MULRELIN_CENTERED | NFLHIP_MULRELIN_FLOOR | NFLHIP_MULRELIN_RESCALE)) || (plan & (plan - 1)) || !b0 != !b1)
    return NFLHIP_ERR_INVALID;
  const size_t L = nm - k_special, row = n * wb, ib = batch * L * row, orows = (flags & NFLHIP_MULRELIN_RESCALE) ? L - 1 : L;
  if (orows == 0) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  int rc = NFLHIP_OK;
  if (device_ptrs) {
    const void *const ins[4] = {a0, a1, b0, b1};
    for (int k = 0; k < 4 && !rc; ++k) rc = own(ctx, ins[k], ib, stream);
    if (!rc) rc = own(ctx, out0, batch * orows * row, stream);
    if (!rc) rc = own(ctx, out1, batch * orows * row, stream);
    if (!rc) rc = own(ctx, key, 2 * dnum * nm * row, stream);
    if (rc) return rc;
  }
  nflhip_ctx *one = NULL;
  char *d = (char *)malloc(5 * ib), *d0 = d, *d1 = d0 + ib, *d2 = d1 + ib, *k0 = d2 + ib, *k1 = k0 + ib;
  if (!d) return NFLHIP_ERR_NOMEM;
  rc = toy_tensor(ctx, d0, d1, d2, a0, a1, b0, b1, batch, L);
  const int ksflags = (flags & NFLHIP_MULRELIN_CENTERED ? NFLHIP_KEYSWITCH_CENTERED : 0) | (flags & NFLHIP_MULRELIN_FLOOR ? NFLHIP_KEYSWITCH_FLOOR : 0);
  if (!rc) rc = nflhip_keyswitch_ntt(ctx, k0, k1, d2, key, batch, k_special, alpha, ksflags);
  if (!rc) rc = nflhip_ctx_create(&one, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, 1, NULL, NULL, NULL, 0);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, d0, d0, k0, NULL, batch * L);
  if (!rc) rc = nflhip_pointwise(one, NFLHIP_OP_ADD, d1, d1, k1, NULL, batch * L);
  for (size_t b = 0; b < batch && !rc; ++b) {   /* the kept rows of every polynomial */
    memcpy((char *)out0 + b * orows * row, d0 + b * L * row, orows * row);
    memcpy((char *)out1 + b * orows * row, d1 + b * L * row, orows * row);
  }
  if (one) nflhip_ctx_destroy(one);
  free(d);
  return rc;
}
int nflhip_mulrelin_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1,
                            const void *d_key, size_t batch, size_t k_special, size_t alpha, int flags, void *stream) {
  if (!ctx) return NFLHIP_ERR_INVALID;
  return toy_mulrelin(ctx, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, d_key, batch, k_special, alpha, flags, stream, 1);
}
int nflhip_mulrelin_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                        const void *h_key, size_t batch, size_t k_special, size_t alpha, int flags) {
  if (!ctx) return NFLHIP_ERR_INVALID;
  return toy_mulrelin(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, flags, NULL, 0);
}
