/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_keyswitch_ntt_dev / nflhip_keyswitch_ntt / nflhip_keyswitch_digits and toy sums of
 * products (nflhip_dot_dev, nflhip_dot) over plain host memory, linked INTO the program tests/cpp_keyswitch/keyswitch_main.cpp when it
 * runs against the CPU stand-in of tests/cpp/mock (whose generated versions of these entries only fail), next to the toy base
 * conversions of tests/cpp_baseconv_ntt and tests/cpp_baseconv.  The toy key switch is the header's definition over the other toys:
 * the input embedded into nm rows, nflhip_baseconv_ntt_dev per digit, the sum of products per component, nflhip_moddown_ntt_dev -- so
 * what it keeps of the real entry is what the header layer relies on: the layouts ([batch][L][n] in and out, [dnum][2][nm][n] key,
 * term-major), the digit ranges, a batched call equal to a loop of single calls, the host variant equal to the device variant and,
 * through the stand-in's own device copy, that every buffer belongs to the device of the context the call is made on. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static uint64_t ldw(size_t wb, const void *p, size_t i) {
  return wb == 8 ? ((const uint64_t *)p)[i] : wb == 4 ? ((const uint32_t *)p)[i] : ((const uint16_t *)p)[i];
}
static void stw(size_t wb, void *p, size_t i, uint64_t v) {
  if (wb == 8) ((uint64_t *)p)[i] = v;
  else if (wb == 4) ((uint32_t *)p)[i] = (uint32_t)v;
  else ((uint16_t *)p)[i] = (uint16_t)v;
}
static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream); }

/* out[g] = addend[g] + sum_j a(g, j) b(g, j), word by word, wrapping */
int nflhip_dot_dev(nflhip_ctx *ctx, void *d_out, const nflhip_dot_operand *a, const nflhip_dot_operand *b, const void *d_addend, size_t groups,
                   size_t terms, int flags, void *stream) {
  const size_t words = nflhip_degree(ctx) * nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8;
  (void)stream;
  if (!a || !b || terms == 0 || (flags & ~NFLHIP_DOT_UNTILED)) return NFLHIP_ERR_INVALID;
  for (size_t g = 0; g < groups; ++g)
    for (size_t w = 0; w < words; ++w) {
      uint64_t s = d_addend ? ldw(wb, d_addend, g * words + w) : 0;
      for (size_t j = 0; j < terms; ++j)
        s += ldw(wb, a->ptr, (g * a->group_stride + j * a->term_stride) * words + w) * ldw(wb, b->ptr, (g * b->group_stride + j * b->term_stride) * words + w);
      stw(wb, d_out, g * words + w, s);
    }
  return NFLHIP_OK;
}
int nflhip_dot(nflhip_ctx *ctx, void *h_out, const void *h_a, const void *h_b, size_t groups, size_t terms, int b_shared) {
  const nflhip_dot_operand a = {h_a, terms, 1}, b = {h_b, b_shared ? 0 : terms, 1};
  return nflhip_dot_dev(ctx, h_out, &a, &b, NULL, groups, terms, 0, NULL);
}

size_t nflhip_keyswitch_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha) {
  const size_t nm = nflhip_nmoduli(ctx);
  if (k_special == 0 || k_special >= nm || alpha == 0 || alpha > nm - k_special) return 0;
  return (nm - k_special + alpha - 1) / alpha;
}
int nflhip_keyswitch_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch, size_t k_special,
                             size_t alpha, int flags, void *stream) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, dnum = nflhip_keyswitch_digits(ctx, k_special, alpha);
  const int plan = flags & (NFLHIP_KEYSWITCH_COMPOSED | NFLHIP_KEYSWITCH_FUSED | NFLHIP_KEYSWITCH_SEQUENCE);
  if (dnum == 0 || (flags & ~(plan | NFLHIP_KEYSWITCH_CENTERED | NFLHIP_KEYSWITCH_FLOOR)) || (plan & (plan - 1))) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t L = nm - k_special, row = n * wb, pb = nm * row;
  int rc = own(ctx, d_in, batch * L * row, stream);
  if (!rc) rc = own(ctx, d_out0, batch * L * row, stream);
  if (!rc) rc = own(ctx, d_out1, batch * L * row, stream);
  if (!rc) rc = own(ctx, d_key, 2 * dnum * pb, stream);
  if (rc) return rc;
  char *X = (char *)calloc(batch * (3 + dnum), pb), *U = X + batch * pb, *acc = U + dnum * batch * pb;
  if (!X) return NFLHIP_ERR_NOMEM;
  for (size_t b = 0; b < batch; ++b) memcpy(X + b * pb, (const char *)d_in + b * L * row, L * row);
  for (size_t d = 0; d < dnum && !rc; ++d) {
    const size_t s0 = d * alpha, ks = L - s0 < alpha ? L - s0 : alpha;
    rc = nflhip_baseconv_ntt_dev(ctx, U + d * batch * pb, X, batch, s0, ks, 0, nm, flags & NFLHIP_KEYSWITCH_CENTERED ? NFLHIP_BASECONV_CENTERED : 0, stream);
  }
  for (size_t c = 0; c < 2 && !rc; ++c) {
    const nflhip_dot_operand a = {U, 1, batch}, k = {(const char *)d_key + c * pb, 0, 2};
    rc = nflhip_dot_dev(ctx, acc + c * batch * pb, &a, &k, NULL, batch, dnum, 0, stream);
    if (!rc) rc = nflhip_moddown_ntt_dev(ctx, c ? d_out1 : d_out0, acc + c * batch * pb, batch, k_special, flags & NFLHIP_KEYSWITCH_FLOOR ? NFLHIP_MODDOWN_FLOOR : 0, stream);
  }
  free(X);
  return rc;
}
int nflhip_keyswitch_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch, size_t k_special, size_t alpha,
                         int flags) {
  return nflhip_keyswitch_ntt_dev(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, flags, NULL);
}
