/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_keyswitch_level_ntt_dev / nflhip_keyswitch_level_ntt / nflhip_mulrelin_level_ntt_dev /
 * nflhip_mulrelin_level_ntt / nflhip_keyswitch_level_digits over plain host memory, linked INTO the program tests/cpp_level/level_main.cpp
 * when it runs against the CPU stand-in of tests/cpp/mock (whose generated versions of these entries only fail), next to the toy
 * multiplication, key switch and base conversions of tests/cpp_mulrelin, tests/cpp_keyswitch, tests/cpp_baseconv_ntt and
 * tests/cpp_baseconv.  A toy level call is the header's definition over those toys: a stand-in context of level + K rows, the key
 * gathered as key_l[d][c][r] = key[d][c][phys(r)] for d < dnum_l, and the toy top-level entry on both with min(alpha, level).  So what it
 * keeps of the real entries is what the header layer relies on: which argument is K and which the level, the layouts ([batch][level][n]
 * operands, the key in the PARENT's layout with 2 dnum_l whole polynomials read, term-major), the rescaled outputs' rows, a batched
 * call equal to a loop of single calls, the host variant equal to the device variant and, through the stand-in's own device copy,
 * that every buffer belongs to the device of the context the call is made on and is as long as the call reads. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }

size_t nflhip_keyswitch_level_digits(const nflhip_ctx *ctx, size_t k_special, size_t alpha, size_t level) {
  const size_t nm = ctx ? nflhip_nmoduli(ctx) : 0;
  if (k_special == 0 || k_special >= nm || alpha == 0 || alpha > nm - k_special || level == 0 || level > nm - k_special) return 0;
  return (level + alpha - 1) / alpha;
}

/* the stand-in context over level + K rows and the gathered key; *keyl is malloc'ed */
static int level_parts(nflhip_ctx *ctx, const void *key, size_t K, size_t alpha, size_t level, nflhip_ctx **child, void **keyl) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), row = n * ((size_t)nflhip_limb_bits(ctx) / 8);
  const size_t dl = nflhip_keyswitch_level_digits(ctx, K, alpha, level), rows = level + K, hole = nm - K - level;
  char *g = (char *)malloc(2 * dl * rows * row);
  if (!g) return NFLHIP_ERR_NOMEM;
  for (size_t t = 0; t < 2 * dl; ++t)
    for (size_t r = 0; r < rows; ++r) memcpy(g + (t * rows + r) * row, (const char *)key + (t * nm + (r < level ? r : r + hole)) * row, row);
  const int rc = nflhip_ctx_create(child, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, rows, NULL, NULL, NULL, 0);
  if (rc) free(g);
  else *keyl = g;
  return rc;
}

int nflhip_keyswitch_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_in, const void *d_key, size_t batch, size_t k_special,
                                   size_t alpha, size_t level, int flags, void *stream) {
  const size_t dl = ctx ? nflhip_keyswitch_level_digits(ctx, k_special, alpha, level) : 0;
  if (dl == 0) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t row = nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8), ob = batch * level * row;
  int rc = own(ctx, d_in, ob, stream);
  if (!rc) rc = own(ctx, d_out0, ob, stream);
  if (!rc) rc = own(ctx, d_out1, ob, stream);
  if (!rc) rc = own(ctx, d_key, 2 * dl * nflhip_nmoduli(ctx) * row, stream);
  if (rc) return rc;
  nflhip_ctx *child = NULL;
  void *keyl = NULL;
  if ((rc = level_parts(ctx, d_key, k_special, alpha, level, &child, &keyl))) return rc;
  rc = nflhip_keyswitch_ntt_dev(child, d_out0, d_out1, d_in, keyl, batch, k_special, alpha < level ? alpha : level, flags, stream);
  free(keyl);
  nflhip_ctx_destroy(child);
  return rc;
}
int nflhip_keyswitch_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch, size_t k_special,
                               size_t alpha, size_t level, int flags) {
  return nflhip_keyswitch_level_ntt_dev(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, level, flags, NULL);
}

int nflhip_mulrelin_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1,
                                  const void *d_key, size_t batch, size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  const size_t dl = ctx ? nflhip_keyswitch_level_digits(ctx, k_special, alpha, level) : 0;
  if (dl == 0 || !d_b0 != !d_b1 || ((flags & NFLHIP_MULRELIN_RESCALE) && level < 2)) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t row = nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8), ib = batch * level * row;
  const size_t ob = (flags & NFLHIP_MULRELIN_RESCALE) ? ib - batch * row : ib;
  int rc = own(ctx, d_out0, ob, stream);
  if (!rc) rc = own(ctx, d_out1, ob, stream);
  const void *const ins[4] = {d_a0, d_a1, d_b0, d_b1};
  for (int k = 0; k < 4 && !rc; ++k) rc = own(ctx, ins[k], ib, stream);
  if (!rc) rc = own(ctx, d_key, 2 * dl * nflhip_nmoduli(ctx) * row, stream);
  if (rc) return rc;
  nflhip_ctx *child = NULL;
  void *keyl = NULL;
  if ((rc = level_parts(ctx, d_key, k_special, alpha, level, &child, &keyl))) return rc;
  rc = nflhip_mulrelin_ntt_dev(child, d_out0, d_out1, d_a0, d_a1, d_b0, d_b1, keyl, batch, k_special, alpha < level ? alpha : level, flags, stream);
  free(keyl);
  nflhip_ctx_destroy(child);
  return rc;
}
int nflhip_mulrelin_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                              const void *h_key, size_t batch, size_t k_special, size_t alpha, size_t level, int flags) {
  return nflhip_mulrelin_level_ntt_dev(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, level, flags, NULL);
}
