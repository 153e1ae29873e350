/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_rotate_hoisted_level_ntt_dev / nflhip_rotate_hoisted_level_ntt /
 * nflhip_lintrans_level_ntt_dev / nflhip_lintrans_level_ntt over plain host memory, linked INTO the program
 * tests/cpp_level_rotate/level_rotate_main.cpp when it runs against the CPU stand-in of tests/cpp/mock (whose generated versions of these
 * entries only fail), next to the toy rotation, linear transform, key switch and base conversions of tests/cpp_rotate,
 * tests/cpp_lintrans, tests/cpp_keyswitch, tests/cpp_baseconv_ntt and tests/cpp_baseconv.  A toy level call is the header's definition
 * over those toys: a stand-in context of level + K rows, every key gathered as key_l[d][c][r] = key[d][c][phys(r)] for d < dnum_l, every
 * weight as weight_l[r] = weight[phys(r)], and the toy top-level entry on them with min(alpha, level); level == L forwards.  The toy
 * linear transform reads the kept rows of a weight only, which are a prefix in either layout, so below the top level the special rows of
 * the gathered weight are added into its kept rows first: a weight that does not lie in the PARENT's layout on all nm rows changes the
 * result.  So what the toys keep of the real entries is what the header layer relies on: which argument is K and which the level, the
 * layouts ([batch][level][n] operands; keys in the parent's layout with 2 dnum_l whole polynomials read, term-major, one key per
 * pointer; weights whole polynomials of the parent), a batched call equal to a loop of single calls, the host variant equal to the
 * device variant and, through the stand-in's own device copy, that every buffer belongs to the device of the context the call is made
 * on and is as long as the call reads. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }

static size_t level_digits(const nflhip_ctx *ctx, size_t K, size_t alpha, size_t level) {
  const size_t nm = ctx ? nflhip_nmoduli(ctx) : 0;
  if (K == 0 || K >= nm || alpha == 0 || alpha > nm - K || level == 0 || level > nm - K) return 0;
  return (level + alpha - 1) / alpha;
}

/* polys whole polynomials of the parent gathered onto the rows A_l; malloc'ed */
static char *gather(nflhip_ctx *ctx, const void *src, size_t polys, size_t K, size_t level) {
  const size_t nm = nflhip_nmoduli(ctx), row = nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8), rows = level + K, hole = nm - K - level;
  char *g = (char *)malloc(polys * rows * row);
  if (!g) return NULL;
  for (size_t t = 0; t < polys; ++t)
    for (size_t r = 0; r < rows; ++r) memcpy(g + (t * rows + r) * row, (const char *)src + (t * nm + (r < level ? r : r + hole)) * row, row);
  return g;
}

/* the shared body: weights == NULL is the rotation (outs = count pairs), else the linear transform (outs = one pair) */
static int level_call(nflhip_ctx *ctx, void *const *out0s, void *const *out1s, const void *c0, const void *c1, const void *const *keys,
                      const void *const *weights, const uint64_t *ks, size_t count, size_t batch, size_t K, size_t alpha, size_t level, int flags,
                      void *stream) {
  const size_t dl = level_digits(ctx, K, alpha, level), max = weights ? NFLHIP_LINTRANS_MAX_TERMS : NFLHIP_ROTATE_MAX_OUTPUTS;
  if (dl == 0 || count == 0 || count > max) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wbytes = (size_t)nflhip_limb_bits(ctx) / 8, row = n * wbytes, ob = batch * level * row;
  const size_t nouts = weights ? 1 : count, rows = level + K;
  int rc = own(ctx, c1, ob, stream);
  if (!rc) rc = own(ctx, c0, ob, stream);
  for (size_t m = 0; m < nouts && !rc; ++m) {
    rc = own(ctx, out0s[m], ob, stream);
    if (!rc) rc = own(ctx, out1s[m], ob, stream);
  }
  for (size_t m = 0; m < count && !rc; ++m) {
    if (!weights && !keys[m]) return NFLHIP_ERR_INVALID;
    rc = own(ctx, keys[m], 2 * dl * nm * row, stream);
    if (!rc && weights) rc = own(ctx, weights[m], nm * row, stream);
  }
  if (rc) return rc;
  if (level == nm - K)
    return weights ? nflhip_lintrans_ntt_dev(ctx, out0s[0], out1s[0], c0, c1, keys, weights, ks, count, batch, K, alpha, flags, stream)
                   : nflhip_rotate_hoisted_ntt_dev(ctx, out0s, out1s, c0, c1, keys, ks, count, batch, K, alpha, flags, stream);
  nflhip_ctx *child = NULL;
  if ((rc = nflhip_ctx_create(&child, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, rows, NULL, NULL, NULL, 0))) return rc;
  const void *gk[NFLHIP_LINTRANS_MAX_TERMS] = {0}, *gw[NFLHIP_LINTRANS_MAX_TERMS] = {0};
  for (size_t m = 0; m < count && !rc; ++m) {
    if (keys[m] && !(gk[m] = gather(ctx, keys[m], 2 * dl, K, level))) rc = NFLHIP_ERR_NOMEM;
    if (!rc && weights) {
      char *w = gather(ctx, weights[m], 1, K, level);
      if (!w) {
        rc = NFLHIP_ERR_NOMEM;
        break;
      }
      for (size_t r = 0; r < level; ++r)   /* (the special rows into the kept ones, byte-wise: only the layout matters) */
        for (size_t i = 0; i < row; ++i) w[r * row + i] = (char)(w[r * row + i] ^ w[(level + r % K) * row + i]);
      gw[m] = w;
    }
  }
  const size_t al = alpha < level ? alpha : level;
  if (!rc)
    rc = weights ? nflhip_lintrans_ntt_dev(child, out0s[0], out1s[0], c0, c1, gk, gw, ks, count, batch, K, al, flags, stream)
                 : nflhip_rotate_hoisted_ntt_dev(child, out0s, out1s, c0, c1, gk, ks, count, batch, K, al, flags, stream);
  for (size_t m = 0; m < count; ++m) {
    free((void *)gk[m]);
    free((void *)gw[m]);
  }
  nflhip_ctx_destroy(child);
  return rc;
}

int nflhip_rotate_hoisted_level_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                        const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                        size_t level, int flags, void *stream) {
  return level_call(ctx, d_out0s, d_out1s, d_c0, d_c1, d_keys, NULL, ks, count, batch, k_special, alpha, level, flags, stream);
}
int nflhip_rotate_hoisted_level_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                                    const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                    size_t level, int flags) {
  return level_call(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, NULL, ks, count, batch, k_special, alpha, level, flags, NULL);
}
int nflhip_lintrans_level_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_keys,
                                  const void *const *d_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                  size_t level, int flags, void *stream) {
  if (!d_weights) return NFLHIP_ERR_INVALID;
  return level_call(ctx, &d_out0, &d_out1, d_c0, d_c1, d_keys, d_weights, ks, count, batch, k_special, alpha, level, flags, stream);
}
int nflhip_lintrans_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_keys,
                              const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                              size_t level, int flags) {
  if (!h_weights) return NFLHIP_ERR_INVALID;
  return level_call(ctx, &h_out0, &h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, level, flags, NULL);
}
