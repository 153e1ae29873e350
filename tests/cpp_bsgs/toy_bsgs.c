/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_bsgs_ntt_dev / nflhip_bsgs_ntt over plain host memory, linked INTO the program
 * tests/cpp_bsgs/bsgs_main.cpp when it runs against the CPU stand-in of tests/cpp/mock (whose generated versions of these entries only
 * fail), next to the toy level entries of tests/cpp_level_rotate and the toys they build on.  A toy BSGS call is today's way over those
 * toys: per giant step j the toy level linear transform of (c0, c1) with the baby keys and the diagonals weights[j * n1 + i] that are not
 * NULL, then, where gkeys[j] is not NULL, the toy level rotation of that pair by gks[j] with gkeys[j]; the pairs are combined byte by byte
 * (exclusive or: only the layout matters).  So what the toy keeps of the real entry is what the header layer relies on: which keys are
 * the babies' and which the giants', that the diagonal of (j, i) lies at j * n1 + i, which argument is K and which the level, the layouts
 * of the level entries, a batched call equal to a loop of single calls, the host variant equal to the device variant and, through the
 * stand-in's own device copy, that every buffer belongs to the device of the context and is as long as the call reads. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }

static int bsgs_call(nflhip_ctx *ctx, void *out0, void *out1, const void *c0, const void *c1, const void *const *bkeys, const uint64_t *bks, size_t n1,
                     const void *const *gkeys, const uint64_t *gks, size_t n2, const void *const *weights, size_t batch, size_t K, size_t alpha,
                     size_t level, int flags, void *stream, int host) {
  const size_t nm = ctx ? nflhip_nmoduli(ctx) : 0;
  if (K == 0 || K >= nm || alpha == 0 || alpha > nm - K || level == 0 || level > nm - K) return NFLHIP_ERR_INVALID;
  if (n1 == 0 || n1 > NFLHIP_BSGS_MAX_BABY || n2 == 0 || n2 > NFLHIP_BSGS_MAX_GIANT) return NFLHIP_ERR_INVALID;
  if (flags & ~(NFLHIP_BSGS_CENTERED | NFLHIP_BSGS_FLOOR)) return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t dl = (level + alpha - 1) / alpha, row = nflhip_degree(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8), ob = batch * level * row;
  int rc = own(ctx, c1, ob, stream);
  if (!rc) rc = own(ctx, c0, ob, stream);
  if (!rc) rc = own(ctx, out0, ob, stream);
  if (!rc) rc = own(ctx, out1, ob, stream);
  for (size_t m = 0; m < n1 + n2 && !rc; ++m) rc = own(ctx, m < n1 ? bkeys[m] : gkeys[m - n1], 2 * dl * nm * row, stream);
  for (size_t q = 0; q < n1 * n2 && !rc; ++q) rc = own(ctx, weights[q], nm * row, stream);
  if (rc) return rc;
  char *buf = (char *)calloc(6, ob), *a0 = buf, *a1 = buf + ob, *t0 = a1 + ob, *t1 = t0 + ob, *r0 = t1 + ob, *r1 = r0 + ob;
  if (!buf) return NFLHIP_ERR_NOMEM;
  for (size_t j = 0; j < n2 && !rc; ++j) {
    const void *kp[NFLHIP_BSGS_MAX_BABY], *wp[NFLHIP_BSGS_MAX_BABY];
    uint64_t ks[NFLHIP_BSGS_MAX_BABY];
    size_t cnt = 0;
    for (size_t i = 0; i < n1; ++i)
      if (weights[j * n1 + i]) kp[cnt] = bkeys[i], wp[cnt] = weights[j * n1 + i], ks[cnt++] = bks[i];
    if (!cnt) rc = NFLHIP_ERR_INVALID;
    if (!rc)
      rc = host ? nflhip_lintrans_level_ntt(ctx, t0, t1, c0, c1, kp, wp, ks, cnt, batch, K, alpha, level, flags)
                : nflhip_lintrans_level_ntt_dev(ctx, t0, t1, c0, c1, kp, wp, ks, cnt, batch, K, alpha, level, flags, stream);
    const char *s0 = t0, *s1 = t1;
    if (!rc && gkeys[j]) {
      void *o0 = r0, *o1 = r1;
      rc = host ? nflhip_rotate_hoisted_level_ntt(ctx, &o0, &o1, t0, t1, &gkeys[j], &gks[j], 1, batch, K, alpha, level, flags)
                : nflhip_rotate_hoisted_level_ntt_dev(ctx, &o0, &o1, t0, t1, &gkeys[j], &gks[j], 1, batch, K, alpha, level, flags, stream);
      s0 = r0, s1 = r1;
    }
    for (size_t b = 0; b < ob && !rc; ++b) a0[b] = (char)(a0[b] ^ s0[b]), a1[b] = (char)(a1[b] ^ s1[b]);
  }
  if (!rc) memcpy(out0, a0, ob), memcpy(out1, a1, ob);
  free(buf);
  return rc;
}

int nflhip_bsgs_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_bkeys, const uint64_t *bks,
                        size_t n1, const void *const *d_gkeys, const uint64_t *gks, size_t n2, const void *const *d_weights, size_t batch,
                        size_t k_special, size_t alpha, size_t level, int flags, void *stream) {
  return bsgs_call(ctx, d_out0, d_out1, d_c0, d_c1, d_bkeys, bks, n1, d_gkeys, gks, n2, d_weights, batch, k_special, alpha, level, flags, stream, 0);
}
int nflhip_bsgs_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_bkeys, const uint64_t *bks,
                    size_t n1, const void *const *h_gkeys, const uint64_t *gks, size_t n2, const void *const *h_weights, size_t batch, size_t k_special,
                    size_t alpha, size_t level, int flags) {
  return bsgs_call(ctx, h_out0, h_out1, h_c0, h_c1, h_bkeys, bks, n1, h_gkeys, gks, n2, h_weights, batch, k_special, alpha, level, flags, NULL, 1);
}
