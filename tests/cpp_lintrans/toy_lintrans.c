/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_lintrans_ntt_dev / nflhip_lintrans_ntt over plain host memory, linked INTO the
 * program tests/cpp_lintrans/lintrans_main.cpp when it runs against the CPU stand-in of tests/cpp/mock (whose generated versions of
 * these entries only fail), next to the toy permutation of tests/cpp_rotate, the toy key switch of tests/cpp_keyswitch and the toy
 * base conversions.  The toy has no extended basis to accumulate in: it is, over the other toys and the stand-in's own element-wise
 * MUL and ADD on the first L rows, term by term in order,
 *     out0 = sum_{keyed m} w_m (.) perm_{k_m}(d0_m)  +  sum_{all m} w_m (.) perm_{k_m}(c0),      (d0_m, d1_m) = toy key switch of c1
 *     out1 = sum_{keyed m} w_m (.) perm_{k_m}(d1_m)  +  sum_{unkeyed m} w_m (.) c1,
 * the first term of a sum assigned, the others added.  What it keeps of the real entry is what the header layer relies on: the
 * layouts ([batch][L][n] ciphertext and outputs, one [dnum][2][nm][n] key and one [nm][n] diagonal per term, the diagonal's first L
 * rows used on the kept rows), the pairing of keys[m], weights[m] and ks[m], a NULL key for the unrotated diagonal, c0 in out0 only, a
 * NULL c0, a batched call equal to a loop of single calls, the host variant equal to the device variant and, through the stand-in's
 * own device copy, that every buffer belongs to the device of the context the call is made on. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream); }

/* out (+)= w (.) x for every polynomial of the batch; *have: out already holds a term */
static int add_term(nflhip_ctx *kept, char *out, const void *w, const char *x, char *tmp, size_t batch, size_t qb, int *have) {
  int rc = NFLHIP_OK;
  for (size_t g = 0; g < batch && !rc; ++g) {
    rc = nflhip_pointwise(kept, NFLHIP_OP_MUL, *have ? tmp : out + g * qb, w, x + g * qb, NULL, 1);
    if (!rc && *have) rc = nflhip_pointwise(kept, NFLHIP_OP_ADD, out + g * qb, out + g * qb, tmp, NULL, 1);
  }
  *have = 1;
  return rc;
}

int nflhip_lintrans_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, const void *const *d_keys,
                            const void *const *d_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags,
                            void *stream) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, dnum = nflhip_keyswitch_digits(ctx, k_special, alpha);
  const int plan = flags & (NFLHIP_LINTRANS_SEQUENCE | NFLHIP_LINTRANS_HOISTED);
  if (dnum == 0 || count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS || (flags & ~(plan | NFLHIP_LINTRANS_CENTERED | NFLHIP_LINTRANS_FLOOR)) ||
      plan == (NFLHIP_LINTRANS_SEQUENCE | NFLHIP_LINTRANS_HOISTED))
    return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t L = nm - k_special, qb = L * n * wb, ob = batch * qb;
  int rc = own(ctx, d_c1, ob, stream);
  if (!rc && d_c0) rc = own(ctx, d_c0, ob, stream);
  if (!rc) rc = own(ctx, d_out0, ob, stream);
  if (!rc) rc = own(ctx, d_out1, ob, stream);
  for (size_t m = 0; m < count && !rc; ++m) {
    if (!(ks[m] & 1) || (!d_keys[m] && ks[m] % (2 * n) != 1)) return NFLHIP_ERR_INVALID;
    if (d_keys[m]) rc = own(ctx, d_keys[m], 2 * dnum * nm * n * wb, stream);
    if (!rc) rc = own(ctx, d_weights[m], nm * n * wb, stream);
  }
  if (rc) return rc;
  /* the ring of the ciphertext: a stand-in context with the first L moduli, for its element-wise ops and the toy permutation's row count */
  nflhip_ctx *kept = NULL;
  if ((rc = nflhip_ctx_create(&kept, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, L, NULL, NULL, NULL, 0))) return rc;
  char *t0 = (char *)malloc(5 * ob + qb), *t1 = t0 + ob, *p = t1 + ob, *r0 = p + ob, *r1 = r0 + ob, *tmp = r1 + ob;
  int have0 = 0, have1 = 0;
  if (!t0) rc = NFLHIP_ERR_NOMEM;
  for (size_t m = 0; m < count && !rc; ++m) {
    if (!d_keys[m]) continue;
    rc = nflhip_keyswitch_ntt_dev(ctx, t0, t1, d_c1, d_keys[m], batch, k_special, alpha, flags & (NFLHIP_LINTRANS_CENTERED | NFLHIP_LINTRANS_FLOOR), stream);
    if (!rc) rc = nflhip_automorphism(kept, p, t0, batch, ks[m], NFLHIP_FORM_NTT);
    if (!rc) rc = add_term(kept, r0, d_weights[m], p, tmp, batch, qb, &have0);
    if (!rc) rc = nflhip_automorphism(kept, p, t1, batch, ks[m], NFLHIP_FORM_NTT);
    if (!rc) rc = add_term(kept, r1, d_weights[m], p, tmp, batch, qb, &have1);
  }
  for (size_t m = 0; m < count && !rc && d_c0; ++m) {
    rc = nflhip_automorphism(kept, p, d_c0, batch, ks[m], NFLHIP_FORM_NTT);
    if (!rc) rc = add_term(kept, r0, d_weights[m], p, tmp, batch, qb, &have0);
  }
  for (size_t m = 0; m < count && !rc; ++m)
    if (!d_keys[m]) rc = add_term(kept, r1, d_weights[m], (const char *)d_c1, tmp, batch, qb, &have1);
  if (!rc) {
    if (have0) memcpy(d_out0, r0, ob);
    else memset(d_out0, 0, ob);
    if (have1) memcpy(d_out1, r1, ob);
    else memset(d_out1, 0, ob);
  }
  free(t0);
  nflhip_ctx_destroy(kept);
  return rc;
}
int nflhip_lintrans_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_keys,
                        const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags) {
  return nflhip_lintrans_ntt_dev(ctx, h_out0, h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, flags, NULL);
}
