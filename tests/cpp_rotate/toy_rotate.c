/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_rotate_hoisted_ntt_dev / nflhip_rotate_hoisted_ntt and toy NTT-form automorphisms
 * (nflhip_automorphism_dev, nflhip_automorphism) over plain host memory, linked INTO the program tests/cpp_rotate/rotate_main.cpp when
 * it runs against the CPU stand-in of tests/cpp/mock (whose generated versions of these entries only fail), next to the toy key switch
 * of tests/cpp_keyswitch and the toy base conversions.  The toy rotation is the header's definition over the other toys: per rotation
 * nflhip_keyswitch_ntt_dev of c1 against keys[m], the stand-in's own element-wise ADD of c0, the toy permutation by ks[m] of both
 * results -- so what it keeps of the real entry is what the header layer relies on: the layouts ([batch][L][n] ciphertext and outputs,
 * one [dnum][2][nm][n] key per rotation), the pairing of keys[m] with ks[m], c0 added to out0 only, a NULL c0, a batched call equal to
 * a loop of single calls, the host variant equal to the device variant and, through the stand-in's own device copy, that every buffer
 * belongs to the device of the context the call is made on. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream); }

/* the toy permutation of a row: out[j] = in[j k mod n] -- a bijection for odd k, the identity for k = 1, and it composes like the
 * real one (k then k' is k k') */
static int permute(nflhip_ctx *ctx, void *out, const void *in, size_t batch, uint64_t k) {
  const size_t n = nflhip_degree(ctx), rows = batch * nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8;
  if (!(k & 1)) return NFLHIP_ERR_INVALID;
  for (size_t r = 0; r < rows; ++r)
    for (size_t j = 0; j < n; ++j) memcpy((char *)out + (r * n + j) * wb, (const char *)in + (r * n + (size_t)((j * k) % n)) * wb, wb);
  return NFLHIP_OK;
}
int nflhip_automorphism_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, uint64_t k, int form, void *stream) {
  const size_t bytes = batch * nflhip_degree(ctx) * nflhip_nmoduli(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8);
  if (form != NFLHIP_FORM_NTT) return NFLHIP_ERR_UNSUPPORTED; /* (the toy has no coefficient form) */
  int rc = own(ctx, d_out, bytes, stream);
  if (!rc) rc = own(ctx, d_in, bytes, stream);
  return rc ? rc : permute(ctx, d_out, d_in, batch, k);
}
int nflhip_automorphism(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, uint64_t k, int form) {
  if (form != NFLHIP_FORM_NTT) return NFLHIP_ERR_UNSUPPORTED;
  return permute(ctx, h_out, h_in, batch, k);
}

int nflhip_rotate_hoisted_ntt_dev(nflhip_ctx *ctx, void *const *d_out0s, void *const *d_out1s, const void *d_c0, const void *d_c1,
                                  const void *const *d_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                  int flags, void *stream) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, dnum = nflhip_keyswitch_digits(ctx, k_special, alpha);
  const int plan = flags & (NFLHIP_ROTATE_SEQUENCE | NFLHIP_ROTATE_HOISTED);
  if (dnum == 0 || count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS || (flags & ~(plan | NFLHIP_ROTATE_CENTERED | NFLHIP_ROTATE_FLOOR)) ||
      plan == (NFLHIP_ROTATE_SEQUENCE | NFLHIP_ROTATE_HOISTED))
    return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t L = nm - k_special, ob = batch * L * n * wb;
  int rc = own(ctx, d_c1, ob, stream);
  if (!rc && d_c0) rc = own(ctx, d_c0, ob, stream);
  for (size_t m = 0; m < count && !rc; ++m) {
    if (!(ks[m] & 1)) return NFLHIP_ERR_INVALID;
    rc = own(ctx, d_out0s[m], ob, stream);
    if (!rc) rc = own(ctx, d_out1s[m], ob, stream);
    if (!rc) rc = own(ctx, d_keys[m], 2 * dnum * nm * n * wb, stream);
  }
  if (rc) return rc;
  /* the ring of the ciphertext: a stand-in context with the first L moduli, for its element-wise ADD and the row count of permute */
  nflhip_ctx *kept = NULL;
  if ((rc = nflhip_ctx_create(&kept, nflhip_ctx_device(ctx), nflhip_limb_bits(ctx), n, L, NULL, NULL, NULL, 0))) return rc;
  char *t0 = (char *)malloc(2 * ob), *t1 = t0 + ob;
  if (!t0) rc = NFLHIP_ERR_NOMEM;
  for (size_t m = 0; m < count && !rc; ++m) {
    rc = nflhip_keyswitch_ntt_dev(ctx, t0, t1, d_c1, d_keys[m], batch, k_special, alpha, flags & (NFLHIP_ROTATE_CENTERED | NFLHIP_ROTATE_FLOOR), stream);
    if (!rc && d_c0) rc = nflhip_pointwise(kept, NFLHIP_OP_ADD, t0, t0, d_c0, NULL, batch);
    if (!rc) rc = permute(kept, d_out0s[m], t0, batch, ks[m]);
    if (!rc) rc = permute(kept, d_out1s[m], t1, batch, ks[m]);
  }
  free(t0);
  nflhip_ctx_destroy(kept);
  return rc;
}
int nflhip_rotate_hoisted_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                              const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags) {
  return nflhip_rotate_hoisted_ntt_dev(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, ks, count, batch, k_special, alpha, flags, NULL);
}
