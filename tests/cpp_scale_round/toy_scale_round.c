/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_scale_round_dev / nflhip_scale_round_ntt_dev / nflhip_bfv_tensor_ntt_dev and their
 * host variants over plain host memory, linked INTO the program tests/cpp_scale_round/scale_round_main.cpp when it runs against the CPU
 * stand-in of tests/cpp/mock (whose generated versions of these entries only fail), next to the toy tensor product of
 * tests/cpp_mulrelin and the toy base conversions under it.  The toy scale-round is a word-wise scramble of all nmoduli words of a
 * position, of ks, t, the form and the floor flag, written to the dense [batch][ks][n] (KEEP: [batch][nmoduli - ks][n]); the toy
 * tensor product is the four steps of the header's definition through the toy entries.  So what they keep of the real entries is what
 * the header layer relies on: which operand is which, ks, t and the flags passed through, the layouts, a batched call equal to a loop
 * of single calls, the host variant equal to the device variant and, through the stand-in's own device copy, that every buffer belongs
 * to the device of the context the call is made on. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "nflhip.h"

static uint64_t mixw(uint64_t h, uint64_t v) { h = (h ^ v) * 0x9E3779B97F4A7C15ull; return h ^ (h >> 31); }
static uint64_t ldw(size_t wb, const void *p, size_t i) {
  return wb == 8 ? ((const uint64_t *)p)[i] : wb == 4 ? ((const uint32_t *)p)[i] : ((const uint16_t *)p)[i];
}
static void stw(size_t wb, void *p, size_t i, uint64_t v) {
  if (wb == 8) ((uint64_t *)p)[i] = v;
  else if (wb == 4) ((uint32_t *)p)[i] = (uint32_t)v;
  else ((uint16_t *)p)[i] = (uint16_t)v;
}
static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return p ? nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream) : NFLHIP_OK; }

static int toy(nflhip_ctx *ctx, void *out, const void *in, size_t batch, size_t ks, uint64_t t, int flags, int ntt, int device_ptrs, void *stream) {
  if (!ctx) return NFLHIP_ERR_INVALID;
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8;
  if (ks == 0 || ks >= nm || t == 0 || (t >> (8 * wb - 3)) || (flags & ~(NFLHIP_SCALE_ROUND_FLOOR | NFLHIP_SCALE_ROUND_KEEP | NFLHIP_SCALE_ROUND_TWO_PASS)))
    return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const int keep = (flags & NFLHIP_SCALE_ROUND_KEEP) != 0;
  const size_t orows = keep ? nm - ks : ks;
  if (device_ptrs) {
    int rc = own(ctx, in, batch * nm * n * wb, stream);
    if (!rc) rc = own(ctx, out, batch * orows * n * wb, stream);
    if (rc) return rc;
  }
  for (size_t b = 0; b < batch; ++b) {
    const char *x = (const char *)in + b * nm * n * wb;
    char *o = (char *)out + b * orows * n * wb;
    for (size_t c = 0; c < n; ++c) {
      uint64_t h = mixw(mixw(mixw(0x5ca1e, t), (uint64_t)(ks * 8 + (size_t)(ntt ? 4 : 0) + (size_t)(flags & NFLHIP_SCALE_ROUND_FLOOR ? 2 : 0) + (size_t)keep)), nm);
      for (size_t r = 0; r < nm; ++r) h = mixw(h, ldw(wb, x, r * n + c));   /* (the plans give the same words) */
      for (size_t j = 0; j < orows; ++j) stw(wb, o, j * n + c, mixw(h, j + 7) >> 9);
    }
  }
  return NFLHIP_OK;
}

int nflhip_scale_round_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  return toy(ctx, d_out, d_in, batch, ks, t, flags, 0, 1, stream);
}
int nflhip_scale_round(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags) {
  return toy(ctx, h_out, h_in, batch, ks, t, flags, 0, 0, NULL);
}
int nflhip_scale_round_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  return toy(ctx, d_out, d_in, batch, ks, t, flags, 1, 1, stream);
}
int nflhip_scale_round_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags) {
  return toy(ctx, h_out, h_in, batch, ks, t, flags, 1, 0, NULL);
}

/* the four steps of the definition: embed, base-extend (centred), tensor product on nmoduli rows, scale-round of each component */
static int toy_bfv(nflhip_ctx *ctx, void *o0, void *o1, void *o2, const void *a0, const void *a1, const void *b0, const void *b1, size_t batch, size_t ks,
                   uint64_t t, int flags, int device_ptrs, void *stream) {
  if (!ctx) return NFLHIP_ERR_INVALID;
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, row = n * wb;
  if (ks == 0 || ks >= nm || t == 0 || (t >> (8 * wb - 3)) || (flags & ~(NFLHIP_SCALE_ROUND_FLOOR | NFLHIP_SCALE_ROUND_TWO_PASS)) || !b0 != !b1)
    return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  const size_t ib = batch * ks * row, pb = batch * nm * row, nin = b0 ? 4 : 2;
  const void *const ins[4] = {a0, a1, b0, b1};
  void *const outs[3] = {o0, o1, o2};
  int rc = NFLHIP_OK;
  if (device_ptrs) {
    for (size_t k = 0; k < nin && !rc; ++k) rc = own(ctx, ins[k], ib, stream);
    for (size_t k = 0; k < 3 && !rc; ++k) rc = own(ctx, outs[k], ib, stream);
    if (rc) return rc;
  }
  char *E = (char *)calloc(7 * pb + 3 * ib, 1), *T = E + 4 * pb, *R = T + 3 * pb;
  if (!E) return NFLHIP_ERR_NOMEM;
  for (size_t k = 0; k < nin && !rc; ++k) {
    for (size_t b = 0; b < batch; ++b) memcpy(E + k * pb + b * nm * row, (const char *)ins[k] + b * ks * row, ks * row);
    rc = nflhip_baseconv_ntt(ctx, E + k * pb, E + k * pb, batch, 0, ks, 0, nm, NFLHIP_BASECONV_CENTERED);
  }
  if (!rc) rc = nflhip_tensor_ntt(ctx, T, T + pb, T + 2 * pb, E, E + pb, b0 ? E + 2 * pb : NULL, b0 ? E + 3 * pb : NULL, batch, nm, 0);
  for (size_t k = 0; k < 3 && !rc; ++k) rc = nflhip_scale_round_ntt(ctx, R + k * ib, T + k * pb, batch, ks, t, flags);
  for (size_t k = 0; k < 3 && !rc; ++k) memcpy(outs[k], R + k * ib, ib);   /* (an output may be an input) */
  free(E);
  return rc;
}
int nflhip_bfv_tensor_ntt_dev(nflhip_ctx *ctx, void *d_out0, void *d_out1, void *d_out2, const void *d_a0, const void *d_a1, const void *d_b0,
                              const void *d_b1, size_t batch, size_t ks, uint64_t t, int flags, void *stream) {
  return toy_bfv(ctx, d_out0, d_out1, d_out2, d_a0, d_a1, d_b0, d_b1, batch, ks, t, flags, 1, stream);
}
int nflhip_bfv_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0,
                          const void *h_b1, size_t batch, size_t ks, uint64_t t, int flags) {
  return toy_bfv(ctx, h_out0, h_out1, h_out2, h_a0, h_a1, h_b0, h_b1, batch, ks, t, flags, 0, NULL);
}
