/* TEST INFRASTRUCTURE -- NOT A BACKEND.  Toy nflhip_baseconv_ntt_dev / nflhip_moddown_ntt_dev and their host variants over plain host
 * memory, linked INTO the program tests/cpp_baseconv_ntt/baseconv_ntt_main.cpp when it runs against the CPU stand-in of tests/cpp/mock
 * (whose generated versions of these entries only fail), next to tests/cpp_baseconv/toy_baseconv.c for the coefficient-form entries.
 * What they keep of the real entries is what the header layer relies on: a batched call equals a loop of single-polynomial calls, the
 * host variant equals the device variant, the layouts and strides, every source word read before a word of its position is written,
 * and -- through the stand-in's own device copy -- that every buffer belongs to the device of the context the call is made on.  The
 * arithmetic is a word-wise scramble, different from the coefficient-form toy's, so a call that reaches the wrong entry shows. */
#include <stdint.h>
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
/* the stand-in's device copy of a buffer onto itself: fails when [p, p + bytes) is not inside a buffer of ctx's device (host
 * arrays, which its registry does not know, pass) */
static int own(nflhip_ctx *ctx, const void *p, size_t bytes, void *stream) { return nflhip_memcpy_d2d(ctx, (void *)p, p, bytes, stream); }

static int toy(nflhip_ctx *ctx, void *out, const void *in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags, int down,
               void *stream) {
  const size_t n = nflhip_degree(ctx), nm = nflhip_nmoduli(ctx), wb = (size_t)nflhip_limb_bits(ctx) / 8, onm = down ? kd : nm;
  const int plan = flags & (NFLHIP_BASECONV_NTT_COMPOSED | NFLHIP_BASECONV_NTT_FUSED);
  if (ks == 0 || kd == 0 || s0 + ks > nm || d0 + kd > nm || (flags & ~(0x100 | plan)) || plan == (NFLHIP_BASECONV_NTT_COMPOSED | NFLHIP_BASECONV_NTT_FUSED))
    return NFLHIP_ERR_INVALID;
  if (batch == 0) return NFLHIP_OK;
  int rc = own(ctx, in, batch * nm * n * wb, stream);
  if (!rc) rc = own(ctx, out, batch * onm * n * wb, stream);
  if (rc) return rc;
  for (size_t b = 0; b < batch; ++b) {
    const char *x = (const char *)in + b * nm * n * wb;
    char *o = (char *)out + b * onm * n * wb;
    for (size_t c = 0; c < n; ++c) {
      uint64_t h = mixw(mixw(0xa77, (uint64_t)(flags & 0x100)), (uint64_t)(s0 * 1024 + ks));   /* (the plans give the same words) */
      for (size_t i = 0; i < ks; ++i) h = mixw(h, ldw(wb, x, (s0 + i) * n + c));
      for (size_t j = 0; j < kd; ++j) {
        const uint64_t xj = down ? ldw(wb, x, (d0 + j) * n + c) : 0;
        stw(wb, o, (d0 + j) * n + c, mixw(mixw(h, j + 3), xj) >> 9);
      }
    }
  }
  return NFLHIP_OK;
}

int nflhip_baseconv_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags,
                            void *stream) {
  return toy(ctx, d_out, d_in, batch, s0, ks, d0, kd, flags, 0, stream);
}
int nflhip_baseconv_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags) {
  if (h_out != h_in) memmove(h_out, h_in, batch * nflhip_degree(ctx) * nflhip_nmoduli(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8));
  return toy(ctx, h_out, h_out, batch, s0, ks, d0, kd, flags, 0, NULL);
}
int nflhip_moddown_ntt_dev(nflhip_ctx *ctx, void *d_out, const void *d_in, size_t batch, size_t k, int flags, void *stream) {
  const size_t nm = nflhip_nmoduli(ctx);
  if (k == 0 || k >= nm) return NFLHIP_ERR_INVALID;
  return toy(ctx, d_out, d_in, batch, nm - k, k, 0, nm - k, flags, 1, stream);
}
int nflhip_moddown_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags) {
  return nflhip_moddown_ntt_dev(ctx, h_out, h_in, batch, k, flags, NULL);
}

/* the host variants of the coefficient-form entries, over the toy device entries of tests/cpp_baseconv/toy_baseconv.c: nfl::poly
 * reaches them where the program compares the two forms */
int nflhip_baseconv(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags) {
  if (h_out != h_in) memmove(h_out, h_in, batch * nflhip_degree(ctx) * nflhip_nmoduli(ctx) * ((size_t)nflhip_limb_bits(ctx) / 8));
  return nflhip_baseconv_dev(ctx, h_out, h_out, batch, s0, ks, d0, kd, flags, NULL);
}
int nflhip_moddown(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags) {
  return nflhip_moddown_dev(ctx, h_out, h_in, batch, k, flags, NULL);
}
