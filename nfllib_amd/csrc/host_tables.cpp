// host_tables.cpp -- every per-context table (DevTables, kernels.h) computed on the host, once per context, from
// params<T>::P / primitive_roots / invkMaxPolyDegree.  Plain host arithmetic: no HIP, no context; api.hip uploads the bytes.
#include "host_tables.h"

#include "../../include/nflhip.h"
#include "table_types.h"

namespace nflhip {
namespace {

typedef unsigned __int128 u128;
typedef HostTables::Bytes Bytes;

inline uint64_t mulmod_h(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((u128)a * b % p); }
uint64_t powmod_h(uint64_t a, uint64_t e, uint64_t p) {
  uint64_t r = 1 % p;
  a %= p;
  while (e) {
    if (e & 1) r = mulmod_h(r, a, p);
    a = mulmod_h(a, a, p);
    e >>= 1;
  }
  return r;
}
inline uint64_t shoup_h(uint64_t w, uint64_t p, int wb) { return (uint64_t)((((u128)w) << wb) / p); }
unsigned bitrev_h(unsigned k, int bits) {
  unsigned r = 0;
  for (int i = 0; i < bits; ++i) {
    r = (r << 1) | (k & 1u);
    k >>= 1;
  }
  return r;
}

// little-endian multi-limb helpers for the CRT constants (gmp.hpp:113-155)
typedef std::vector<uint64_t> Big;
void big_trim(Big &a) { while (!a.empty() && a.back() == 0) a.pop_back(); }
Big big_mul_u64(const Big &a, uint64_t w) {
  Big r(a.size() + 1, 0);
  u128 c = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    c += (u128)a[i] * w;
    r[i] = (uint64_t)c;
    c >>= 64;
  }
  r[a.size()] = (uint64_t)c;
  big_trim(r);
  return r;
}
uint64_t big_divrem_u64(const Big &a, uint64_t d, Big *q) {
  Big out(a.size(), 0);
  u128 r = 0;
  for (size_t k = a.size(); k-- > 0;) {
    r = (r << 64) | a[k];
    out[k] = (uint64_t)(r / d);
    r %= d;
  }
  big_trim(out);
  if (q) *q = out;
  return (uint64_t)r;
}
size_t big_bits(const Big &a) {
  if (a.empty()) return 0;
  size_t b = 0;
  uint64_t t = a.back();
  while (t) { ++b; t >>= 1; }
  return (a.size() - 1) * 64 + b;
}
Big big_shl(const Big &a, int k, size_t limbs) {
  Big r(limbs, 0);
  for (size_t i = 0; i < a.size() && i < limbs; ++i) {
    r[i] |= a[i] << k;
    if (k && i + 1 < limbs) r[i + 1] |= a[i] >> (64 - k);
  }
  return r;
}

template <typename V> Bytes to_bytes(const std::vector<V> &v) {
  const unsigned char *b = (const unsigned char *)v.data();
  return Bytes(b, b + v.size() * sizeof(V));
}

int invalid(std::string *err, const char *msg) {
  *err = msg;
  return NFLHIP_ERR_INVALID;
}

// fewest moduli for which the lift runs as an int8 GEMM on the matrix cores (kernels_crt_mfma.hip).  Its cost hardly depends on
// the modulus count (the tile is always 32 modulus slots x 256 columns: 0.48 ms at 12 moduli, 0.75 ms at 30 for 4 Mi
// coefficients), the VALU kernels of kernels_crt.hip grow with its square (0.24 ms at 12, 0.56 at 20, 0.76 at 24, 1.19 at 30):
// they cross between 20 and 21.  The projection's VALU kernels take a second launch beyond 16 residues: 0.40 ms at 16, 0.61 at 18
// against the GEMM's 0.40 / 0.43 -- it takes over at 17 (same-box sweeps in profiles/r04_crt_mfma.txt)
#ifndef NFLHIP_CRT_MFMA_MIN_NM
#define NFLHIP_CRT_MFMA_MIN_NM 21
#endif
#ifndef NFLHIP_CRT_MFMA_PROJ_MIN_NM
#define NFLHIP_CRT_MFMA_PROJ_MIN_NM 17
#endif

const size_t kStride = 36;  // fixed, zero-padded row stride of the device CRT tables

struct CrtBase {
  Big Q;                       // the moduli product
  std::vector<Big> quot;       // Q / p_cm            (mpz_divexact)
  std::vector<uint64_t> yinv;  // (Q/p_cm)^-1 mod p_cm (mpz_invert)
  bool ok;                     // the register-resident lift's tables hold a coefficient
};

// CRT constants
CrtBase crt_constants(HostTables &h) {
  const size_t nm = h.P.size();
  CrtBase c;
  c.Q = Big(1, 1);
  for (size_t cm = 0; cm < nm; ++cm) c.Q = big_mul_u64(c.Q, h.P[cm]);
  const Big &Q = c.Q;
  h.crt_L = (big_bits(Q) + 63) / 64;
  h.crt_Lacc = h.crt_L + 1;
  const size_t Lacc = h.crt_Lacc;
  h.Q = Q;
  h.Q.resize(h.crt_L, 0);
  h.crt_Q0 = Q.empty() ? 0 : Q[0];
  c.ok = Lacc <= kStride;  // beyond that crt_lift reports NFLHIP_ERR_UNSUPPORTED, the transforms still work
  std::vector<uint64_t> qhat(nm * kStride, 0), qsh(6 * kStride, 0);
  c.quot.resize(nm);
  c.yinv.assign(nm, 0);
  h.lifting.resize(nm);
  for (size_t cm = 0; cm < nm; ++cm) {
    Big &quot = c.quot[cm];
    big_divrem_u64(Q, h.P[cm], &quot);
    const uint64_t qmod = big_divrem_u64(quot, h.P[cm], nullptr);
    c.yinv[cm] = powmod_h(qmod, h.P[cm] - 2, h.P[cm]);
    for (size_t k = 0; c.ok && k < quot.size(); ++k) qhat[cm * kStride + k] = quot[k];
    h.lifting[cm] = big_mul_u64(quot, c.yinv[cm]);         // lifting_integers[cm] (gmp.hpp:149-150)
  }
  for (int k = 0; c.ok && k < 6; ++k) {
    Big sh = big_shl(Q, k, Lacc);
    for (size_t i = 0; i < Lacc; ++i) qsh[k * kStride + i] = sh[i];
  }
  h.qhat = to_bytes(qhat);
  h.qsh = to_bytes(qsh);
  // beyond the register-resident lift kernels (nm > 32 or more limbs than their tables hold): limb-serial tables
  if (!c.ok || nm > 32) {
    const int Lw = (int)h.crt_L + 2;
    int nsh = 0;
    while ((((size_t)1) << nsh) <= nm) ++nsh;  // 2^nsh > nm >= S / Q
    std::vector<uint64_t> qhat_w(nm * (size_t)Lw, 0), qsh_w((size_t)nsh * Lw, 0);
    for (size_t cm = 0; cm < nm; ++cm)
      for (size_t k = 0; k < c.quot[cm].size(); ++k) qhat_w[cm * Lw + k] = c.quot[cm][k];
    for (int k = 0; k < nsh; ++k) {
      Big sh = big_shl(Q, k, (size_t)Lw);
      for (int i = 0; i < Lw; ++i) qsh_w[(size_t)k * Lw + i] = sh[i];
    }
    h.qhat_w = to_bytes(qhat_w);
    h.qsh_w = to_bytes(qsh_w);
    h.crt_Lw = Lw;
    h.crt_nsh = nsh;
  }
  return c;
}

// carry-free multiply-accumulate tables for 64-bit limbs (kernels_crt.hip)
void carry_free_parts(HostTables &h, const CrtBase &c) {
  const size_t nm = h.P.size(), L = h.crt_L, S32 = 2 * kStride;
  std::vector<uint32_t> qparts(nm * 3 * S32, 0);
  for (size_t cm = 0; cm < nm; ++cm)
    for (int j = 0; j < 3; ++j) {
      const Big sh = big_shl(c.quot[cm], 21 * j, L);  // (Q/p) << 42 < Q: fits L words
      for (size_t i = 0; i < L; ++i) {
        qparts[(cm * 3 + j) * S32 + 2 * i] = (uint32_t)sh[i];
        qparts[(cm * 3 + j) * S32 + 2 * i + 1] = (uint32_t)(sh[i] >> 32);
      }
    }
  h.proj_K = (int)(2 * L + 2);
  const size_t nmS = (nm + 3) & ~(size_t)3;  // row stride: zero padded, the kernel runs without guards
  std::vector<uint32_t> bparts((size_t)h.proj_K * 2 * 3 * nmS, 0);
  for (size_t cm = 0; cm < nm; ++cm) {
    const uint64_t p = h.P[cm], two32 = (((uint64_t)1) << 32) % p;
    uint64_t cur = 1 % p;  // 2^(32 t) mod p, t = 2k + half
    for (size_t t = 0; t < (size_t)h.proj_K * 2; ++t) {
      uint32_t *e = &bparts[t * 3 * nmS + cm];
      e[0] = (uint32_t)(cur & 0x1fffff);
      e[nmS] = (uint32_t)((cur >> 21) & 0x1fffff);
      e[2 * nmS] = (uint32_t)(cur >> 42);
      cur = mulmod_h(cur, two32, p);
    }
  }
  h.qparts = to_bytes(qparts);
  h.bparts = to_bytes(bparts);
  // Q / 2^(32 max(2L - 3, 0)) from its top words (the kernel divides the top five 32-bit digits of the sum by it)
  long double qt = 0.0L;
  for (size_t k = L; k-- > 0;) qt = qt * 18446744073709551616.0L + (long double)c.Q[k];
  for (long w = 0; w < 2 * (long)L - 3; ++w) qt /= 4294967296.0L;
  h.inv_qtop = (double)(1.0L / qt);
}

// the lift as an int8 GEMM (kernels_crt_mfma.hip): balanced base-256 digits of Q/p_cm, laid out as the B operand of
// v_mfma_i32_32x32x32_i8 -- K-step s, N-tile t, lane (column j = lane & 31, half h = lane >> 5), byte e:
// modulus slot cm = 4 s + 2 h + (e >> 3), digit of y a = e & 7, column k = 8 j + t  ->  digit k - a of Q/p_cm.
// Slot 31 is the quotient row: the digits of Q itself against the single digit "-floor(S / Q)" (a = 0).
void lift_fragments(HostTables &h, const CrtBase &c) {
  const size_t nm = h.P.size(), ND = 264;
  std::vector<int8_t> dig(32 * ND, 0);
  for (size_t cm = 0; cm < 32; ++cm) {
    if (cm >= nm && cm != 31) continue;
    const Big &quot = cm < nm ? c.quot[cm] : c.Q;  // (with 32 moduli the slot is the 32nd modulus's and the kernel subtracts the quotient itself)
    int carry = 0;
    for (size_t k = 0; k < ND; ++k) {
      const size_t w = k / 8;
      int v = (w < quot.size() ? (int)((quot[w] >> (8 * (k % 8))) & 0xff) : 0) + carry;
      carry = 0;
      if (v >= 128) { v -= 256; carry = 1; }
      dig[cm * ND + k] = (int8_t)v;
    }
  }
  std::vector<int8_t> bfrag((size_t)8 * 8 * 64 * 16, 0);
  for (int st = 0; st < 8; ++st)
    for (int t = 0; t < 8; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 16; ++e) {
          const int cm = 4 * st + 2 * (lane >> 5) + (e >> 3), a = e & 7, k = 8 * (lane & 31) + t;
          if (k >= a && ((size_t)cm < nm || a == 0)) bfrag[(((size_t)st * 8 + t) * 64 + lane) * 16 + e] = dig[cm * ND + (k - a)];
        }
  h.crt_bfrag = to_bytes(bfrag);
}

// the projection as an int8 GEMM (kernels_crt_mfma.hip): balanced base-256 digits of 256^k mod p_cm, k < 256, as the B
// operand -- K-step s, N-tile t = digit, lane (cm = lane & 31, half h = lane >> 5), byte e: k = 32 s + 16 h + e -- and the
// per-residue constant 2^18 p + 128 sum_k (256^k mod p) (the input bytes enter as a - 128; the sum is made non-negative)
void projection_fragments(HostTables &h) {
  const size_t nm = h.P.size();
  std::vector<int8_t> dig((size_t)32 * 256 * 8, 0);   // [cm][k][digit]
  std::vector<uint64_t> coff(32 * 2, 0), c2048(32 * 2, 0);
  for (size_t cm = 0; cm < nm; ++cm) {
    const uint64_t p = h.P[cm];
    uint64_t cur = 1 % p;
    __int128 colsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 256; ++k) {
      int carry = 0;
      for (int b = 0; b < 8; ++b) {
        int v = (int)((cur >> (8 * b)) & 0xff) + carry;
        carry = 0;
        if (v >= 128 && b < 7) { v -= 256; carry = 1; }   // (the top digit of a 62-bit value is below 65: no carry out)
        dig[(cm * 256 + k) * 8 + b] = (int8_t)v;
        colsum[b] += 128 * v;
      }
      cur = mulmod_h(cur, 256 % p, p);
    }
    __int128 off = (__int128)p << 18;
    for (int b = 0; b < 8; ++b) off += colsum[b] * ((__int128)1 << (8 * b));
    coff[2 * cm] = (uint64_t)off;
    coff[2 * cm + 1] = (uint64_t)((unsigned __int128)off >> 64);
    c2048[2 * cm] = powmod_h(2 % p, 2048, p);
    c2048[2 * cm + 1] = shoup_h(c2048[2 * cm], p, 64);
  }
  std::vector<int8_t> bproj((size_t)8 * 8 * 64 * 16, 0);
  for (int st = 0; st < 8; ++st)
    for (int t = 0; t < 8; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 16; ++e) {
          const size_t cm = lane & 31;
          const int k = 32 * st + 16 * (lane >> 5) + e;
          if (cm < nm) bproj[(((size_t)st * 8 + t) * 64 + lane) * 16 + e] = dig[(cm * 256 + k) * 8 + t];
        }
  h.crt_bproj = to_bytes(bproj);
  h.crt_coff = to_bytes(coff);
  h.crt_c2048 = to_bytes(c2048);
}

// twiddles + per-modulus constants
template <typename T>
int twiddles_and_modconst(HostTables &h, size_t n, int cyclic, int kmax_log2, const std::vector<uint64_t> &yinv,
                          std::vector<Tw<T>> &psi, std::vector<ModConst<T>> &mc, std::string *err) {
  const int wb = 8 * (int)sizeof(T);
  const size_t nm = h.P.size();
  int logn = 0;
  while ((((size_t)1) << logn) < n) ++logn;
  psi.resize(nm * n);
  mc.resize(nm);
  for (size_t cm = 0; cm < nm; ++cm) {
    const uint64_t p = h.P[cm];
    // phi: primitive 2n-th root from the primitive 2*kMax-th root (core.hpp:640-645)
    uint64_t phi = h.roots[cm];
    for (int i = 0; i < kmax_log2 - logn; ++i) phi = mulmod_h(phi, phi, p);
    if (powmod_h(phi, n, p) != p - 1) return invalid(err, "primitive root has the wrong order");
    h.phi.push_back(phi);
    const uint64_t base = cyclic == 2 ? powmod_h(phi, 2 * n - 1, p) : phi;  // phi^-1 for the inverse tables
    std::vector<uint64_t> pw(n);
    uint64_t cur = 1;
    for (size_t i = 0; i < n; ++i) {
      pw[i] = cur;
      cur = mulmod_h(cur, base, p);
    }
    Tw<T> *tw = psi.data() + cm * n;
    for (size_t k = 0; k < n; ++k) {
      // negacyclic: psi_br[k] = phi^bitrev(k).  With k = m + j (m = the power of two <= k: stage with m blocks, block j)
      // that exponent is (n/2m)(2 brev_m(j) + 1); the cyclic transform core::ntt computes needs omega^((n/2m) brev_m(j))
      // = phi^(bitrev(k) - n/2m) in the same slot, so every forward kernel runs it unchanged on this table.
      size_t e = bitrev_h((unsigned)k, logn);
      if (cyclic && k > 0) {
        size_t m = 1;
        while (2 * m <= k) m *= 2;
        e -= n / (2 * m);
      }
      const uint64_t w = pw[e];
      tw[k].w = (T)w;
      tw[k].wp = (T)shoup_h(w, p, wb);
    }
    ModConst<T> &m = mc[cm];
    m.p = (T)p;
    m.p2 = (T)(2 * p);
    m.mu = (T)((((u128)1) << (2 * wb - 4)) / p);
    // n^-1 = kMax^-1 * (kMax/n) (core.hpp:664-665)
    const uint64_t ninv = mulmod_h(h.invk[cm], (((uint64_t)1) << kmax_log2) / n, p);
    if (mulmod_h(ninv, n % p, p) != 1 % p) return invalid(err, "invkMaxPolyDegree is not the inverse");
    m.ninv = (T)ninv;
    m.ninv_sh = (T)shoup_h(ninv, p, wb);
    const uint64_t w1 = n >= 2 ? (uint64_t)tw[1].w : 1;
    const uint64_t w1n = mulmod_h(w1, ninv, p);
    m.w1ninv = (T)w1n;
    m.w1ninv_sh = (T)shoup_h(w1n, p, wb);
    const uint64_t beta = (uint64_t)((((u128)1) << 64) % p);
    m.beta = (T)beta;
    m.beta_sh = (T)shoup_h(beta, p, wb);
    m.yinv = (T)yinv[cm];
    m.yinv_sh = (T)shoup_h(yinv[cm], p, wb);
    int bits = 0;
    while (bits < wb && (((u128)1) << bits) <= (u128)p) ++bits;
    m.mask = (T)(bits >= 64 ? ~(uint64_t)0 : ((((uint64_t)1) << bits) - 1));
    m.delta = (T)((((uint64_t)1) << (wb - 2)) - p);
    m.mu2 = (T)((((u128)1) << (2 * wb - 3)) / p);
  }
  return NFLHIP_OK;
}

// the generated 64-bit kernels read the last four stages (indices n/16 .. n-1) LANE-MAJOR: stage logn-4+s transposed
// from [(u << s) + g] to [g (n/16) + u], so that the 64 lanes of a wave fetch consecutive records
// (tools/gen_polymul_asm.py tw_base_lm); indices below n/16 are shared with the natural table
template <typename T> std::vector<Tw<T>> lane_major(const std::vector<Tw<T>> &psi, size_t n, size_t nm) {
  std::vector<Tw<T>> lm(psi);
  const size_t m = n >> 4;
  for (size_t cm = 0; cm < nm; ++cm)
    for (int s = 0; s < 4; ++s) {
      const Tw<T> *src = psi.data() + cm * n + (m << s);
      Tw<T> *dst = lm.data() + cm * n + (m << s);
      for (size_t u = 0; u < m; ++u)
        for (size_t g = 0; g < ((size_t)1 << s); ++g) dst[g * m + u] = src[(u << s) + g];
    }
  return lm;
}

// The records the products on incomplete transforms read: the inverse undoes logn - level stages, so the scale folded into its
// last stage is (n / 2^level)^-1, in the n^-1 fields.
// 32-bit limbs, rows of 1024 / 2048 / 4096 words (tools/gen_row1024_u32_asm.py base_mul, level 2 only): floor(2^62 / p) - 2^32
// in the mu field.
// 64-bit limbs, the metric product (nflhip_polymul4096i{1,2}_asm): the base multiplication reduces sums below 2^127 with
// floor(2^127 / p) = 2^65 + m, m < 2^35 (delta < 2^32), handed over in the mu2 field
template <typename T> std::vector<ModConst<T>> incomplete_records(const std::vector<ModConst<T>> &mc, int level) {
  const int wb = 8 * (int)sizeof(T);
  std::vector<ModConst<T>> mi(mc);
  for (size_t cm = 0; cm < mc.size(); ++cm) {
    const uint64_t p = (uint64_t)mc[cm].p;
    const uint64_t ng = mulmod_h((uint64_t)mc[cm].ninv, (uint64_t)1 << level, p);
    const uint64_t wg = mulmod_h((uint64_t)mc[cm].w1ninv, (uint64_t)1 << level, p);
    mi[cm].ninv = (T)ng;
    mi[cm].ninv_sh = (T)shoup_h(ng, p, wb);
    mi[cm].w1ninv = (T)wg;
    mi[cm].w1ninv_sh = (T)shoup_h(wg, p, wb);
    if (wb == 32) mi[cm].mu = (T)(uint64_t)(((((u128)1) << 62) / p) - (((u128)1) << 32));
    else mi[cm].mu2 = (T)(uint64_t)(((((u128)1) << 127) / p) - (((u128)1) << 65));
  }
  return mi;
}

// RNS rescale by the last modulus q (kernels_rescale.hip): q^-1 mod p_i, its Shoup companion and h = (q - 1) / 2 per kept row
template <typename T> std::vector<RescConst<T>> rescale_records(const std::vector<uint64_t> &P) {
  const int wb = 8 * (int)sizeof(T);
  const size_t nm = P.size();
  const uint64_t q = P[nm - 1];
  std::vector<RescConst<T>> resc(nm - 1);
  for (size_t cm = 0; cm + 1 < nm; ++cm) {
    const uint64_t p = P[cm];
    if (q % p == 0) return {};  // (a chain that repeats its last modulus has no rescale: the entry reports it)
    const uint64_t qinv = powmod_h(q % p, p - 2, p);
    resc[cm].qinv = (T)qinv;
    resc[cm].qinv_sh = (T)shoup_h(qinv, p, wb);
    resc[cm].h = (T)((q - 1) / 2);
    resc[cm].p = (T)p;
  }
  return resc;
}

template <typename T>
int build(HostTables &h, size_t n, size_t nm, int cyclic, int kmax_log2, const T *P, const T *roots, const T *invk, std::string *err) {
  const int wb = 8 * (int)sizeof(T);
  // moduli sanity: the engine relies on p being 2 bits below the word (params.hpp:27-28,61-62,104-105)
  for (size_t cm = 0; cm < nm; ++cm) {
    const uint64_t p = P[cm];
    if (p < 3 || (p >> (wb - 2)) != 0 || (p >> (wb - 3)) == 0) return invalid(err, "modulus is not (word-2) bits long");
    h.P.push_back(p);
    h.roots.push_back(roots[cm]);
    h.invk.push_back(invk[cm]);
    if (((((uint64_t)1) << (wb - 2)) - p) >> 32) h.small_delta = 0;
    if (h.small_delta) h.nm_small = (int)cm + 1;
  }
  const CrtBase crt = crt_constants(h);
  if (wb == 64 && crt.ok && nm <= 32) carry_free_parts(h, crt);
  if (wb == 64 && crt.ok && nm >= NFLHIP_CRT_MFMA_MIN_NM && nm <= 32 && h.crt_L >= 4 && h.crt_L <= 31) lift_fragments(h, crt);
  if (wb == 64 && h.small_delta && nm >= NFLHIP_CRT_MFMA_PROJ_MIN_NM && nm <= 32) projection_fragments(h);

  std::vector<Tw<T>> psi;
  std::vector<ModConst<T>> mc;
  const int rc = twiddles_and_modconst(h, n, cyclic, kmax_log2, crt.yinv, psi, mc, err);
  if (rc) return rc;
  h.psi = to_bytes(psi);
  h.mc = to_bytes(mc);
  if (wb == 64 && n >= 4096) h.psi_lm = to_bytes(lane_major(psi, n, nm));
  if (nm >= 2 && !cyclic) h.resc = to_bytes(rescale_records<T>(h.P));
  if (wb == 32 && n >= 1024 && n <= 4096 && !cyclic) h.mc_inc[1] = to_bytes(incomplete_records(mc, 2));
  if (wb == 64 && n >= 1024 && !cyclic && (h.small_delta || (n == 4096 && h.nm_small > 0)))
    for (int level = 1; level <= 2; ++level) h.mc_inc[level - 1] = to_bytes(incomplete_records(mc, level));
  return NFLHIP_OK;
}

}  // namespace

int build_host_tables(int limb_bits, size_t n, size_t nm, int cyclic, int kmax_log2, const void *P, const void *roots,
                      const void *invk, HostTables *out, std::string *err) {
  *out = HostTables();
  if (limb_bits == 16) return build(*out, n, nm, cyclic, kmax_log2, (const uint16_t *)P, (const uint16_t *)roots, (const uint16_t *)invk, err);
  if (limb_bits == 32) return build(*out, n, nm, cyclic, kmax_log2, (const uint32_t *)P, (const uint32_t *)roots, (const uint32_t *)invk, err);
  return build(*out, n, nm, cyclic, kmax_log2, (const uint64_t *)P, (const uint64_t *)roots, (const uint64_t *)invk, err);
}

// RNS base conversion: the record of one pair of row ranges (host_tables.h).  (Q/p_i) mod p_j from prefix and suffix products of the
// source moduli mod p_j, so the cost is ks kd multiplications; inverses by Fermat (the moduli are prime).
int build_baseconv_record(int limb_bits, const std::vector<uint64_t> &P, size_t s0, size_t ks, size_t d0, size_t kd, bool moddown,
                          std::vector<uint64_t> *out, std::string *err) {
  const size_t nm = P.size();
  if (ks == 0 || kd == 0 || s0 >= nm || ks > nm - s0 || d0 >= nm || kd > nm - d0) return invalid(err, "baseconv: a row range is empty or outside the context");
  if (moddown && (s0 + ks != nm || d0 != 0 || kd != s0)) return invalid(err, "moddown: the dropped rows are the last k, the kept rows the others");
  out->assign(baseconv_record_words(ks, kd), 0);
  uint64_t *src = out->data(), *dst = src + 4 * ks, *c = dst + 8 * kd;
  std::vector<uint64_t> pre(ks + 1), suf(ks + 1);
  // products of the source moduli mod p, without the i-th: pre[i] suf[i + 1]
  auto products = [&](uint64_t p) {
    pre[0] = suf[ks] = 1 % p;
    for (size_t i = 0; i < ks; ++i) pre[i + 1] = mulmod_h(pre[i], P[s0 + i] % p, p);
    for (size_t i = ks; i-- > 0;) suf[i] = mulmod_h(suf[i + 1], P[s0 + i] % p, p);
  };
  for (size_t i = 0; i < ks; ++i) {
    const uint64_t p = P[s0 + i];
    products(p);
    const uint64_t qi = mulmod_h(pre[i], suf[i + 1], p);  // (Q/p_i) mod p_i
    if (qi == 0) return invalid(err, "baseconv: a source modulus repeats");
    const uint64_t inv = powmod_h(qi, p - 2, p);
    src[4 * i] = inv;
    src[4 * i + 1] = shoup_h(inv, p, limb_bits);
    src[4 * i + 2] = p;
    src[4 * i + 3] = (uint64_t)((((u128)1) << (limb_bits == 64 ? 124 : 60)) / p);
  }
  for (size_t j = 0; j < kd; ++j) {
    const uint64_t p = P[d0 + j];
    products(p);
    const uint64_t Qj = pre[ks];
    dst[8 * j] = p;
    dst[8 * j + 1] = Qj;
    dst[8 * j + 2] = shoup_h(Qj, p, limb_bits);
    if (moddown) {
      if (Qj == 0) return invalid(err, "moddown: a kept modulus repeats a dropped one");
      const uint64_t inv = powmod_h(Qj, p - 2, p);
      dst[8 * j + 3] = inv;
      dst[8 * j + 4] = shoup_h(inv, p, limb_bits);
    }
    for (size_t i = 0; i < ks; ++i) c[j * ks + i] = mulmod_h(pre[i], suf[i + 1], p);
  }
  return NFLHIP_OK;
}

// Scale-and-round by t/Q: the two conversion records one behind the other (host_tables.h), the first one carrying t.
int build_scale_round_record(int limb_bits, const std::vector<uint64_t> &P, size_t ks, uint64_t t, std::vector<uint64_t> *out, std::string *err) {
  const size_t nm = P.size();
  if (ks == 0 || ks >= nm) return invalid(err, "scale_round: ks is out of range (1 to nmoduli - 1)");
  if (t == 0 || t >> (limb_bits - 3)) return invalid(err, "scale_round: t is out of range (1 to 2^(limb_bits - 3) - 1)");
  const size_t kd = nm - ks;
  std::vector<uint64_t> fwd, back;
  int rc = build_baseconv_record(limb_bits, P, 0, ks, ks, kd, false, &fwd, err);
  if (!rc) rc = build_baseconv_record(limb_bits, P, ks, kd, 0, ks, false, &back, err);
  if (rc) return rc;
  uint64_t *src = fwd.data(), *dst = src + 4 * ks;
  for (size_t i = 0; i < ks; ++i) {  // y_i = x_i (t (Q/p_i)^-1) mod p_i: t folded into the constant, the same words
    const uint64_t p = P[i], w = mulmod_h(src[4 * i], t % p, p);
    src[4 * i] = w;
    src[4 * i + 1] = shoup_h(w, p, limb_bits);
  }
  for (size_t j = 0; j < kd; ++j) {
    const uint64_t p = dst[8 * j], Qj = dst[8 * j + 1];
    if (Qj == 0) return invalid(err, "scale_round: a modulus of the rows D repeats one of the rows S");
    const uint64_t inv = powmod_h(Qj, p - 2, p);
    dst[8 * j + 3] = inv;
    dst[8 * j + 4] = shoup_h(inv, p, limb_bits);
    dst[8 * j + 5] = t % p;
    dst[8 * j + 6] = shoup_h(t % p, p, limb_bits);
  }
  *out = fwd;
  out->resize(scale_round_back_offset(ks, kd), 0);  // (the second record starts on 32 bytes, as a record of its own does)
  out->insert(out->end(), back.begin(), back.end());
  return NFLHIP_OK;
}

// the reference's own table layouts (poly.hpp:228-237), rebuilt on the host from phi: what a caller holding
// core::base sees.  Host arithmetic, once per request; the device never reads these.
std::vector<uint64_t> reference_table(uint64_t p, uint64_t phi, uint64_t invk, int kmax_log2, size_t n, int wb, int which) {
  const size_t words = (which == NFLHIP_TAB_OMEGAS || which == NFLHIP_TAB_INVOMEGAS) ? 2 * n : n;
  std::vector<uint64_t> v(words, 0);
  const uint64_t invphi = powmod_h(phi, 2 * n - 1, p);
  if (which == NFLHIP_TAB_PHIS || which == NFLHIP_TAB_SHOUPPHIS) {  // core.hpp:649-656
    uint64_t t = 1;
    for (size_t i = 0; i < n; ++i) {
      v[i] = which == NFLHIP_TAB_PHIS ? t : shoup_h(t, p, wb);
      t = mulmod_h(t, phi, p);
    }
  } else if (which == NFLHIP_TAB_INVPOLY_INVPHIS || which == NFLHIP_TAB_SHOUPINVPOLY_INVPHIS) {  // core.hpp:664-676
    uint64_t t = mulmod_h(invk, (((uint64_t)1) << kmax_log2) / n, p);
    for (size_t i = 0; i < n; ++i) {
      v[i] = which == NFLHIP_TAB_INVPOLY_INVPHIS ? t : shoup_h(t, p, wb);
      t = mulmod_h(t, invphi, p);
    }
  } else {  // core::prep_wtab, core.hpp:564-581: stage-concatenated powers, Shoup companions at offset n
    uint64_t wcur = which == NFLHIP_TAB_OMEGAS ? mulmod_h(phi, phi, p) : mulmod_h(invphi, invphi, p);
    size_t pos = 0;
    for (size_t K = n; K >= 2; K /= 2) {
      uint64_t wi = 1;
      for (size_t i = 0; i < K / 2; ++i, ++pos) {
        v[pos] = wi;
        v[n + pos] = shoup_h(wi, p, wb);
        wi = mulmod_h(wi, wcur, p);
      }
      wcur = mulmod_h(wcur, wcur, p);
    }
  }
  return v;
}

}  // namespace nflhip
