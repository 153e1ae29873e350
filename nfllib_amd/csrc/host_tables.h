// host_tables.h -- every per-context table, computed on the host (see host_tables.cpp).  No HIP: api.hip uploads the result.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace nflhip {

struct HostTables {
  typedef std::vector<unsigned char> Bytes;
  // the device tables, byte for byte as DevTables (kernels.h) describes them; an empty vector: the context has no such table
  Bytes psi, psi_lm, mc, mc_inc[2], resc;
  Bytes qhat, qsh, qparts, bparts, qhat_w, qsh_w;
  Bytes crt_bfrag, crt_bproj, crt_coff, crt_c2048;
  // the scalars of DevTables
  int proj_K = 0;
  double inv_qtop = 0;
  int crt_Lw = 0, crt_nsh = 0;
  // the shape facts the moduli decide (Shape, kernels.h)
  size_t crt_L = 0, crt_Lacc = 0;
  uint64_t crt_Q0 = 0;
  int small_delta = 1, nm_small = 0;
  // host copies the context keeps for introspection and for its child contexts
  std::vector<uint64_t> Q;                     // moduli_product limbs
  std::vector<std::vector<uint64_t>> lifting;  // lifting_integers[cm]
  std::vector<uint64_t> P, roots, invk, phi;   // params<T>::P / primitive_roots / invkMaxPolyDegree, phi = 2n-th root per modulus
};

// Fills *out for n = 2^k coefficients and nm moduli of limb_bits (16 / 32 / 64) bits: P, roots, invk are arrays of nm limbs of that
// width.  cyclic: 0 negacyclic tables, 1 / 2 cyclic over omega / omega^-1.  Returns NFLHIP_OK, or an NFLHIP_ERR_* code with *err set.
int build_host_tables(int limb_bits, size_t n, size_t nm, int cyclic, int kmax_log2, const void *P, const void *roots,
                      const void *invk, HostTables *out, std::string *err);

// RNS base conversion (kernels_baseconv.hip; include/nflhip.h "RNS base conversion"): the record of one pair of row ranges, source
// rows S = [s0, s0 + ks) and destination rows D = [d0, d0 + kd) of the moduli P (nm words of limb_bits bits each, as uint64_t), as
// 64-bit words whatever the limb width, Q = prod_{i in S} p_i:
//   [4 ks]    per source row i:       (Q/p_i)^-1 mod p_i, its Shoup companion floor(w 2^W / p_i), p_i, the 60-bit reciprocal
//                                     (floor(2^60 / p_i) for 16- / 32-bit limbs; floor(2^124 / p_i) = ModConst::mu for 64-bit limbs)
//   [8 kd]    per destination row j:  p_j, Q mod p_j, its Shoup companion, Q^-1 mod p_j, its Shoup companion (both 0 unless
//                                     `moddown`), three zero words
//   [kd][ks]  c_ij = (Q/p_i) mod p_j, destination-major
// moddown: S is the last ks rows, D the rows before them (s0 = nm - ks, d0 = 0, kd = nm - ks), and Q^-1 mod p_j must exist.
// Returns NFLHIP_OK, or NFLHIP_ERR_INVALID with *err set: a range outside [0, nm), an empty range, a repeated source modulus, or
// (moddown) a kept modulus that repeats a dropped one.
int build_baseconv_record(int limb_bits, const std::vector<uint64_t> &P, size_t s0, size_t ks, size_t d0, size_t kd, bool moddown,
                          std::vector<uint64_t> *out, std::string *err);
inline size_t baseconv_record_words(size_t ks, size_t kd) { return 4 * ks + 8 * kd + ks * kd; }

// Scale-and-round by t/Q (kernels_scale_round.hip; include/nflhip.h "BFV multiplication"): S = [0, ks), D = [ks, nm), kd = nm - ks.
// Two records of the layout above, one behind the other:
//   first   (S -> D), baseconv_record_words(ks, kd) words, with t folded in: a source row's constant is t (Q/p_i)^-1 mod p_i and its
//           Shoup companion; a destination row's words 3, 4 hold Q^-1 mod p_j and its companion, words 5, 6 t and its companion
//   second  (D -> S), from word scale_round_back_offset(ks, kd) on (the first record padded to 32 bytes), baseconv_record_words(kd, ks)
//           words, exactly build_baseconv_record(ks, kd, 0, ks, false): k_baseconv reads it
// Returns NFLHIP_OK, or NFLHIP_ERR_INVALID with *err set: ks outside [1, nm - 1], t outside [1, 2^(limb_bits - 3)), a repeated modulus.
inline size_t scale_round_back_offset(size_t ks, size_t kd) { return (baseconv_record_words(ks, kd) + 3) & ~(size_t)3; }
int build_scale_round_record(int limb_bits, const std::vector<uint64_t> &P, size_t ks, uint64_t t, std::vector<uint64_t> *out, std::string *err);

// nflhip_get_table, NFLHIP_TAB_PHIS .. NFLHIP_TAB_INVOMEGAS: one modulus's table in the reference's own layout (n words, 2 n for
// the two omega tables), each word below 2^limb_bits
std::vector<uint64_t> reference_table(uint64_t p, uint64_t phi, uint64_t invk, int kmax_log2, size_t n, int limb_bits, int which);

}  // namespace nflhip
