// table_types.h -- the record types of the per-context device tables, shared by the host code that computes them
// (host_tables.cpp) and the kernels that read them (kernels.h).  No HIP header: this compiles with the plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nflhip {

// Per-modulus device constants (engine layout; derived from params<T>::P,
// primitive_roots, invkMaxPolyDegree -- reference params.hpp -- by host_tables.cpp twiddles_and_modconst).
template <typename T> struct ModConst {
  T p;          // modulus
  T p2;         // 2p
  T mu;         // floor(2^(2W-4)/p): Barrett constant for exact x*y mod p
  T ninv;       // n^-1 mod p                       (core.hpp:664-665)
  T ninv_sh;    // Shoup companion of ninv
  T w1ninv;     // psi_br[1] * n^-1 mod p (last inverse stage, merged scale)
  T w1ninv_sh;  // its Shoup companion
  T beta;       // 2^64 mod p (CRT project, Horner step)
  T beta_sh;    // its Shoup companion
  T yinv;       // (Q/p)^-1 mod p (CRT lift)         (gmp.hpp:141-147)
  T yinv_sh;    // its Shoup companion
  T mask;       // 2^(floor(log2 p)+1) - 1           (core.hpp:165-166)
  T delta;      // 2^(W-2) - p: the primes are 2^(W-2) - c*2*kMax + 1 (params.hpp:20,54,96)
  T mu2;        // floor(2^(2W-3)/p): Barrett constant for lazily reduced operands (< 2^(W-2) + 3*delta)
};

// Per-kept-row constants of the RNS rescale by the LAST modulus q = p_(nm-1) (kernels_rescale.hip): row i < nm - 1
template <typename T> struct alignas(4 * sizeof(T)) RescConst {
  T qinv;     // q^-1 mod p_i
  T qinv_sh;  // its Shoup companion
  T h;        // (q - 1) / 2, below every p_i (the moduli of a limb width have one bit length)
  T p;        // p_i again, so that a kept row costs one 4-word record
};

// Twiddle pair as stored on the device: psi^bitrev(k) and its Shoup companion.
template <typename T> struct alignas(2 * sizeof(T)) Tw {
  T w, wp;
};

}  // namespace nflhip
