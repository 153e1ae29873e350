"""numpy restatement of the Galois automorphisms sigma_k : a(X) -> a(X^k) mod (X^n + 1), k odd (include/nflhip.h), on
[..., nmoduli, degree] word arrays -- what tests/test_automorphism_cpu.py and tests/test_gpu_automorphism.py check against."""
import numpy as np


def rev(x, logn):
    """log2(n)-bit reversal of every entry of an integer array"""
    x = np.asarray(x, dtype=np.int64)
    r = np.zeros_like(x)
    for b in range(logn):
        r |= ((x >> b) & 1) << (logn - 1 - b)
    return r


def sigma_coeff(a, k, P):
    """coefficient form: for i in [0, n), e = i k mod 2n; out[e] = in[i] when e < n, else out[e - n] = (p - in[i]) mod p"""
    n = a.shape[-1]
    k %= 2 * n
    e = (np.arange(n, dtype=np.int64) * k) % (2 * n)
    lo = e < n
    out = np.empty_like(a)
    out[..., e[lo]] = a[..., lo]
    p = np.asarray([int(x) for x in P], dtype=np.uint64).astype(a.dtype).reshape(-1, 1)
    x = a[..., ~lo]
    out[..., e[~lo] - n] = np.where(x == 0, x, (p - x).astype(a.dtype))
    return out


def ntt_source(n, k):
    """j' for every slot j of the NTT form (nflhip_ntt_fwd_dev's order): 2 rev(j') + 1 = k (2 rev(j) + 1) mod 2n"""
    logn = n.bit_length() - 1
    j = np.arange(n, dtype=np.int64)
    t = (k % (2 * n)) * (2 * rev(j, logn) + 1) % (2 * n)
    return rev((t - 1) // 2, logn)


def sigma_ntt(a, k):
    """NTT form: out[j] = in[j'], the stored words unchanged"""
    return a[..., ntt_source(a.shape[-1], k)]
