"""Python-integer restatement of the RNS base conversion and the mod-down by the last k moduli (include/nflhip.h "RNS base
conversion") on [..., nmoduli, degree] word arrays -- what tests/test_baseconv_cpu.py and tests/test_gpu_baseconv.py check against.
Two independent statements: baseconv_rns / moddown_rns are the row formulas with the fixed-point correction v exactly as the
header defines it (they define the words bit for bit); baseconv_exact / moddown_exact go through the integer behind the residues
(CRT-combine, centre, reduce) and are what the claims of DESIGN.md 5.14 are checked with."""
from fractions import Fraction

import numpy as np

_LB = {2: 16, 4: 32, 8: 64}


def limb_bits(a):
    return _LB[np.asarray(a).dtype.itemsize]


def prod(v):
    r = 1
    for x in v:
        r *= int(x)
    return r


def band(P, src, lb):
    """the width ks e / 2^60 of the band above 1/2 in which the centred conversion may keep x instead of x - Q"""
    e = Fraction(5, 4) if lb == 64 else Fraction(2**(lb - 2))
    return src[1] * e / 2**60


def fixed(y, p, lb):
    """f: the fixed-point image of y / p with 60 fraction bits, as the header defines it (y an integer or an object array)"""
    if lb == 64:
        return (y * (2**124 // p)) >> 64
    return y * (2**60 // p)


def parts(a, P, src):
    """per source row the canonical y_i (object arrays [ks][..., n]), plus u = floor(sum y_i / p_i) and v of the header"""
    a = np.asarray(a)
    lb, (s0, ks) = limb_bits(a), src
    Ps = [int(p) for p in P[s0:s0 + ks]]
    Q = prod(Ps)
    y, F, U = [], 0, 0
    for i, p in enumerate(Ps):
        yi = (a[..., s0 + i, :].astype(object) * pow(Q // p % p, -1, p)) % p
        y.append(yi)
        F = F + fixed(yi, p, lb)
        U = U + yi * (Q // p)           # = x + u Q
    return y, U // Q, (F + 2**59) >> 60


def baseconv_rns(a, P, src, dst, centered=False):
    """the row formula: a copy of `a` whose rows dst hold (sum_i y_i c_ij [- v Q_j]) mod p_j"""
    a = np.asarray(a)
    (s0, ks), (d0, kd) = src, dst
    Ps = [int(p) for p in P[s0:s0 + ks]]
    Q = prod(Ps)
    y, _, v = parts(a, P, src)
    out = a.copy()
    for j in range(d0, d0 + kd):
        pj = int(P[j])
        acc = 0
        for i, p in enumerate(Ps):
            acc = acc + y[i] * (Q // p % pj)
        if centered:
            acc = acc - v * (Q % pj)
        out[..., j, :] = (acc % pj).astype(a.dtype)
    return out


def crt_rows(a, P, src):
    """x in [0, Q) behind rows src of every coefficient position (an object array of Python integers)"""
    a = np.asarray(a)
    s0, ks = src
    Ps = [int(p) for p in P[s0:s0 + ks]]
    Q = prod(Ps)
    X = 0
    for i, p in enumerate(Ps):
        qi = Q // p
        X = X + a[..., s0 + i, :].astype(object) * (qi * pow(qi % p, -1, p))
    return X % Q


def centre(x, Q):
    """the centred representative: x below Q / 2, x - Q from there on (object array)"""
    return x - Q * (2 * x >= Q).astype(object)


def baseconv_exact(a, P, src, dst, centered=False, keep=None):
    """the exact statement.  Fast mode needs u, which is not a function of x alone: it is taken from the y_i (parts).  Centred mode
    reduces the centred representative; `keep` (a boolean array) marks positions -- those in the band -- that keep x itself."""
    a = np.asarray(a)
    s0, ks = src
    Q = prod(P[s0:s0 + ks])
    x = crt_rows(a, P, src)
    if centered:
        val = centre(x, Q)
        if keep is not None:
            val = np.where(keep, x, val)
    else:
        val = x + parts(a, P, src)[1] * Q
    out = a.copy()
    for j in range(dst[0], dst[0] + dst[1]):
        out[..., j, :] = (val % int(P[j])).astype(a.dtype)
    return out


def in_band(a, P, src):
    """boolean array: x / Q lies in [1/2, 1/2 + ks e / 2^60)"""
    Q = prod(P[src[0]:src[0] + src[1]])
    w = band(P, src, limb_bits(a))
    x = crt_rows(a, P, src)
    lo, hi = (Q + 1) // 2, Fraction(Q) * (Fraction(1, 2) + w)
    f = np.frompyfunc(lambda v: bool(lo <= v < hi), 1, 1)
    return f(x).astype(bool)


def rows_of(X, P, rows, dtype):
    """residues of the integers X (object array [..., n]) in the given rows: [..., len(rows), n]"""
    X = np.asarray(X, dtype=object)
    out = np.empty(X.shape[:-1] + (len(rows), X.shape[-1]), dtype=dtype)
    for t, j in enumerate(rows):
        out[..., t, :] = (X % int(P[j])).astype(dtype)
    return out


def moddown_rns(a, P, k, floor=False):
    """the row formula: Y_j = (x_j - conv_j) P^-1 mod p_j, conv the centred (default) or fast conversion of the last k rows"""
    a = np.asarray(a)
    nm = a.shape[-2]
    conv = baseconv_rns(a, P, (nm - k, k), (0, nm - k), centered=not floor)
    Pk = prod(P[nm - k:nm])
    out = np.empty(a.shape[:-2] + (nm - k, a.shape[-1]), dtype=a.dtype)
    for j in range(nm - k):
        pj = int(P[j])
        out[..., j, :] = (((a[..., j, :].astype(object) - conv[..., j, :].astype(object)) * pow(Pk % pj, -1, pj)) % pj).astype(a.dtype)
    return out


def moddown_exact(a, P, k, how):
    """through the integer X in [0, Q_all): how = "floor" -> floor(X / P); "nearest" -> floor(X / P) + (2 (X mod P) >= P);
    "approx" -> floor(X / P) - u (the fast conversion's u); all mod Q_all / P"""
    a = np.asarray(a)
    nm = a.shape[-2]
    Pk, Qk = prod(P[nm - k:nm]), prod(P[:nm - k])
    X = crt_rows(a, P, (0, nm))
    Y = X // Pk
    if how == "nearest":
        Y = Y + (2 * (X % Pk) >= Pk).astype(object)
    elif how == "approx":
        Y = Y - parts(a, P, (nm - k, k))[1]
    return rows_of(Y % Qk, P, range(nm - k), a.dtype)


def random_batch(P, n, batch, dtype, seed):
    rnd = np.random.RandomState(seed)
    out = np.empty((batch, len(P), n), dtype=dtype)
    for i, p in enumerate(P):
        out[:, i, :] = rnd.randint(0, int(p), size=(batch, n), dtype=np.int64).astype(dtype)
    return out


def plant(a, P, src, values, b=0, first=0):
    """writes the integers `values` (each in [0, Q) of rows src) into rows src of polynomial b at positions first, first + 1, ..."""
    s0, ks = src
    for t, x in enumerate(values):
        for i in range(s0, s0 + ks):
            a[b, i, first + t] = int(x) % int(P[i])
    return a


def edge_values(P, src):
    """x = 0, 1, floor(Q/2) - 1, floor(Q/2), floor(Q/2) + 1, Q - 1"""
    Q = prod(P[src[0]:src[0] + src[1]])
    return [0, 1 % Q, (Q // 2 - 1) % Q, Q // 2, (Q // 2 + 1) % Q, Q - 1]


def band_values(P, src, lb):
    """x just below the band, at its lower edge, inside it, at its last point and just above it"""
    Q = prod(P[src[0]:src[0] + src[1]])
    lo = (Q + 1) // 2                                   # the first x with x / Q >= 1/2 (Q is odd, or ks = 1 and Q = p)
    top = Fraction(Q) * (Fraction(1, 2) + band(P, src, lb))
    hi = int(top) if top != int(top) else int(top) - 1  # the last x inside the band
    return [v % Q for v in (lo - 2, lo - 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1, hi + 2)]


def all_y_max(P, src):
    """the source words x_i for which every y_i = p_i - 1: x_i = (p_i - 1) (Q/p_i) mod p_i"""
    s0, ks = src
    Ps = [int(p) for p in P[s0:s0 + ks]]
    Q = prod(Ps)
    return [((p - 1) * (Q // p)) % p for p in Ps]
