"""Python-integer restatement of the ciphertext multiplication with relinearisation (include/nflhip.h "ciphertext multiplication") --
what tests/test_mulrelin_cpu.py and tests/test_gpu_mulrelin.py check against.  It is the header's definition and nothing else: the
tensor product on Python integers, the mod-up of every digit by baseconv_util.baseconv_rns, the sums of products with pi (.) d_c as
their addend, ONE mod-down by baseconv_util.moddown_rns (by one row more with the rescale), the CPU oracle's transforms in between.
two_step is the way around it: the tensor product, keyswitch_util.keyswitch_rns on its third component, the addition."""
import numpy as np

import baseconv_util as B
from keyswitch_util import digits, keyswitch_rns


def tensor_rns(a0, a1, b0, b1, P):
    """(a0 b0, a0 b1 + a1 b0, a1 b1) row by row mod P[j] on the rows the blocks have; b0 = b1 = None: the square"""
    a0, a1 = np.asarray(a0), np.asarray(a1)
    b0, b1 = (a0, a1) if b0 is None else (np.asarray(b0), np.asarray(b1))
    outs = [np.empty_like(a0) for _ in range(3)]
    for j in range(a0.shape[-2]):
        p = int(P[j])
        x0, x1, y0, y1 = (v[..., j, :].astype(object) for v in (a0, a1, b0, b1))
        for o, v in zip(outs, (x0 * y0, x0 * y1 + x1 * y0, x1 * y1)):
            o[..., j, :] = (v % p).astype(a0.dtype)
    return outs


def mulrelin_rns(a0, a1, b0, b1, key, P, K, alpha, centered, floor, rescale, orc, orc_kept, orc_out=None):
    """a*, b* = [batch, L, n] in NTT form over the first L = nm - K moduli, key = [dnum, 2, nm, n]; orc the oracle of the full context,
    orc_kept of the first L moduli, orc_out of the first L - 1 (the rescale).  Returns (out0, out1) in NTT form."""
    key = np.asarray(key)
    nm = len(P)
    L = nm - K
    d = tensor_rns(a0, a1, b0, b1, P)
    batch, _, n = d[0].shape
    S = digits(nm, K, alpha)
    assert d[0].shape[1] == L and key.shape == (len(S), 2, nm, n)
    Ps = B.prod(P[L:])
    X = np.zeros((batch, nm, n), dtype=d[0].dtype)
    X[:, :L] = orc_kept.intt(np.ascontiguousarray(d[2]))
    acc = []
    for c in range(2):                                   # the addend: pi_j d_c on the kept rows, zero on the special ones
        A = np.zeros((batch, nm, n), dtype=object)
        for j in range(L):
            A[:, j] = d[c][:, j].astype(object) * (Ps % int(P[j]))
        acc.append(A)
    for t, src in enumerate(S):
        U = orc.ntt(B.baseconv_rns(X, P, src, (0, nm), centered=centered)).astype(object)
        for c in range(2):
            acc[c] = acc[c] + U * key[t, c].astype(object)[None]
    outs = []
    for c in range(2):
        r = np.empty((batch, nm, n), dtype=d[0].dtype)
        for j in range(nm):
            r[:, j] = (acc[c][:, j] % int(P[j])).astype(d[0].dtype)
        down = B.moddown_rns(orc.intt(r), P, K + 1 if rescale else K, floor=floor)
        outs.append((orc_out if rescale else orc_kept).ntt(down))
    return outs[0], outs[1]


def two_step(a0, a1, b0, b1, key, P, K, alpha, centered, floor, orc, orc_kept):
    """d_c + key_switch(d2)_c: the composition the one call replaces (no rescale)"""
    d = tensor_rns(a0, a1, b0, b1, P)
    ks = keyswitch_rns(np.ascontiguousarray(d[2]), key, P, K, alpha, centered, floor, orc, orc_kept)
    outs = []
    for c in range(2):
        o = np.empty_like(d[c])
        for j in range(d[c].shape[-2]):
            o[:, j] = ((d[c][:, j].astype(object) + ks[c][:, j].astype(object)) % int(P[j])).astype(o.dtype)
        outs.append(o)
    return outs[0], outs[1]


def relin_key(P, K, alpha, n, s_ntt, s2_ntt, orc, rnd, dtype=np.uint64, seed=7):
    """key[d][0] = -a_d s + e_d + P g_d s', key[d][1] = a_d in NTT form over all moduli, |e_d| <= 8 (tests/test_keyswitch_cpu.py)"""
    nm = len(P)
    L = nm - K
    Q, Ps = B.prod(P[:L]), B.prod(P[L:])
    S = digits(nm, K, alpha)
    key = np.empty((len(S), 2, nm, n), dtype=dtype)
    for t, (s0, ks) in enumerate(S):
        Qd = B.prod(P[s0:s0 + ks])
        g = (Q // Qd) * pow((Q // Qd) % Qd, -1, Qd)
        a_ntt = B.random_batch(P, n, 1, dtype, seed + t)[0]
        e_ntt = orc.ntt(B.rows_of(rnd.randint(-8, 9, size=n).astype(object), P, range(nm), dtype)[None])[0]
        for j, p in enumerate(P):
            key[t, 0, j] = ((e_ntt[j].astype(object) - a_ntt[j].astype(object) * s_ntt[j] + (Ps * g) % p * s2_ntt[j]) % p).astype(dtype)
        key[t, 1] = a_ntt
    return key
