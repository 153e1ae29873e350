"""Python-integer restatement of the sums of ciphertext products (include/nflhip.h "sums of ciphertext products") -- what
tests/test_mulrelin_dot_cpu.py, tests/test_gpu_tensor_dot.py and tests/test_gpu_mulrelin_dot.py check against.  tensor_dot_rns is the
header's three sums on Python integers.  mulrelin_dot_rns is the multiplication's map (mulrelin_util.mulrelin_rns at a level,
level_util.mulrelin_level_rns) with (d0, d1, d2) replaced by (D0, D1, D2): the same steps through the same helpers -- the mod-up of
every digit by baseconv_util.baseconv_rns, the sums against the gathered key with pi (.) D_c as their addend, ONE mod-down by
baseconv_util.moddown_rns -- and nothing of its own.  lazy_two_step is the way around it: D_c + key switch of D2."""
import numpy as np

import baseconv_util as B
from keyswitch_util import digits
from level_util import RowsOracle, gather_key, keyswitch_level_rns, level_rows


def operand(x, groups, terms, shared=False):
    """a dense block [groups * terms, rows, n], or [terms, rows, n] shared by every group -> [groups, terms, rows, n]"""
    x = np.asarray(x)
    if shared:
        assert x.shape[0] == terms
        return np.broadcast_to(x[None], (groups,) + x.shape)
    assert x.shape[0] == groups * terms
    return x.reshape((groups, terms) + x.shape[1:])


def tensor_dot_rns(a0, a1, b0, b1, P):
    """a*, b* = [groups, terms, rows, n] (b0 = b1 = None: the squares); (D0, D1, D2), each [groups, rows, n], row j mod P[j]"""
    a0, a1 = np.asarray(a0), np.asarray(a1)
    b0, b1 = (a0, a1) if b0 is None else (np.asarray(b0), np.asarray(b1))
    groups, _, rows, n = a0.shape
    outs = [np.empty((groups, rows, n), dtype=a0.dtype) for _ in range(3)]
    for j in range(rows):
        p = int(P[j])
        x0, x1, y0, y1 = (v[:, :, j, :].astype(object) for v in (a0, a1, b0, b1))
        for o, v in zip(outs, (x0 * y0, x0 * y1 + x1 * y0, x1 * y1)):
            o[:, j, :] = (v.sum(axis=1) % p).astype(a0.dtype)
    return outs


def relin_sums_rns(D, key, P, K, alpha, centered, floor, rescale, orc, orc_kept, orc_out=None):
    """mulrelin_util.mulrelin_rns from its second line on: D = (D0, D1, D2) on the first L = len(P) - K moduli of P"""
    key = np.asarray(key)
    nm = len(P)
    L = nm - K
    groups, _, n = D[0].shape
    S = digits(nm, K, alpha)
    assert D[0].shape[1] == L and key.shape == (len(S), 2, nm, n)
    Ps = B.prod(P[L:])
    X = np.zeros((groups, nm, n), dtype=D[0].dtype)
    X[:, :L] = orc_kept.intt(np.ascontiguousarray(D[2]))
    acc = []
    for c in range(2):
        A = np.zeros((groups, nm, n), dtype=object)
        for j in range(L):
            A[:, j] = D[c][:, j].astype(object) * (Ps % int(P[j]))
        acc.append(A)
    for t, src in enumerate(S):
        U = orc.ntt(B.baseconv_rns(X, P, src, (0, nm), centered=centered)).astype(object)
        for c in range(2):
            acc[c] = acc[c] + U * key[t, c].astype(object)[None]
    outs = []
    for c in range(2):
        r = np.empty((groups, nm, n), dtype=D[0].dtype)
        for j in range(nm):
            r[:, j] = (acc[c][:, j] % int(P[j])).astype(D[0].dtype)
        down = B.moddown_rns(orc.intt(r), P, K + 1 if rescale else K, floor=floor)
        outs.append((orc_out if rescale else orc_kept).ntt(down))
    return outs[0], outs[1]


def mulrelin_dot_rns(a0, a1, b0, b1, key, P, K, alpha, level, centered, floor, rescale, orc):
    """a*, b* = [groups, terms, l, n] in NTT form, key = the TOP-LEVEL key [dnum_L, 2, nm, n], P the nm moduli, orc the oracle of the
    full context; returns (out0, out1), [groups, l or l - 1, n]"""
    nm = len(P)
    rows = level_rows(nm, K, level)
    Pl = [P[j] for j in rows]
    D = tensor_dot_rns(a0, a1, b0, b1, Pl)
    return relin_sums_rns(D, gather_key(key, nm, K, alpha, level), Pl, K, min(alpha, level), centered, floor, rescale,
                          RowsOracle(orc, nm, rows), RowsOracle(orc, nm, range(level)), RowsOracle(orc, nm, range(level - 1)))


def lazy_two_step(a0, a1, b0, b1, key, P, K, alpha, level, centered, floor, orc):
    """D_c + key_switch_level(D2)_c: identity 1 for sums (no rescale)"""
    D = tensor_dot_rns(a0, a1, b0, b1, P[:level])
    ks = keyswitch_level_rns(np.ascontiguousarray(D[2]), key, P, K, alpha, level, centered, floor, orc)
    outs = []
    for c in range(2):
        o = np.empty_like(D[c])
        for j in range(level):
            o[:, j] = ((D[c][:, j].astype(object) + ks[c][:, j].astype(object)) % int(P[j])).astype(o.dtype)
        outs.append(o)
    return outs[0], outs[1]
