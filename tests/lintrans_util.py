"""Python-integer restatement of the weighted sum of NTT-form automorphisms and of the slot linear transform (include/nflhip.h
"weighted sums of automorphisms", "slot linear transforms") -- what tests/test_lintrans_cpu.py, tests/test_gpu_automorphism_mac.py and
tests/test_gpu_lintrans.py check against.  It is the header's two definitions and nothing else: the mod-up of every digit by
baseconv_util.baseconv_rns as keyswitch_util.keyswitch_rns forms it, the sums of products on Python integers,
automorph_util.sigma_ntt, ONE baseconv_util.moddown_rns of the weighted sums, with the CPU oracle's transforms in between."""
import numpy as np

import baseconv_util as B
from automorph_util import sigma_ntt
from keyswitch_util import digits


def reduce_rows(acc, P, dtype):
    """the object array acc = [batch, len(P), n] row by row mod P[j], as canonical words"""
    out = np.empty(acc.shape, dtype=dtype)
    for j, p in enumerate(P):
        out[:, j] = (acc[:, j] % int(p)).astype(dtype)
    return out


def mac_rns(ins, weights, ks, P, addend=None):
    """out = addend + sum_t weights[t] (.) sigma^NTT_ks[t](ins[t]) mod P[j]: ins[t] = [batch, rows, n] over the first rows = len(P)
    moduli, weights[t] = [>= rows, n] (the rows past `rows` are not read)"""
    rows = len(P)
    acc = np.zeros(np.asarray(ins[0]).shape, dtype=object) if addend is None else np.asarray(addend).astype(object)
    for x, w, k in zip(ins, weights, ks):
        x = np.asarray(x)
        assert x.shape[1] == rows
        acc = acc + sigma_ntt(x, k).astype(object) * np.asarray(w)[:rows].astype(object)[None]
    return reduce_rows(acc, P, np.asarray(ins[0]).dtype)


def modup_digits(c1, P, K, alpha, centered, orc, orc_kept):
    """U_d = [batch, nm, n] in NTT form for every digit d, as keyswitch_util.keyswitch_rns forms it from c1 = [batch, L, n]"""
    c1 = np.ascontiguousarray(c1)
    nm = len(P)
    L = nm - K
    batch, _, n = c1.shape
    X = np.zeros((batch, nm, n), dtype=c1.dtype)
    X[:, :L] = orc_kept.intt(c1)
    return [orc.ntt(B.baseconv_rns(X, P, src, (0, nm), centered=centered)) for src in digits(nm, K, alpha)]


def keyswitch_sums(U, key, P):
    """S_c = sum_d U_d (.) key[d][c] mod p_j for c = 0, 1: [batch, nm, n] canonical words (nflhip_dot_dev)"""
    out = []
    for c in range(2):
        acc = np.zeros(U[0].shape, dtype=object)
        for d, u in enumerate(U):
            acc = acc + u.astype(object) * np.asarray(key)[d, c].astype(object)[None]
        out.append(reduce_rows(acc, P, U[0].dtype))
    return out


def lintrans_rns(c0, c1, keys, weights, ks, P, K, alpha, centered, floor, orc, orc_kept, memo=None):
    """c0 (or None), c1 = [batch, L, n] in NTT form over the first L = nm - K moduli; keys[m] = [dnum, 2, nm, n] or None (the
    unrotated diagonal, ks[m] = 1 mod 2n); weights[m] = [nm, n]; ks[m] odd.  Returns (out0, out1).  memo: a dict that keeps the
    mod-up and the key-switch sums per key object (id), for callers that repeat them."""
    c1 = np.asarray(c1)
    nm = len(P)
    L = nm - K
    n = c1.shape[-1]
    memo = {} if memo is None else memo
    keyed = [m for m, key in enumerate(keys) if key is not None]
    assert all(keys[m] is not None or ks[m] % (2 * n) == 1 for m in range(len(ks)))
    Y = [np.zeros_like(c1), np.zeros_like(c1)]
    if keyed:
        if "U" not in memo:
            memo["U"] = modup_digits(c1, P, K, alpha, centered, orc, orc_kept)
        for m in keyed:
            if id(keys[m]) not in memo:
                memo[id(keys[m])] = keyswitch_sums(memo["U"], keys[m], P)
        for c in range(2):
            A = mac_rns([memo[id(keys[m])][c] for m in keyed], [weights[m] for m in keyed], [ks[m] for m in keyed], P)
            Y[c] = orc_kept.ntt(B.moddown_rns(orc.intt(A), P, K, floor=floor))
    out0 = Y[0] if c0 is None else mac_rns([c0] * len(ks), weights, ks, P[:L], addend=Y[0])
    un = [m for m in range(len(ks)) if keys[m] is None]
    out1 = mac_rns([c1] * len(un), [weights[m] for m in un], [1] * len(un), P[:L], addend=Y[1]) if un else Y[1]
    return out0, out1
