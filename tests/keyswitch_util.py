"""Python-integer restatement of the hybrid key switch in NTT form (include/nflhip.h "hybrid key switching") -- what
tests/test_keyswitch_cpu.py and tests/test_gpu_keyswitch.py check against.  It is the header's definition and nothing else: the
mod-up of every digit by baseconv_util.baseconv_rns, the sums of products on Python integers, the mod-down by
baseconv_util.moddown_rns, with the CPU oracle's transforms in between."""
import numpy as np

import baseconv_util as B


def digits(nm, K, alpha):
    """the digits S_d = (first row, count) of the first L = nm - K rows; the last may be short"""
    L = nm - K
    return [(s0, min(alpha, L - s0)) for s0 in range(0, L, alpha)]


def keyswitch_rns(a_ntt, key, P, K, alpha, centered, floor, orc, orc_kept):
    """a_ntt = [batch, L, n] in NTT form over the first L = nm - K moduli, key = [dnum, 2, nm, n] in NTT form over all nm; orc the
    oracle of the full context, orc_kept of the first L moduli.  Returns (out0, out1), each [batch, L, n] in NTT form."""
    a_ntt, key = np.ascontiguousarray(a_ntt), np.asarray(key)
    nm = len(P)
    L = nm - K
    batch, _, n = a_ntt.shape
    S = digits(nm, K, alpha)
    assert a_ntt.shape[1] == L and key.shape == (len(S), 2, nm, n)
    X = np.zeros((batch, nm, n), dtype=a_ntt.dtype)
    X[:, :L] = orc_kept.intt(a_ntt)                      # rows [0, L) of the context are the moduli of orc_kept
    acc = [np.zeros((batch, nm, n), dtype=object), np.zeros((batch, nm, n), dtype=object)]
    for d, src in enumerate(S):
        U = orc.ntt(B.baseconv_rns(X, P, src, (0, nm), centered=centered)).astype(object)
        for c in range(2):
            acc[c] = acc[c] + U * key[d, c].astype(object)[None]
    outs = []
    for c in range(2):
        r = np.empty((batch, nm, n), dtype=a_ntt.dtype)
        for j in range(nm):
            r[:, j] = (acc[c][:, j] % int(P[j])).astype(a_ntt.dtype)
        outs.append(orc_kept.ntt(B.moddown_rns(orc.intt(r), P, K, floor=floor)))
    return outs[0], outs[1]
