"""Python-integer restatement of a hoisted rotation (include/nflhip.h "hoisted rotations") -- what tests/test_rotate_cpu.py and
tests/test_gpu_rotate.py check against.  It is the header's definition and nothing else: per rotation keyswitch_util.keyswitch_rns
of c1, the addition of c0 on Python integers, automorph_util.sigma_ntt of both results -- the permutation last."""
import numpy as np

from automorph_util import sigma_ntt
from keyswitch_util import keyswitch_rns


def add_rows(x, y, P):
    """x + y row by row mod P[j] on Python integers; x, y = [batch, len(P), n]"""
    out = np.empty_like(x)
    for j, p in enumerate(P):
        out[:, j] = ((x[:, j].astype(object) + y[:, j].astype(object)) % int(p)).astype(x.dtype)
    return out


def rotate_rns(c0, c1, keys, ks, P, K, alpha, centered, floor, orc, orc_kept, memo=None):
    """c0 (or None), c1 = [batch, L, n] in NTT form over the first L = nm - K moduli; keys[m] = [dnum, 2, nm, n] in NTT form over all
    nm; ks[m] odd.  Returns [(out0, out1)] per rotation.  memo: a dict that keeps the key switch per key object (id), for callers
    that repeat a key."""
    L = len(P) - K
    outs = []
    for key, k in zip(keys, ks):
        if memo is not None and id(key) in memo:
            d0, d1 = memo[id(key)]
        else:
            d0, d1 = keyswitch_rns(c1, key, P, K, alpha, centered, floor, orc, orc_kept)
            if memo is not None:
                memo[id(key)] = (d0, d1)
        y0 = d0 if c0 is None else add_rows(d0, np.asarray(c0), P[:L])
        outs.append((sigma_ntt(y0, k), sigma_ntt(d1, k)))
    return outs
