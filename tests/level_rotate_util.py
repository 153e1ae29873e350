"""Hoisted rotations and slot linear transforms below the top level (include/nflhip.h "rotations and linear transforms at a level")
restated through what exists: rotate_util.rotate_rns and lintrans_util.lintrans_rns on the moduli P_l = [P[j] for j in A_l],
A_l = [0, l) and [L, nm), with level_util.gather_key per Galois key, weights[m][A_l] per diagonal and level_util.RowsOracle for the
transforms -- the header's definition of a level call and nothing else."""
import numpy as np

from level_util import RowsOracle, gather_key, level_rows
from lintrans_util import lintrans_rns
from rotate_util import rotate_rns


def _level(P, K, level, orc):
    nm = len(P)
    rows = level_rows(nm, K, level)
    return rows, [P[j] for j in rows], RowsOracle(orc, nm, rows), RowsOracle(orc, nm, range(level))


def _gathered(keys, nm, K, alpha, level, memo):
    """gather_key per DISTINCT key object, kept in memo so that a repeated key is one object for the restatement's own memo"""
    out = []
    for key in keys:
        if key is None:
            out.append(None)
            continue
        k = ("gathered", id(key))
        if k not in memo:
            memo[k] = gather_key(key, nm, K, alpha, level)
        out.append(memo[k])
    return out


def gather_weight(w, nm, K, level):
    """weight_l[r] = weight[phys(r)]: what the explicit level context takes"""
    return np.ascontiguousarray(np.asarray(w)[level_rows(nm, K, level)])


def rotate_level_rns(c0, c1, keys, ks, P, K, alpha, level, centered, floor, orc, memo=None):
    """c0 (or None), c1 = [batch, l, n]; keys[m] = the TOP-LEVEL Galois key [dnum_L, 2, nm, n]; P the nm moduli, orc the oracle of the
    full context.  Returns [(out0, out1)] per rotation, each [batch, l, n].  memo: a dict kept by the caller per (level, modes)."""
    memo = {} if memo is None else memo
    _, Pl, o_all, o_kept = _level(P, K, level, orc)
    return rotate_rns(c0, c1, _gathered(keys, len(P), K, alpha, level, memo), ks, Pl, K, alpha, centered, floor, o_all, o_kept, memo=memo)


def lintrans_level_rns(c0, c1, keys, weights, ks, P, K, alpha, level, centered, floor, orc, memo=None):
    """as rotate_level_rns; keys[m] may be None (the unrotated diagonal), weights[m] = the TOP-LEVEL diagonal [nm, n].  Returns
    (out0, out1).  memo: a dict kept by the caller per (level, centered)."""
    memo = {} if memo is None else memo
    nm = len(P)
    _, Pl, o_all, o_kept = _level(P, K, level, orc)
    ws = [gather_weight(w, nm, K, level) for w in weights]
    return lintrans_rns(c0, c1, _gathered(keys, nm, K, alpha, level, memo), ws, ks, Pl, K, alpha, centered, floor, o_all, o_kept, memo=memo)
