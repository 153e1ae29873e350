"""Python-integer restatement of the several-output weighted sum of NTT-form automorphisms and of the BSGS slot linear transform
(include/nflhip.h "weighted sums of automorphisms into several outputs", "BSGS slot linear transforms") -- what tests/test_bsgs_cpu.py,
tests/test_gpu_automorphism_mac_multi.py and tests/test_gpu_bsgs.py check against.  It is the header's map and nothing else, from the
pieces that exist: lintrans_util.mac_rns / modup_digits / keyswitch_sums, baseconv_util.moddown_rns, automorph_util.sigma_ntt and the
CPU oracle's transforms; the level form through level_util and level_rotate_util.gather_weight."""
import numpy as np

import baseconv_util as B
from automorph_util import sigma_ntt
from level_rotate_util import _gathered, _level, gather_weight
from lintrans_util import keyswitch_sums, mac_rns, modup_digits, reduce_rows


def mac_multi_rns(ins, weights, ks, P, addends=None):
    """[addends[o] + sum_t weights[o][t] (.) sigma^NTT_ks[t](ins[t]) mod P[j] for o]: mac_rns per output over its non-None weights"""
    outs = []
    for o, ws in enumerate(weights):
        sel = [t for t, w in enumerate(ws) if w is not None]
        add = None if addends is None else addends[o]
        if sel:
            outs.append(mac_rns([ins[t] for t in sel], [ws[t] for t in sel], [ks[t] for t in sel], P, addend=add))
        else:
            outs.append(np.zeros_like(np.asarray(ins[0])) if add is None else np.array(add))
    return outs


def _add(x, y, P):
    return reduce_rows(x.astype(object) + y.astype(object), P, x.dtype)


def bsgs_rns(c0, c1, bkeys, bks, gkeys, gks, weights, P, K, alpha, centered, floor, orc, orc_kept, memo=None):
    """c0 (or None), c1 = [batch, L, n] in NTT form over the first L = nm - K moduli; bkeys[i] / gkeys[j] = [dnum, 2, nm, n] or None (the
    unrotated step, k = 1 mod 2n); weights[j][i] = [nm, n] or None; every k odd.  Returns (out0, out1).  memo: a dict that keeps the
    mod-up of c1 and the babies' key-switch sums per key object (id), for callers that repeat them."""
    c1 = np.asarray(c1)
    nm = len(P)
    L = nm - K
    n = c1.shape[-1]
    n1, n2 = len(bks), len(gks)
    memo = {} if memo is None else memo
    assert all(bkeys[i] is not None or bks[i] % (2 * n) == 1 for i in range(n1)) and all(gkeys[j] is not None or gks[j] % (2 * n) == 1 for j in range(n2))
    assert all(any(w is not None for w in weights[j]) for j in range(n2))
    keyed = [i for i in range(n1) if bkeys[i] is not None]
    unkeyed = [i for i in range(n1) if bkeys[i] is None]
    zero_all, zero_kept = np.zeros((c1.shape[0], nm, n), dtype=c1.dtype), np.zeros_like(c1)

    def moddown(x):
        return orc_kept.ntt(B.moddown_rns(orc.intt(x), P, K, floor=floor))
    S = {}
    if keyed:
        if "U" not in memo:
            memo["U"] = modup_digits(c1, P, K, alpha, centered, orc, orc_kept)
        for i in keyed:
            if id(bkeys[i]) not in memo:
                memo[id(bkeys[i])] = keyswitch_sums(memo["U"], bkeys[i], P)
            S[i] = memo[id(bkeys[i])]
    A, O, summed = [zero_all, zero_all], [zero_kept, zero_kept], False
    for j in range(n2):
        w = weights[j]
        ki = [i for i in keyed if w[i] is not None]
        V = [mac_rns([S[i][c] for i in ki], [w[i] for i in ki], [bks[i] for i in ki], P) if ki else zero_all for c in range(2)]
        ai = [i for i in range(n1) if w[i] is not None]
        W0 = None if c0 is None else mac_rns([c0] * len(ai), [w[i] for i in ai], [bks[i] for i in ai], P[:L])
        ui = [i for i in unkeyed if w[i] is not None]
        W1 = mac_rns([c1] * len(ui), [w[i] for i in ui], [1] * len(ui), P[:L]) if ui else zero_kept
        if gkeys[j] is not None:
            v = _add(moddown(V[1]) if keyed else zero_kept, W1, P[:L])
            T = keyswitch_sums(modup_digits(v, P, K, alpha, centered, orc, orc_kept), gkeys[j], P)
            A = [_add(A[0], sigma_ntt(_add(V[0], T[0], P), gks[j]), P), _add(A[1], sigma_ntt(T[1], gks[j]), P)]
            summed = True
            if W0 is not None:
                O[0] = _add(O[0], sigma_ntt(W0, gks[j]), P[:L])
        else:
            if keyed:
                A = [_add(A[c], V[c], P) for c in range(2)]
                summed = True
            if W0 is not None:
                O[0] = _add(O[0], W0, P[:L])
            O[1] = _add(O[1], W1, P[:L])
    if not summed:
        return O[0], O[1]
    return _add(moddown(A[0]), O[0], P[:L]), _add(moddown(A[1]), O[1], P[:L])


def bsgs_level_rns(c0, c1, bkeys, bks, gkeys, gks, weights, P, K, alpha, level, centered, floor, orc, memo=None):
    """the level call: c0 (or None), c1 = [batch, l, n]; the keys are the TOP-LEVEL Galois keys [dnum_L, 2, nm, n], the weights the
    TOP-LEVEL diagonals [nm, n]; P the nm moduli, orc the oracle of the full context.  bsgs_rns on the moduli of the live rows with the
    gathered keys and weights and min(alpha, l).  memo: a dict kept by the caller per (level, centered)."""
    memo = {} if memo is None else memo
    nm = len(P)
    _, Pl, o_all, o_kept = _level(P, K, level, orc)
    ws = [[None if w is None else gather_weight(w, nm, K, level) for w in row] for row in weights]
    gb, gg = _gathered(bkeys, nm, K, alpha, level, memo), _gathered(gkeys, nm, K, alpha, level, memo)
    return bsgs_rns(c0, c1, gb, bks, gg, gks, ws, Pl, K, min(alpha, level), centered, floor, o_all, o_kept, memo=memo)
