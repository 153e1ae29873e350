"""Calls below the top level (include/nflhip.h "leveled key switching") restated through what exists: keyswitch_util.keyswitch_rns and
mulrelin_util.mulrelin_rns on the moduli P_l = [P[j] for j in A_l], A_l = [0, l) and [L, nm), with the gathered key
key[:dnum_l, :, A_l] -- the header's definition of a level call.  The one thing those functions need besides is an oracle over a row
SUBSET of the full context: RowsOracle embeds into nm rows, transforms with the full oracle and extracts.  The transforms are per
row, so this is exact."""
import numpy as np

from keyswitch_util import keyswitch_rns
from mulrelin_util import mulrelin_rns


def level_rows(nm, K, level):
    """A_l"""
    L = nm - K
    assert 1 <= level <= L
    return list(range(level)) + list(range(L, nm))


def level_digits(level, alpha):
    """dnum_l = ceil(l / alpha)"""
    return (level + alpha - 1) // alpha


class RowsOracle:
    """ntt / intt of [batch, len(rows), n] blocks under the moduli `rows` of the full oracle's context"""

    def __init__(self, orc, nm, rows):
        self.orc, self.nm, self.rows = orc, nm, list(rows)

    def _run(self, f, x):
        x = np.asarray(x)
        full = np.zeros((x.shape[0], self.nm, x.shape[2]), dtype=x.dtype)
        full[:, self.rows] = x
        return np.ascontiguousarray(f(full)[:, self.rows])

    def ntt(self, x):
        return self._run(self.orc.ntt, x)

    def intt(self, x):
        return self._run(self.orc.intt, x)


def gather_key(key, nm, K, alpha, level):
    """key_l[d][c][r] = key[d][c][phys(r)] for d < dnum_l: what the explicit level context takes"""
    return np.ascontiguousarray(np.asarray(key)[:level_digits(level, alpha)][:, :, level_rows(nm, K, level)])


def _oracles(orc, nm, K, level):
    rows = level_rows(nm, K, level)
    return RowsOracle(orc, nm, rows), RowsOracle(orc, nm, range(level)), RowsOracle(orc, nm, range(level - 1))


def keyswitch_level_rns(a_ntt, key, P, K, alpha, level, centered, floor, orc):
    """a_ntt = [batch, l, n], key = the TOP-LEVEL key [dnum_L, 2, nm, n], P the nm moduli, orc the oracle of the full context"""
    nm = len(P)
    rows = level_rows(nm, K, level)
    o_all, o_kept, _ = _oracles(orc, nm, K, level)
    return keyswitch_rns(a_ntt, gather_key(key, nm, K, alpha, level), [P[j] for j in rows], K, alpha, centered, floor, o_all, o_kept)


def mulrelin_level_rns(a0, a1, b0, b1, key, P, K, alpha, level, centered, floor, rescale, orc):
    """a*, b* = [batch, l, n] (b0 = b1 = None: the square), key = the TOP-LEVEL key; returns [batch, l or l - 1, n]"""
    nm = len(P)
    rows = level_rows(nm, K, level)
    o_all, o_kept, o_out = _oracles(orc, nm, K, level)
    return mulrelin_rns(a0, a1, b0, b1, gather_key(key, nm, K, alpha, level), [P[j] for j in rows], K, alpha, centered, floor, rescale,
                        o_all, o_kept, o_out)
