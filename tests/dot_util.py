"""Python-integer restatement of the sum of products across polynomials (include/nflhip.h "sums of products") on word arrays --
what tests/test_dot_cpu.py and tests/test_gpu_dot.py check against:
    out[g][m][i] = (addend[g][m][i] + sum_j a[g][j][m][i] * b[g][j][m][i]) mod p_m."""
import numpy as np


def dot_ref(a, b, P, addend=None, positions=None, rows=None):
    """a = [groups, terms, nm, n]; b alike, or [terms, nm, n] for an operand every group shares; addend = [groups, nm, n] or
    None.  Exact Python integers on object arrays.  `positions` restricts the last axis and `rows` the moduli (sampled checks
    of large cases); the result keeps the dtype of a."""
    a, b = np.asarray(a), np.asarray(b)
    if b.ndim == 3:
        b = b[None]
    nm = a.shape[-2]
    rows = list(range(nm)) if rows is None else list(rows)
    sel = slice(None) if positions is None else np.asarray(positions)
    out = np.empty((a.shape[0], len(rows), a.shape[-1] if positions is None else len(sel)), dtype=a.dtype)
    for k, m in enumerate(rows):
        s = (a[:, :, m, sel].astype(object) * b[:, :, m, sel].astype(object)).sum(axis=1)
        if addend is not None:
            s = s + np.asarray(addend)[:, m, sel].astype(object)
        out[:, k, :] = (s % int(P[m])).astype(a.dtype)
    return out


def random_polys(P, n, count, dtype, seed):
    rnd = np.random.RandomState(seed)
    out = np.empty((count, len(P), n), dtype=dtype)
    for i, p in enumerate(P):
        out[:, i, :] = rnd.randint(0, int(p), size=(count, n), dtype=np.int64).astype(dtype)
    return out


def full_polys(P, n, count, dtype):
    """every word p_m - 1: the largest products, the lazy accumulator's edge"""
    return np.broadcast_to(np.array([int(p) - 1 for p in P], dtype=dtype)[None, :, None], (count, len(P), n)).copy()


def edge_polys(P, n, count, dtype, seed=1):
    """`count` polynomials that cycle through: every word 0; every word p_m - 1; a mix (words drawn from {0, 1, p_m - 1});
    random"""
    out = random_polys(P, n, count, dtype, seed)
    rnd = np.random.RandomState(seed + 1000)
    for k in range(count):
        if k % 4 == 0:
            out[k] = 0
        elif k % 4 == 1:
            out[k] = full_polys(P, n, 1, dtype)[0]
        elif k % 4 == 2:
            pick = rnd.randint(0, 3, size=(len(P), n))
            top = np.array([int(p) - 1 for p in P], dtype=dtype)[:, None]
            out[k] = np.where(pick == 0, np.zeros_like(top), np.where(pick == 1, np.ones_like(top), top))
    return out
