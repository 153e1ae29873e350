"""Python-integer restatement of the RNS rescale by the last modulus (include/nflhip.h "RNS rescale") on [..., nmoduli, degree]
word arrays -- what tests/test_rescale_cpu.py and tests/test_gpu_rescale.py check against.  Two independent functions:
rescale_exact goes through the integer X in [0, Q) behind the residues, rescale_rns is the row formula."""
import numpy as np


def _consts(P, nm):
    P = [int(p) for p in P[:nm]]
    q = P[-1]
    return P, q, (q - 1) // 2


def crt_combine(a, P, positions=None):
    """X in [0, Q) for every coefficient position (an object array of Python integers, shape [..., len(positions) or n])"""
    a = np.asarray(a)
    nm = a.shape[-2]
    P, _, _ = _consts(P, nm)
    Q = 1
    for p in P:
        Q *= p
    sel = slice(None) if positions is None else np.asarray(positions)
    X = 0
    for i, p in enumerate(P):
        qi = Q // p
        X = X + a[..., i, sel].astype(object) * (qi * pow(qi % p, -1, p))
    return X % Q


def divide_round(X, P, dtype):
    """residues mod p_0 .. p_(L-1) of floor((X + h) / q) mod Q / q, for an object array X of integers in [0, Q)"""
    P, q, h = _consts(P, len(P))
    Qp = 1
    for p in P[:-1]:
        Qp *= p
    Y = ((X + h) // q) % Qp
    out = np.empty(X.shape[:-1] + (len(P) - 1, X.shape[-1]), dtype=dtype)
    for i, p in enumerate(P[:-1]):
        out[..., i, :] = (Y % p).astype(dtype)
    return out


def rescale_exact(a, P, positions=None):
    """CRT-combine to X, (X + h) // q % Q', reduce per kept row; `positions` restricts the last axis (sampled checks)"""
    a = np.asarray(a)
    return divide_round(crt_combine(a, P, positions), [int(p) for p in P[:a.shape[-2]]], a.dtype)


def rescale_rns(a, P):
    """the row formula: r = (x_L + h) mod q, y_i = (x_i + h - r) q^-1 mod p_i"""
    a = np.asarray(a)
    nm = a.shape[-2]
    P, q, h = _consts(P, nm)
    r = (a[..., nm - 1, :].astype(object) + h) % q
    out = np.empty(a.shape[:-2] + (nm - 1, a.shape[-1]), dtype=a.dtype)
    for i, p in enumerate(P[:-1]):
        out[..., i, :] = (((a[..., i, :].astype(object) + h - r) * pow(q % p, -1, p)) % p).astype(a.dtype)
    return out


def rescale_ntt(A, P, big, small, core=rescale_rns):
    """NTT form: `big` / `small` are oracles (ntt, intt) of the nm- and the (nm - 1)-modulus contexts"""
    return small.ntt(core(big.intt(np.ascontiguousarray(A)), P))


def random_batch(P, n, batch, dtype, seed):
    rnd = np.random.RandomState(seed)
    out = np.empty((batch, len(P), n), dtype=dtype)
    for i, p in enumerate(P):
        out[:, i, :] = rnd.randint(0, int(p), size=(batch, n), dtype=np.int64).astype(dtype)
    return out


def edge_batch(P, n, dtype, seed=1, combos=True):
    """planted polynomials: every word 0; every word p_i - 1 (X = Q - 1, the result is 0); last-row words from
    {0, h, h + 1, q - 1} crossed with first-row words from {0, p_0 - 1}, the other rows random (combos=False: the first two)"""
    P, q, h = _consts(P, len(P))
    polys = [np.zeros((len(P), n), dtype=dtype), np.array([[p - 1] * n for p in P], dtype=dtype)]
    if combos:
        k = 0
        for last in (0, h, h + 1, q - 1):
            for first in (0, P[0] - 1):
                e = random_batch(P, n, 1, dtype, seed + k)[0]
                e[len(P) - 1, :] = last
                e[0, :] = first
                polys.append(e)
                k += 1
    return np.stack(polys)
