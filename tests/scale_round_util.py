"""Python-integer restatement of the RNS scale-and-round by t/Q (include/nflhip.h "BFV multiplication") on [..., nmoduli, degree]
word arrays -- what tests/test_scale_round_cpu.py, tests/test_gpu_scale_round.py and tests/test_gpu_bfv.py check against.  Two
independent statements: scale_round_rns is the header's row formulas composed from baseconv_util.baseconv_rns (it defines the words
bit for bit); scale_round_exact goes through the integer behind the residues (CRT-combine, centre, round) and is what the claims of
DESIGN.md 5.24 are checked with.  Below them a toy BFV on Python integers (keygen, encrypt, tensor, decrypt)."""
import numpy as np

import baseconv_util as B


def stages(a, P, ks, t, floor=False):
    """the two intermediate word arrays of the header's map, both [..., nm, n]: z (z_r = t x_r mod p_r on every row) and Yf (rows D
    hold Y_j = (z_j - r_j) Q^-1 mod p_j, rows S zero)"""
    a = np.asarray(a)
    nm = len(P)
    kd = nm - ks
    z = np.empty_like(a)
    for r in range(nm):
        z[..., r, :] = ((a[..., r, :].astype(object) * int(t)) % int(P[r])).astype(a.dtype)
    conv = B.baseconv_rns(z, P, (0, ks), (ks, kd), centered=not floor)
    Q = B.prod(P[:ks])
    Yf = np.zeros_like(a)
    for j in range(ks, nm):
        p = int(P[j])
        Yf[..., j, :] = (((z[..., j, :].astype(object) - conv[..., j, :].astype(object)) * pow(Q % p, -1, p)) % p).astype(a.dtype)
    return z, Yf


def scale_round_rns(a, P, ks, t, floor=False, keep=False):
    """the row formulas: [..., nm, n] -> the dense [..., ks, n], or with keep the dense [..., nm - ks, n] of the words Y"""
    nm = len(P)
    _, Yf = stages(a, P, ks, t, floor)
    if keep:
        return np.ascontiguousarray(Yf[..., ks:, :])
    out = B.baseconv_rns(Yf, P, (ks, nm - ks), (0, ks), centered=True)
    return np.ascontiguousarray(out[..., :ks, :])


def scale_round_exact(a, P, ks, t, floor=False, keep=False, keep1=None, keep2=None):
    """through the integer.  X_c the centred integer behind all rows; Y = round(t X_c / Q) -- Q is odd, so there is no tie -- or at
    the positions keep1 marks (those of the first band that kept z itself) floor(t X_c / Q); floor=True: floor(t X_c / Q) - u with
    the fast conversion's u.  keep: Y mod p_j on rows D.  Else the centred representative of Y mod B -- at the positions keep2
    marks, Y mod B itself -- reduced mod p_i on rows S."""
    a = np.asarray(a)
    nm = len(P)
    kd = nm - ks
    Q, Bp = B.prod(P[:ks]), B.prod(P[ks:])
    Xc = B.centre(B.crt_rows(a, P, (0, nm)), Q * Bp)
    tx = Xc * int(t)
    if floor:
        z, _ = stages(a, P, ks, t, floor=True)
        Y = tx // Q - B.parts(z, P, (0, ks))[1]
    else:
        c = B.centre(tx % Q, Q)
        if keep1 is not None:
            c = np.where(keep1, tx % Q, c)
        Y = (tx - c) // Q
    if keep:
        return B.rows_of(Y, P, range(ks, nm), a.dtype)
    y = Y % Bp
    val = B.centre(y, Bp)
    if keep2 is not None:
        val = np.where(keep2, y, val)
    return B.rows_of(val, P, range(ks), a.dtype)


def integers_to_rows(X, P, dtype):
    """residues of the integers X (object array [..., n], any sign) in every row of P: [..., nm, n]"""
    return B.rows_of(X, P, range(len(P)), dtype)


def plant_integers(a, P, values, b=0, first=0):
    """writes the integers `values` (any sign, reduced mod every p_r) into all rows of polynomial b at positions first, first + 1, ..."""
    for k, x in enumerate(values):
        for r, p in enumerate(P):
            a[b, r, first + k] = int(x) % int(p)
    return a


def first_round_values(P, ks, t, lb):
    """X whose z = t X mod Q runs over the edge and band values of rows S: X = z t^-1 mod Q (the rows D then hold X mod p_j)"""
    Q = B.prod(P[:ks])
    ti = pow(int(t), -1, Q)
    return [(z * ti) % Q for z in B.edge_values(P, (0, ks)) + B.band_values(P, (0, ks), lb)]


def second_round_values(P, ks, t, lb):
    """X = ceil(y Q / t) for y over the edge and band values of rows D (as centred integers): floor(t X / Q) = y exactly, and the
    fraction t X / Q - y is below t / Q < 1/2, so the rounding gives y too"""
    nm = len(P)
    Q, Bp = B.prod(P[:ks]), B.prod(P[ks:])
    out = []
    for y in B.edge_values(P, (ks, nm - ks)) + B.band_values(P, (ks, nm - ks), lb):
        yc = y - Bp if 2 * y >= Bp else y           # Y as a centred integer, so that |X| <= B Q / (2 t) + 1 stays inside Q B / 2
        out.append(-((-yc * Q) // int(t)))
    return out


# ---- a toy BFV on Python integers: R = Z[x] / (x^n + 1), ciphertext modulus Q, plaintext modulus t ----
def negacyclic(a, b):
    """the product of two integer coefficient lists in Z[x] / (x^n + 1)"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * y
                else:
                    out[k - n] -= x * y
    return out


def centred_list(v, Q):
    return [((int(x) % Q) - Q if 2 * (int(x) % Q) >= Q else int(x) % Q) for x in v]


def bfv_keygen(n, rnd):
    return [int(x) for x in rnd.randint(-1, 2, size=n)]   # ternary secret


def bfv_encrypt(m, s, Q, t, rnd):
    """(c0, c1) with c0 + c1 s = floor(Q / t) m + e mod Q, e in [-3, 3]"""
    n = len(s)
    a = [int(rnd.randint(0, 2**31)) * int(rnd.randint(0, 2**31)) * int(rnd.randint(0, 2**31)) % Q for _ in range(n)]
    e = [int(x) for x in rnd.randint(-3, 4, size=n)]
    as_ = negacyclic(a, s)
    c0 = [((Q // t) * int(mi) + ei - x) % Q for mi, ei, x in zip(m, e, as_)]
    return c0, a


def bfv_decrypt(cs, s, Q, t):
    """cs = (c0, c1[, c2]): round(t (c0 + c1 s + c2 s^2 mod Q, centred) / Q) mod t"""
    n = len(s)
    acc, sp = [0] * n, [1] + [0] * (n - 1)
    for c in cs:
        acc = [x + y for x, y in zip(acc, negacyclic(centred_list(c, Q), sp))]
        sp = negacyclic(sp, s)
    return [((2 * t * x + Q) // (2 * Q)) % t for x in centred_list(acc, Q)]


def bfv_tensor_integers(a, b, Q):
    """the tensor product over the integers of the centred lifts: (a0 b0, a0 b1 + a1 b0, a1 b1), coefficient lists of any sign"""
    a0, a1, b0, b1 = (centred_list(v, Q) for v in (a[0], a[1], b[0], b[1]))
    return negacyclic(a0, b0), [x + y for x, y in zip(negacyclic(a0, b1), negacyclic(a1, b0))], negacyclic(a1, b1)


def lists_to_rows(v, P, dtype):
    """an integer coefficient list -> [1, len(P), n] residues"""
    return integers_to_rows(np.array([v], dtype=object), P, dtype)


def rows_to_list(a, P):
    """[len(P), n] residues -> the integers in [0, prod P) behind them"""
    return [int(x) for x in B.crt_rows(np.asarray(a)[None], P, (0, len(P)))[0]]
