"""Python-integer restatement of the gadget decomposition (include/nflhip.h "gadget decomposition") -- what
tests/test_decompose_cpu.py and tests/test_gpu_decompose.py check against.  Moduli of `bits` = limb_bits - 2 bits, digit
width w, B = 2^w, l = ceil(bits / w), terms = nm * l; term j = m * l + t is digit t of row m:
    unsigned   d_t = (x >> w t) & (B - 1)
    signed     c = x if x <= (p - 1) / 2 else x - p;  r_0 = c;  t < l - 1: d_t = ((r_t + B/2) mod B) - B/2,
               r_(t+1) = (r_t - d_t) / B;  d_(l-1) = r_(l-1)
The digits are computed by the definition, step by step, on Python integers (never by the closed form the kernels use)."""
import numpy as np

_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
_COMPACT = {"i8": np.int8, "i16": np.int16, "i32": np.int32}


def nbits(limb_bits):
    return limb_bits - 2


def ndigits(limb_bits, w):
    return -(-nbits(limb_bits) // w)


def digits_of(x, p, w, l, signed):
    """the l digits of the canonical word x of a row with modulus p, as Python integers"""
    x, B = int(x), 1 << w
    if not signed:
        return [(x >> (w * t)) & (B - 1) for t in range(l)]
    r = x if x <= (p - 1) // 2 else x - p
    out = []
    for _ in range(l - 1):
        d = ((r + B // 2) % B) - B // 2
        out.append(d)
        assert (r - d) % B == 0
        r = (r - d) // B
    out.append(r)
    return out


def digit_polys(x, P, limb_bits, w, signed=False):
    """x = [batch, nm, n] words -> object array [batch, terms, n] of Python-integer digits"""
    x = np.asarray(x)
    batch, nm, n = x.shape
    l = ndigits(limb_bits, w)
    out = np.empty((batch, nm * l, n), dtype=object)
    B = 1 << w
    for m in range(nm):          # digits_of on whole rows: object arrays keep Python's integers, floor division and modulo
        p, r = int(P[m]), x[:, m, :].astype(object)
        if signed:
            r = np.where(r <= (p - 1) // 2, r, r - p)
        for t in range(l):
            if not signed:
                d = (r >> (w * t)) & (B - 1)
            elif t < l - 1:
                d = ((r + B // 2) % B) - B // 2
                r = (r - d) // B
            else:
                d = r
            out[:, m * l + t, :] = d
    return out


def decompose_ref(x, P, limb_bits, w, signed=False, fmt="words"):
    """the output of nflhip_decompose_dev in coefficient form: fmt "words" -> [batch * terms, nm, n] of the limb type, word
    (b, j, m', i) = d if d >= 0 else p_m' + d; fmt "i8" / "i16" / "i32" -> [batch * terms, n] signed integers"""
    d = digit_polys(x, P, limb_bits, w, signed)
    batch, terms, n = d.shape
    if fmt != "words":
        info = np.iinfo(_COMPACT[fmt])
        assert info.min <= d.min() and d.max() <= info.max
        return d.astype(np.int64).astype(_COMPACT[fmt]).reshape(batch * terms, n)
    out = np.empty((batch, terms, len(P), n), dtype=_NP[limb_bits])
    for m2, p in enumerate(P):
        spread = np.where(d < 0, d + int(p), d)
        assert 0 <= spread.min() and spread.max() < int(p)
        out[:, :, m2, :] = spread.astype(np.uint64).astype(_NP[limb_bits])
    return out.reshape(batch * terms, len(P), n)


def gadget_mul_ref(y, P, limb_bits, w):
    """[batch, nm, n] -> [batch * terms, nm, n]: term (m, t) holds y[m] * 2^(w t) mod p_m in row m, zeros elsewhere"""
    y = np.asarray(y)
    batch, nm, n = y.shape
    l = ndigits(limb_bits, w)
    out = np.zeros((batch, nm * l, nm, n), dtype=_NP[limb_bits])
    for m, p in enumerate(P):
        row = y[:, m, :].astype(object)
        for t in range(l):
            out[:, m * l + t, m, :] = ((row << (w * t)) % int(p)).astype(np.uint64).astype(_NP[limb_bits])
    return out.reshape(batch * nm * l, nm, n)


def edge_words(p, limb_bits, w):
    """the edge inputs of one row: 0, 1, (p-1)/2, (p+1)/2, p-1; 2^(wt) - 1, 2^(wt), 2^(wt) + 1 for every t; the words whose digits
    are all B/2 - 1, all B/2 and all B - 1 (the longest carry chains), reduced into [0, p) where they exceed it"""
    p, B, l = int(p), 1 << w, ndigits(limb_bits, w)
    vals = [0, 1, (p - 1) // 2, (p + 1) // 2, p - 1]
    for t in range(l):
        vals += [(1 << (w * t)) - 1, 1 << (w * t), (1 << (w * t)) + 1]
    for digit in (B // 2 - 1, B // 2, B - 1):
        v = sum(digit << (w * t) for t in range(l))
        vals += [v % p, v & ((1 << (nbits(limb_bits) - 1)) - 1)]   # (the second: the same digits below the top one, always < p)
    return [v % p for v in vals]


def edge_batch(P, n, limb_bits, w, batch, seed):
    """[B, nm, n] canonical words, B >= batch: random words with every edge word of every row planted among them (at random
    places; B grows past `batch` where the rows are too short to hold them all)"""
    rnd = np.random.RandomState(seed)
    need = max(len(edge_words(p, limb_bits, w)) for p in P)
    batch = max(batch, -(-need // n))
    out = np.empty((batch, len(P), n), dtype=_NP[limb_bits])
    for m, p in enumerate(P):
        e = edge_words(p, limb_bits, w)
        flat = rnd.randint(0, int(p), size=batch * n, dtype=np.int64).astype(_NP[limb_bits])
        flat[rnd.permutation(flat.size)[:len(e)]] = np.array(e, dtype=np.uint64).astype(_NP[limb_bits])
        out[:, m, :] = flat.reshape(batch, n)
    return out
