"""CPU-side checks of the modular arithmetic the kernel generators emit, ONE primitive at a time, at the limits of the input
ranges their docstrings state: tools/asmgen/arith.py (ct_bfly, gs_bfly, canon, final_bfly, pointwise), the base
multiplication of tools/asmgen/incomplete.py, and tools/gen_row1024_u32_asm.py (ct, gs, pointwise, last, base_mul).

Each primitive is emitted through the generators' own Emitter (hazard padding and operand order as shipped), followed by
s_endpgm, and executed by the interpreter of tests/asm_emu.py on one 64-lane wave whose registers hold the constants the
kernel prologues load from the ModConst record and one operand set per lane.  Two butterflies run interleaved on the two
temporary streams, as run_pairs schedules them.  Every result is checked against Python integers twice: it is congruent
to the exact operation, and it lies in the output range the docstring promises (the next stage's precondition).

Whole-kernel tests only reach these limits by chance: a two-bit fold lands in [p, p + 4 delta) with probability about
4 delta / 2^62.  Here the operands are placed there on purpose, on the moduli with the largest delta of each table.
"""
import os
import random
import sys
import zlib

import numpy as np
import pytest

import asm_emu
from nfllib_amd.params import params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

from asmgen import arith, incomplete  # noqa: E402
from asmgen import state as cfg  # noqa: E402
from asmgen.emitter import Emitter, interleave  # noqa: E402
import gen_row1024_u32_asm as g32  # noqa: E402

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
LANES = 64


# ------------------------------------------------------------------ harness
def emit(jobs):
    """the instruction text of up to two primitives, interleaved on streams 0 / 1 as run_pairs schedules them"""
    em = Emitter()
    interleave(em, [j(s) for s, j in enumerate(jobs)])
    return em.lines + ["\ts_endpgm"]


class Program:
    """one parsed listing, run on as many waves as there are operand sets"""

    def __init__(self, lines):
        self.prog, self.labels = asm_emu.parse_program("\n".join(lines))

    def run(self, vregs, sregs):
        w = asm_emu.Wave(self.prog, self.labels, asm_emu.Memory(), None, 0, 0, 0)
        for r, vals in vregs.items():
            w.v[r] = np.array([int(x) & M32 for x in vals], dtype=np.uint64)
        for r, val in sregs.items():
            w.s[r] = int(val) & M32
        for ev in w.run():
            raise AssertionError("an arithmetic primitive reached %s" % ev)
        return w


def put64(vregs, r, vals):
    vregs[r] = [x & M32 for x in vals]
    vregs[r + 1] = [(x >> 32) & M32 for x in vals]


def get64(w, r):
    return [int(lo) | (int(hi) << 32) for lo, hi in zip(w.v[r], w.v[r + 1])]


def get32(w, r):
    return [int(x) for x in w.v[r]]


def lanes(items):
    """split a list of per-lane records into waves of 64 (the last one padded with the first records)"""
    items = list(items)
    for i in range(0, len(items), LANES):
        chunk = items[i:i + LANES]
        yield chunk + items[:LANES - len(chunk)]


def sample(rng, values, ranges, per_range=3):
    """the edge values plus seeded random words in each sub-range [lo, hi)"""
    out = list(values)
    for lo, hi in ranges:
        out += [rng.randrange(lo, hi) for _ in range(per_range)]
    return out


# ------------------------------------------------------------------ 62-bit moduli: p = 2^62 - delta
U64_MODULI = (0, 1, 63, 91)
U32_MODULI = (0, 290)


class Mod64:
    def __init__(self, idx):
        prm = params(64)
        self.idx = idx
        self.p = p = int(prm.P[idx])
        self.delta = (1 << 62) - p
        assert 0 < self.delta < (1 << 32), "not a delta-form modulus"
        g = int(prm.primitive_roots[idx])
        self.n = 4096
        phi = pow(g, 1 << (prm.kmax_log2 - 12), p)     # primitive 2n-th root: the table of a 4096-word context
        assert pow(phi, self.n, p) == p - 1
        self.phi = phi
        self.ninv = int(prm.invkmax[idx]) * (prm.kmax // self.n) % p
        assert self.ninv * self.n % p == 1
        self.w1n = pow(phi, self.n // 2, p) * self.ninv % p
        self.fold_max = (1 << 62) + 3 * self.delta      # fold2's output bound: p + 4 delta
        self.edges_any = [0, 1, p - 1, p, 2 * p - 1, 2 * p, 4 * p - 1, self.fold_max - 1, M64]
        self.ranges_any = [(0, p), (p, 2 * p), (2 * p, 4 * p), (4 * p, 1 << 64), (p, self.fold_max)]
        self.edges_2p = [0, 1, p - 1, p, 2 * p - 1]
        self.ranges_2p = [(0, p), (p, 2 * p)]

    def shoup(self, w):
        return (w << 64) // self.p

    def twiddles(self, rng):
        """1, p - 1 (= -1) and entries of the context's table psi^k with their Shoup companions"""
        ws = [1, self.p - 1] + [pow(self.phi, rng.randrange(1, 2 * self.n), self.p) for _ in range(4)]
        return [(w, self.shoup(w)) for w in ws]

    def scalars(self, mu2=None):
        """the SGPRs the 62-bit kernels' prologue loads (tools/asmgen/block4096.py prologue)"""
        p = self.p
        s = {}
        for base, val in ((24, p), (26, 2 * p), (28, 3 * p), (32, (1 << 125) // p if mu2 is None else mu2),
                          (cfg.S_NINV[0], self.ninv), (cfg.S_NINVSH[0], self.shoup(self.ninv)),
                          (cfg.S_W1N[0], self.w1n), (cfg.S_W1NSH[0], self.shoup(self.w1n))):
            s[base], s[base + 1] = val & M32, val >> 32
        s[30], s[31], s[15] = self.delta, 0x3FFFFFFF, 0xC0000000
        return s

    def vconst(self):
        v = {cfg.V_PHI: [self.p >> 32] * LANES, arith.v_mask(): [0x3FFFFFFF] * LANES}
        for s in (0, 1):
            v[arith.T(s, 15)] = [0] * LANES            # the persistent zero behind the exact quotient's mul_hi
        return v


@pytest.fixture(scope="module", autouse=True)
def pair_map():
    cfg.configure("pair")
    yield


@pytest.fixture(params=U64_MODULI, ids=lambda i: "u64#%d" % i)
def m64(request):
    return Mod64(request.param)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


X0, Y0, X1, Y1 = cfg.V_A, cfg.V_A + 2, cfg.V_A + 4, cfg.V_A + 6
TW0, TW1 = cfg.V_TW, cfg.V_TW + 4


def _tw_strings(base):
    return tuple("v%d" % (base + k) for k in range(4))


def run_pairs64(m, program, combos):
    """combos: records (x, y, w, w') -- two per lane (streams 0 and 1); -> list of (record, x', y')"""
    out = []
    half = (len(combos) + 1) // 2
    pairs = list(zip(combos[:half], combos[half:] + combos[:1]))
    for chunk in lanes(pairs):
        v = m.vconst()
        for (xr, yr, tr), k in (((X0, Y0, TW0), 0), ((X1, Y1, TW1), 1)):
            put64(v, xr, [c[k][0] for c in chunk])
            put64(v, yr, [c[k][1] for c in chunk])
            put64(v, tr, [c[k][2] for c in chunk])
            put64(v, tr + 2, [c[k][3] for c in chunk])
        w = program.run(v, m.scalars())
        for k, (xr, yr) in enumerate(((X0, Y0), (X1, Y1))):
            out += [(c[k], x, y) for c, x, y in zip(chunk, get64(w, xr), get64(w, yr))]
    return out


def cross(xs, ys, tws):
    return [(x, y, w, wp) for x in xs for y in ys for (w, wp) in tws]


# ------------------------------------------------------------------ tools/asmgen/arith.py
def test_ct_bfly_takes_and_returns_any_word(m64):
    """x' = x + w y, y' = x - w y for ANY 64-bit x, y: fold2(x) + (one-off Shoup of y) < 2^62 + 3 delta + 3p = 2^64 exactly"""
    rng = random.Random(_seed(1, m64.idx))
    prog = Program(emit([arith.ct_bfly(X0, Y0, _tw_strings(TW0)), arith.ct_bfly(X1, Y1, _tw_strings(TW1))]))
    vals = sample(rng, m64.edges_any, m64.ranges_any, 2)
    p = m64.p
    for (x, y, w, _), xo, yo in run_pairs64(m64, prog, cross(vals, vals, m64.twiddles(rng))):
        assert (xo - (x + w * y)) % p == 0, (x, y, w)
        assert (yo - (x - w * y)) % p == 0, (x, y, w)


def test_gs_bfly_outputs_below_2p(m64):
    """x' = fold(x + y) < p + 4 delta, y' = (y - x) w with the EXACT Shoup quotient < 2p, for x, y < 2p"""
    rng = random.Random(_seed(2, m64.idx))
    prog = Program(emit([arith.gs_bfly(X0, Y0, _tw_strings(TW0)), arith.gs_bfly(X1, Y1, _tw_strings(TW1))]))
    vals = sample(rng, m64.edges_2p, m64.ranges_2p, 4)
    p = m64.p
    for (x, y, w, _), xo, yo in run_pairs64(m64, prog, cross(vals, vals, m64.twiddles(rng))):
        assert (xo - (x + y)) % p == 0 and xo < m64.fold_max, (x, y, w, xo)
        assert (yo - (y - x) * w) % p == 0, (x, y, w)
        assert yo < 2 * p, (x, y, w, yo)


def test_canon_maps_any_word_to_canonical(m64):
    rng = random.Random(_seed(3, m64.idx))
    prog = Program(emit([arith.canon(X0), arith.canon(X1)]))
    vals = sample(rng, m64.edges_any + [(1 << 62) - 1, 1 << 62, 3 << 62, (3 << 62) - 1], m64.ranges_any, 20)
    p = m64.p
    for (x, _, _, _), xo, _ in run_pairs64(m64, prog, [(x, 0, 0, 0) for x in vals]):
        assert xo == x % p, (x, xo)


def test_final_bfly_is_canonical(m64):
    """the last inverse stage with n^-1 folded in: x' = (x + y) / n, y' = (y - x) w1 / n, both in [0, p) for x, y < 2p"""
    rng = random.Random(_seed(4, m64.idx))
    prog = Program(emit([arith.final_bfly(X0, Y0), arith.final_bfly(X1, Y1)]))
    vals = sample(rng, m64.edges_2p, m64.ranges_2p, 4)
    p = m64.p
    for (x, y, _, _), xo, yo in run_pairs64(m64, prog, cross(vals, vals, [(0, 0)])):
        assert xo == (x + y) * m64.ninv % p, (x, y)
        assert yo == (y - x) * m64.w1n % p, (x, y)


@pytest.mark.parametrize("fold_a,fold_b", [(True, True), (True, False), (False, False)])
def test_pointwise_product(fold_a, fold_b, m64):
    """xa = fold2(xa xb mod p) < p + 4 delta: any word where the operand is folded first, canonical (< p) where it is not;
    the one-off Barrett quotient on th = T >> 61 with mu2 = floor(2^125 / p) keeps r below 4p"""
    rng = random.Random(_seed(5, m64.idx, fold_a, fold_b))
    prog = Program(emit([arith.pointwise(X0, Y0, fold_a, fold_b), arith.pointwise(X1, Y1, fold_a, fold_b)]))
    canon_vals = sample(rng, [0, 1, 2, m64.p - 2, m64.p - 1], [(0, m64.p)], 6)
    any_vals = sample(rng, m64.edges_any, m64.ranges_any, 2)
    p = m64.p
    combos = cross(any_vals if fold_a else canon_vals, any_vals if fold_b else canon_vals, [(0, 0)])
    for (x, y, _, _), xo, _ in run_pairs64(m64, prog, combos):
        assert (xo - x * y) % p == 0, (x, y)
        assert xo < m64.fold_max, (x, y, xo)


# ------------------------------------------------------------------ tools/asmgen/incomplete.py: base multiplication
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("negate", [False, True])
def test_incomplete_base_multiplication(G, negate, m64):
    """c = a b mod (X^G - zeta), zeta = +-w, on ANY 64-bit coefficients (the forward butterflies' outputs): G-term dot
    products of folded words accumulated in 128 bits (< 2^127), one Barrett step with mu = 2^65 + m (m < 2^35, the
    ModConst record of the incomplete kernels) -- every output < p + 4 delta"""
    p = m64.p
    mfield = (1 << 127) // p - (1 << 65)
    assert 0 <= mfield < (1 << 35)
    rng = random.Random(_seed(6, m64.idx, G, negate))
    a0, b0 = [cfg.V_A, cfg.V_A + 2 * G], [cfg.V_B, cfg.V_B + 2 * G]
    tws = [cfg.V_TW, cfg.V_TW + 4]
    rtmp, negtmp = [cfg.V_TW + 8, cfg.V_TW + 16], [cfg.V_TW + 24, cfg.V_TW + 28]
    prog = Program(emit([incomplete.base_mul(a0[s], b0[s], G, _tw_strings(tws[s]), negate, rtmp, negtmp) for s in (0, 1)]))
    vals = sample(rng, m64.edges_any, m64.ranges_any, 2)
    tw = m64.twiddles(rng)
    groups = []
    for v in vals:                                                 # uniform groups: every coefficient one edge value
        for u in (v, M64, 0):
            groups.append(([v] * G, [u] * G, tw[len(groups) % len(tw)]))
    for _ in range(6 * LANES):                                      # mixed groups from the edges and the sub-ranges
        groups.append(([rng.choice(vals) for _ in range(G)], [rng.choice(vals) for _ in range(G)], rng.choice(tw)))
    half = (len(groups) + 1) // 2
    for chunk in lanes(list(zip(groups[:half], groups[half:] + groups[:1]))):
        v = m64.vconst()
        for s in (0, 1):
            for i in range(G):
                put64(v, a0[s] + 2 * i, [c[s][0][i] for c in chunk])
                put64(v, b0[s] + 2 * i, [c[s][1][i] for c in chunk])
            put64(v, tws[s], [c[s][2][0] for c in chunk])
            put64(v, tws[s] + 2, [c[s][2][1] for c in chunk])
        w = prog.run(v, m64.scalars(mu2=mfield))
        for s in (0, 1):
            got = [get64(w, a0[s] + 2 * i) for i in range(G)]
            for lane, c in enumerate(chunk):
                a, b, (z, _) = c[s]
                zeta = p - z if negate else z
                for k in range(G):
                    want = sum(a[i] * b[k - i] for i in range(k + 1)) + zeta * sum(a[i] * b[k + G - i] for i in range(k + 1, G))
                    assert (got[k][lane] - want) % p == 0, (k, a, b, z)
                    assert got[k][lane] < m64.fold_max, (k, a, b, z, got[k][lane])


# ------------------------------------------------------------------ tools/gen_row1024_u32_asm.py: 30-bit moduli
class Mod32:
    def __init__(self, idx):
        prm = params(32)
        self.idx = idx
        self.p = p = int(prm.P[idx])
        assert p < (1 << 30)
        g = int(prm.primitive_roots[idx])
        self.n = 1024
        self.phi = pow(g, 1 << (prm.kmax_log2 - 10), p)
        assert pow(self.phi, self.n, p) == p - 1
        self.ninv = int(prm.invkmax[idx]) * (prm.kmax // self.n) % p
        self.w1n = pow(self.phi, self.n // 2, p) * self.ninv % p
        self.edges_4p = [0, 1, p - 1, p, 2 * p - 1, 2 * p, 4 * p - 1]
        self.ranges_4p = [(0, p), (p, 2 * p), (2 * p, 4 * p)]
        self.edges_2p = [0, 1, p - 1, p, 2 * p - 1]
        self.ranges_2p = [(0, p), (p, 2 * p)]

    def shoup(self, w):
        return (w << 32) // self.p

    def twiddles(self, rng):
        ws = [1, self.p - 1] + [pow(self.phi, rng.randrange(1, 2 * self.n), self.p) for _ in range(4)]
        return [(w, self.shoup(w)) for w in ws]

    def scalars(self, mu=None):
        """RowGen.constants: p, 2p, -p, mu (floor(2^60 / p); the incomplete kernels' record: floor(2^62 / p) - 2^32), n^-1 ..."""
        p = self.p
        return {g32.S_P: p, g32.S_2P: 2 * p, g32.S_NEGP: (1 << 32) - p, g32.S_MU: (1 << 60) // p if mu is None else mu,
                g32.S_NINV: self.ninv, g32.S_NINVSH: self.shoup(self.ninv), g32.S_W1N: self.w1n, g32.S_W1NSH: self.shoup(self.w1n)}

    def vconst(self):
        return {g32.V_P: [self.p] * LANES, g32.V_2P: [2 * self.p] * LANES}


@pytest.fixture(params=U32_MODULI, ids=lambda i: "u32#%d" % i)
def m32(request):
    return Mod32(request.param)


A0, B0, A1, B1 = g32.V_A, g32.V_A + 2, g32.V_A + 4, g32.V_A + 6
TWA0, TWA1 = g32.V_TWA, g32.V_TWA + 2


def emit32(jobs):
    em = Emitter()
    g32.run(em, jobs)
    return em.lines + ["\ts_endpgm"]


def run_pairs32(m, program, combos):
    """combos: records (x, y, w, w'), two per lane; -> list of (record, x', y') (low halves of the register pairs)"""
    out = []
    half = (len(combos) + 1) // 2
    pairs = list(zip(combos[:half], combos[half:] + combos[:1]))
    for chunk in lanes(pairs):
        v = m.vconst()
        for (xr, yr, tr), k in (((A0, B0, TWA0), 0), ((A1, B1, TWA1), 1)):
            v[xr] = [c[k][0] for c in chunk]
            v[yr] = [c[k][1] for c in chunk]
            v[xr + 1] = v[yr + 1] = [0xDEADBEEF] * LANES          # the high halves are scratch
            v[tr] = [c[k][2] for c in chunk]
            v[tr + 1] = [c[k][3] for c in chunk]
        w = program.run(v, m.scalars())
        for k, (xr, yr) in enumerate(((A0, B0), (A1, B1))):
            out += [(c[k], x, y) for c, x, y in zip(chunk, get32(w, xr), get32(w, yr))]
    return out


def _rec32(base):
    return "v%d" % base, "v%d" % (base + 1)


def test_u32_ct_harvey_ranges(m32):
    """x' = x + w y, y' = x - w y with x, y < 4p in and both < 4p out"""
    rng = random.Random(_seed(11, m32.idx))
    prog = Program(emit32([g32.ct(A0, B0, _rec32(TWA0)), g32.ct(A1, B1, _rec32(TWA1))]))
    vals = sample(rng, m32.edges_4p, m32.ranges_4p, 3)
    p = m32.p
    for (x, y, w, _), xo, yo in run_pairs32(m32, prog, cross(vals, vals, m32.twiddles(rng))):
        assert (xo - (x + w * y)) % p == 0 and (yo - (x - w * y)) % p == 0, (x, y, w)
        assert xo < 4 * p and yo < 4 * p, (x, y, w, xo, yo)


def test_u32_gs_outputs_below_2p(m32):
    rng = random.Random(_seed(12, m32.idx))
    prog = Program(emit32([g32.gs(A0, B0, _rec32(TWA0)), g32.gs(A1, B1, _rec32(TWA1))]))
    vals = sample(rng, m32.edges_2p, m32.ranges_2p, 5)
    p = m32.p
    for (x, y, w, _), xo, yo in run_pairs32(m32, prog, cross(vals, vals, m32.twiddles(rng))):
        assert (xo - (x + y)) % p == 0 and (yo - (y - x) * w) % p == 0, (x, y, w)
        assert xo < 2 * p and yo < 2 * p, (x, y, w, xo, yo)


def test_u32_last_stage_is_canonical(m32):
    rng = random.Random(_seed(13, m32.idx))
    prog = Program(emit32([g32.last(A0, B0), g32.last(A1, B1)]))
    vals = sample(rng, m32.edges_2p, m32.ranges_2p, 5)
    p = m32.p
    for (x, y, _, _), xo, yo in run_pairs32(m32, prog, cross(vals, vals, [(0, 0)])):
        assert xo == (x + y) * m32.ninv % p and yo == (y - x) * m32.w1n % p, (x, y)


def test_u32_pointwise_product(m32):
    """a = a b mod p in [0, 2p) for a, b < 4p (the forward butterflies' outputs): Barrett on th = T >> 28 with
    mu = floor(2^60 / p)"""
    rng = random.Random(_seed(14, m32.idx))
    prog = Program(emit32([g32.pointwise(A0, B0), g32.pointwise(A1, B1)]))
    vals = sample(rng, m32.edges_4p, m32.ranges_4p, 4)
    p = m32.p
    for (x, y, _, _), xo, _ in run_pairs32(m32, prog, cross(vals, vals, [(0, 0)])):
        assert (xo - x * y) % p == 0 and xo < 2 * p, (x, y, xo)


@pytest.mark.parametrize("negate", [False, True])
def test_u32_base_multiplication(negate, m32):
    """c = a b mod (X^4 - zeta) on operands < 4p: four-term sums below 2^62 in one carry-free chain, th = T >> 30,
    mu = floor(2^62 / p) = 2^32 + m, q - q^ <= 3 -- results < 2p in the high halves of a's pairs, zeta b_k (k > 0)
    canonical in b's registers"""
    p = m32.p
    mfield = (1 << 62) // p - (1 << 32)
    assert 0 <= mfield < (1 << 32)
    rng = random.Random(_seed(15, m32.idx, negate))
    prog = Program(emit32([g32.base_mul(0, _rec32(TWA0), negate), g32.base_mul(1, _rec32(TWA1), negate)]))
    vals = sample(rng, m32.edges_4p, m32.ranges_4p, 3)
    tw = m32.twiddles(rng)
    groups = []
    for v in vals:
        for u in (v, p - 1, 4 * p - 1):
            groups.append(([v] * 4, [u] * 4, tw[len(groups) % len(tw)]))
    for _ in range(6 * LANES):
        groups.append(([rng.choice(vals) for _ in range(4)], [rng.choice(vals) for _ in range(4)], rng.choice(tw)))
    half = (len(groups) + 1) // 2
    for chunk in lanes(list(zip(groups[:half], groups[half:] + groups[:1]))):
        v = m32.vconst()
        for g4 in (0, 1):
            for i in range(4):
                v[g32.V_A + 2 * (4 * g4 + i)] = [c[g4][0][i] for c in chunk]
                v[g32.V_B + 2 * (4 * g4 + i)] = [c[g4][1][i] for c in chunk]
                v[g32.V_A + 2 * (4 * g4 + i) + 1] = v[g32.V_B + 2 * (4 * g4 + i) + 1] = [0xDEADBEEF] * LANES
            v[TWA0 + 2 * g4] = [c[g4][2][0] for c in chunk]
            v[TWA0 + 2 * g4 + 1] = [c[g4][2][1] for c in chunk]
        w = prog.run(v, m32.scalars(mu=mfield))
        for g4 in (0, 1):
            got = [get32(w, g32.V_A + 2 * (4 * g4 + k) + 1) for k in range(4)]
            zb = [get32(w, g32.V_B + 2 * (4 * g4 + k)) for k in range(4)]
            for lane, c in enumerate(chunk):
                a, b, (z, _) = c[g4]
                zeta = p - z if negate else z
                for k in range(4):
                    want = sum(a[i] * b[k - i] for i in range(k + 1)) + zeta * sum(a[i] * b[k + 4 - i] for i in range(k + 1, 4))
                    assert (got[k][lane] - want) % p == 0, (k, a, b, z)
                    assert got[k][lane] < 2 * p, (k, a, b, z, got[k][lane])
                    if k:
                        assert zb[k][lane] == zeta * b[k] % p, (k, b, z)
