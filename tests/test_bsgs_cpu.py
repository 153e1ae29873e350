"""CPU: BSGS slot linear transforms and the several-output weighted sum of automorphisms (include/nflhip.h "BSGS slot linear
transforms", "weighted sums of automorphisms into several outputs").
  * the C ABI, the Python binding and the Engine carry the new names; a NULL context is refused without a device;
  * the restatement of tests/bsgs_util.py against the restatements it extends (these two validate the reference only);
  * a REAL baby-step giant-step product on that restatement alone: with Galois keys of the header's convention and ternary diagonals,
    out0 + out1 s is sum_j sigma_{g_j}(sum_i pt_{j,i} sigma_{b_i}(c0 + c1 s)) up to the noise the mathematics allows, and no more than
    today's way (a linear transform per giant step, a keyed rotation of each, additions) leaves beyond its roundings;
  * the compiler's resource report for every kernel instance of kernels_bsgs.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from automorph_util import sigma_ntt
from bsgs_util import bsgs_rns, mac_multi_rns
from keyswitch_util import digits
from lintrans_util import lintrans_rns, mac_rns, reduce_rows
from test_level_cpu import _demangled, _resource_report
from test_rotate_cpu import _rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_automorphism_mac_multi_dev", "nflhip_automorphism_mac_multi", "nflhip_bsgs_ntt_dev", "nflhip_bsgs_ntt")
FLAGS = {"CENTERED": 0x100, "FLOOR": 0x200, "SEQUENCE": 0x1000, "HOISTED": 0x2000}
MAP = ("U_d      the mod-up of c1, every digit",
       "S_{i,c}  = sum_d U_d (.) bkeys[i][d][c]",
       "V_{j,c} = sum_{keyed i} w_{j,i} (.) sigma^NTT_{b_i}(S_{i,c})",
       "W_{j,0} = sum_{all i}   w_{j,i} (.) sigma^NTT_{b_i}(c0)",
       "W_{j,1} = sum_{unkeyed i} w_{j,i} (.) c1",
       "v_j     = mod-down(V_{j,1}) + W_{j,1}",
       "T_{j,c} = sum_d mod-up(v_j)_d (.) gkeys[j][d][c]",
       "A_0 += sigma^NTT_{g_j}(V_{j,0} + T_{j,0});   A_1 += sigma^NTT_{g_j}(T_{j,1});   O_0 += sigma^NTT_{g_j}(W_{j,0})",
       "A_c += V_{j,c};   O_0 += W_{j,0};   O_1 += W_{j,1}",
       "out_c = mod-down(A_c) + O_c",
       "out_o[g][r][x] = addend_o[g][r][x] + sum_{t < terms} w_{o,t}[r][x] * in_t[g][r][src_{k_t}(x)]")


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code                                 # entries are added, the number stays
    flags = {k: int(re.search(r"#define\s+NFLHIP_BSGS_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in FLAGS}
    assert flags == FLAGS
    for name in ("NFLHIP_BSGS_MAX_BABY", "NFLHIP_BSGS_MAX_GIANT", "NFLHIP_MAC_MULTI_MAX_OUTPUTS"):
        assert re.search(r"#define\s+%s\s+16\b" % name, code), name
    for line in MAP:
        assert line in txt, line
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert {k: getattr(_lib, "BSGS_" + k) for k in FLAGS} == FLAGS
    assert _lib.BSGS_MAX_BABY == 16 and _lib.BSGS_MAX_GIANT == 16 and _lib.MAC_MULTI_MAX_OUTPUTS == 16
    for meth in ("automorphism_mac_multi", "h_automorphism_mac_multi", "bsgs_linear_transform_ntt", "h_bsgs_linear_transform_ntt"):
        assert callable(getattr(Engine, meth)), meth


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(1024, dtype=np.uint64)
    p = buf.ctypes.data
    one = lambda x: (C.c_void_p * 1)(x)                                          # noqa: E731
    ks = (C.c_uint64 * 1)(5)
    assert L.nflhip_automorphism_mac_multi_dev(None, one(p), None, one(p + 512), one(p + 1024), ks, 1, 1, 1, 1, 0, None) == _lib.ERR_INVALID == 1
    assert L.nflhip_automorphism_mac_multi(None, one(p), None, one(p + 512), one(p + 1024), ks, 1, 1, 1, 1, 0) == _lib.ERR_INVALID
    for level in (0, 1, 2**64 - 1):
        for flags in (0, _lib.BSGS_SEQUENCE, _lib.BSGS_HOISTED | _lib.BSGS_CENTERED):
            assert L.nflhip_bsgs_ntt_dev(None, p, p + 64, None, p + 128, one(p + 256), ks, 1, one(p + 2048), ks, 1, one(p + 4096), 1, 1, 1, level, flags,
                                         None) == _lib.ERR_INVALID
            assert L.nflhip_bsgs_ntt(None, p, p + 64, None, p + 128, one(p + 256), ks, 1, one(p + 2048), ks, 1, one(p + 4096), 1, 1, 1, level,
                                     flags) == _lib.ERR_INVALID


# ---- the reference: these two validate tests/bsgs_util.py and would pass without the feature ----
def test_the_restated_primitive_is_mac_rns_per_output():
    """VALIDATES THE REFERENCE ONLY.  u64/16/3 words below the moduli: every output of mac_multi_rns is mac_rns over its non-None
    weights, an output without a weight is its addend or zero"""
    from nfllib_amd.params import params
    n, nm = 16, 3
    P = [int(v) for v in params(64).P[:nm]]
    ins = [B.random_batch(P, n, 2, np.uint64, 3 + t) for t in range(3)]
    ws = [[B.random_batch(P, n, 1, np.uint64, 20 + 3 * o + t)[0] for t in range(3)] for o in range(4)]
    ws[1][0] = ws[2][1] = ws[2][2] = None
    ws[3] = [None] * 3
    adds = [None, B.random_batch(P, n, 2, np.uint64, 40), None, B.random_batch(P, n, 2, np.uint64, 41)]
    ks = [5, 1, 2 * n - 1]
    got = mac_multi_rns(ins, ws, ks, P, addends=adds)
    assert np.array_equal(got[0], mac_rns(ins, ws[0], ks, P))
    assert np.array_equal(got[1], mac_rns(ins[1:], ws[1][1:], ks[1:], P, addend=adds[1]))
    assert np.array_equal(got[2], mac_rns(ins[:1], ws[2][:1], ks[:1], P))
    assert np.array_equal(got[3], adds[3])
    assert np.array_equal(mac_multi_rns(ins, [[None] * 3], ks, P)[0], np.zeros_like(ins[0]))


@pytest.mark.parametrize("centered,floor", [(False, False), (True, True)])
def test_one_unkeyed_giant_step_is_the_linear_transform(centered, floor, oracle_factory):
    """VALIDATES THE REFERENCE ONLY.  u64/64/5 (2, 2): bsgs_rns with n2 = 1 and the unrotated giant step is lintrans_rns word for word,
    with keyed and unkeyed babies, with and without c0"""
    from nfllib_amd.params import params
    lb, n, nm, K, alpha = 64, 64, 5, 2, 2
    L = nm - K
    P = [int(v) for v in params(lb).P[:nm]]
    orc, ok = oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    dnum = len(digits(nm, K, alpha))
    c0, c1 = (ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed)) for seed in (5, 6))
    keys = [B.random_batch(P, n, 2 * dnum, np.uint64, 100 + i).reshape(dnum, 2, nm, n) for i in range(2)]
    ws = [B.random_batch(P, n, 1, np.uint64, 200 + i)[0] for i in range(4)]
    for bkeys, ks in (([keys[0], None, keys[1], None], [5, 1, 25, 2 * n + 1]), ([keys[0]], [7]), ([None], [1])):
        for a0 in (c0, None):
            want = lintrans_rns(a0, c1, bkeys, ws[:len(ks)], ks, P, K, alpha, centered, floor, orc, ok)
            got = bsgs_rns(a0, c1, bkeys, ks, [None], [1], [ws[:len(ks)]], P, K, alpha, centered, floor, orc, ok)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (ks, a0 is None)


def _galois_key(P, K, alpha, n, S_ntt, k, orc, rnd, seed):
    """the header's convention: from s to sigma_(k^-1)(s) -- key[d][0] = -a_d sigma_(k^-1)(s) + e_d + P g_d s, key[d][1] = a_d, |e| <= 8"""
    nm = len(P)
    L = nm - K
    Q, Ps = B.prod(P[:L]), B.prod(P[L:])
    Sd = digits(nm, K, alpha)
    Sinv = sigma_ntt(S_ntt, pow(k, -1, 2 * n)).astype(object)
    key = np.empty((len(Sd), 2, nm, n), dtype=np.uint64)
    for d, (s0, kd) in enumerate(Sd):
        Qd = B.prod(P[s0:s0 + kd])
        g = (Q // Qd) * pow((Q // Qd) % Qd, -1, Qd)
        a = B.random_batch(P, n, 1, np.uint64, seed + d)[0]
        e = orc.ntt(_rows(rnd.randint(-8, 9, size=n).astype(object), P, np.uint64)[None])[0]
        for j, p in enumerate(P):
            key[d, 0, j] = ((e[j].astype(object) - a[j].astype(object) * Sinv[j] + (Ps * g) % p * S_ntt[j].astype(object)) % p).astype(np.uint64)
        key[d, 1] = a
    return key


CASES = [(K, alpha, centered, [1, 5, 25], [1, 125, 127]) for K, alpha in ((1, 1), (2, 2), (2, 1)) for centered in (False, True)]
CASES += [(2, 2, False, [1], [125, 127]), (2, 2, False, [5, 25], [1])]


@pytest.mark.parametrize("K,alpha,centered,bks,gks", CASES)
def test_the_definition_is_a_bsgs_product(K, alpha, centered, bks, gks, oracle_factory):
    """u64/64/5, ternary s, key noise |e| <= 8, ternary diagonals (T = 1), batch 2; a step with k = 1 has no key.  Every baby's
    key-switch noise meets one diagonal per giant step, every keyed giant adds one key switch and one inner rounding r_j s / P, and
    there is one final rounding:
        0 < | out0 + out1 s - sum_j sigma_{g_j}(sum_i pt_{j,i} sigma_{b_i}(c0 + c1 s)) |_inf <= n2 kb n T B + kg B + (kg + 1)(n + 1),
    B = n dnum alpha 8 2^alpha + n + 1 (tests/test_rotate_cpu.py).  "prev" is today's way: one lintrans_rns per giant step, then
    lintrans_rns with one keyed term and the NTT form of the constant 1 as weight, then additions; its key-switch noises are the same
    and only the roundings differ, so the residue is at most prev + (n2 + kg + 1)(n + 1).  Measured, BSGS (prev)
    against the bound, fast / centred:
        K 1 alpha 1:  1256 / 1192  (1261 / 1191)  1606341
        K 2 alpha 2:  2336 /  474  (2340 /  464)  3187397
        K 2 alpha 1:     9 /   10  (  11 /   11)  1211077
        K 2 alpha 2, fast, one unkeyed baby and two keyed giants:  106 (109)  16709;  two keyed babies and one unkeyed giant:  599 (599)  1056961"""
    from nfllib_amd.params import params
    lb, n, nm, T = 64, 64, 5, 1
    L = nm - K
    P = [int(v) for v in params(lb).P[:nm]]
    orc, ok = oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    rnd = np.random.RandomState(3000 * K + 30 * alpha + centered + 7 * len(bks))
    Q = B.prod(P[:L])
    dnum = len(digits(nm, K, alpha))
    n1, n2 = len(bks), len(gks)
    s = rnd.randint(-1, 2, size=n).astype(object)
    S_ntt = orc.ntt(_rows(s, P, np.uint64)[None])[0]
    bkeys = [None if k == 1 else _galois_key(P, K, alpha, n, S_ntt, k, orc, rnd, 7 + 10 * i) for i, k in enumerate(bks)]
    gkeys = [None if k == 1 else _galois_key(P, K, alpha, n, S_ntt, k, orc, rnd, 307 + 10 * j) for j, k in enumerate(gks)]
    kb, kg = sum(k is not None for k in bkeys), sum(k is not None for k in gkeys)
    weights = [[orc.ntt(_rows(rnd.randint(-T, T + 1, size=n).astype(object), P, np.uint64)[None])[0] for _ in bks] for _ in gks]
    c0, c1 = (ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed)) for seed in (5, 6))
    So = S_ntt.astype(object)

    def add(x, y):
        return reduce_rows(x.astype(object) + y.astype(object), P[:L], np.uint64)

    def residue(out0, out1):
        msg = np.empty_like(c0)                                                   # c0 + c1 s
        for j in range(L):
            msg[:, j] = ((c0[:, j].astype(object) + c1[:, j].astype(object) * So[j]) % P[j]).astype(np.uint64)
        want = np.zeros_like(c0)
        for j in range(n2):
            want = add(want, sigma_ntt(mac_rns([msg] * n1, weights[j], bks, P[:L]), gks[j]))
        r = np.empty_like(c0)
        for j in range(L):
            r[:, j] = ((out0[:, j].astype(object) + out1[:, j].astype(object) * So[j] - want[:, j].astype(object)) % P[j]).astype(np.uint64)
        return max(abs(int(v)) for v in B.centre(B.crt_rows(ok.intt(r), P, (0, L)), Q).ravel())

    norm = residue(*bsgs_rns(c0, c1, bkeys, bks, gkeys, gks, weights, P, K, alpha, centered, False, orc, ok))
    one = orc.ntt(_rows(np.array([1] + [0] * (n - 1), dtype=object), P, np.uint64)[None])[0]
    p0, p1 = np.zeros_like(c0), np.zeros_like(c0)
    for j in range(n2):
        a0, a1 = lintrans_rns(c0, c1, bkeys, weights[j], bks, P, K, alpha, centered, False, orc, ok)
        if gkeys[j] is not None:
            a0, a1 = lintrans_rns(a0, a1, [gkeys[j]], [one], [gks[j]], P, K, alpha, centered, False, orc, ok)
        p0, p1 = add(p0, a0), add(p1, a1)
    prev = residue(p0, p1)
    Bk = n * dnum * alpha * 8 * 2**alpha + n + 1
    bound = n2 * kb * n * T * Bk + kg * Bk + (kg + 1) * (n + 1)
    print("K %d alpha %d centred %d babies %s giants %s: residue %d (prev %d), bound %d" % (K, alpha, centered, bks, gks, norm, prev, bound))
    assert 0 < norm <= bound
    assert norm <= prev + (n2 + kg + 1) * (n + 1)


def test_new_kernel_instances_use_no_scratch_and_spill_no_register(tmp_path):
    """every kernel of kernels_bsgs.hip (hipcc cross-compiles for gfx950 without a GPU): k_permute_mac_multi_ntt with JB = 2 outputs per
    launch, three limb widths x (16-byte groups, words) x (dense, level diagonals); the weightless k_permute_sum_ntt, three limb widths
    x (16-byte groups, words).  No scratch, no spilled register, vector or scalar; the LDS is sized at launch.  (JB = 4 spills scalar
    registers in 10 of its 12 instances and is not shipped: DESIGN.md 5.23.)"""
    kernels = _resource_report(tmp_path, "kernels_bsgs")
    names = _demangled(kernels)
    multi = {k: v for k, v in kernels.items() if "k_permute_mac_multi_ntt<" in names[k]}
    level = {k for k in multi if "MacMultiTermsLevel" in names[k]}
    psum = {k: v for k, v in kernels.items() if "k_permute_sum_ntt<" in names[k]}
    assert len(multi) == 12 and len(level) == 6 and len(psum) == 6 and len(kernels) == 18, sorted(names.values())
    assert all(re.search(r"k_permute_mac_multi_ntt<[^,]+, (true|false), 2, ", names[k]) for k in multi)
    for name, v in sorted(kernels.items()):
        print(names[name].split("(")[0], "VGPRs", v["VGPRs"], "SGPRs", v["TotalSGPRs"], "LDS", v["LDS Size [bytes/block]"], "Occupancy",
              v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
        assert int(v["LDS Size [bytes/block]"]) == 0, name                        # extern __shared__: sized at launch
