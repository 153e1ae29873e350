"""CPU: sums of ciphertext products with one relinearisation (include/nflhip.h "sums of ciphertext products").
The restatement tests validate the reference of tests/mulrelin_dot_util.py only -- they run no code of the library and pass without
the feature.  The binding, export and resource-report tests need the feature."""
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from level_util import mulrelin_level_rns
from mulrelin_dot_util import lazy_two_step, mulrelin_dot_rns, operand, tensor_dot_rns
from mulrelin_util import relin_key, tensor_rns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_tensor_dot_ntt_dev", "nflhip_tensor_dot_ntt", "nflhip_mulrelin_dot_ntt_dev", "nflhip_mulrelin_dot_ntt")


def _moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


# ---- the restatement: these validate the reference only and pass without the feature ----

@pytest.mark.parametrize("square", [False, True])
def test_tensor_dot_is_the_sum_of_the_tensor_products(square):
    """(reference only; passes without the feature)  u64/16/3, 2 groups of 5 terms, dense and shared b: tensor_dot_rns equals the sum
    over terms of mulrelin_util.tensor_rns, row by row"""
    P = _moduli(64, 3)
    groups, terms, n = 2, 5, 16
    blocks = [B.random_batch(P, n, groups * terms, np.uint64, 11 + t) for t in range(4)]
    for shared in (False, True):
        a0, a1 = (operand(x, groups, terms) for x in blocks[:2])
        b0, b1 = (None, None) if square else (operand(x[:terms] if shared else x, groups, terms, shared) for x in blocks[2:])
        got = tensor_dot_rns(a0, a1, b0, b1, P)
        want = [np.zeros((groups, 3, n), dtype=object) for _ in range(3)]
        for j in range(terms):
            d = tensor_rns(a0[:, j], a1[:, j], None if square else b0[:, j], None if square else b1[:, j], P)
            for w, x in zip(want, d):
                w += x.astype(object)
        for g, w in zip(got, want):
            for r, p in enumerate(P):
                assert np.array_equal(g[:, r].astype(object), w[:, r] % p), (square, shared, r)


@pytest.mark.parametrize("level", [4, 3, 2])
def test_identity_one_holds_for_sums(level, oracle_factory):
    """(reference only; passes without the feature)  u64/64/6, (K, alpha) = (2, 2), levels 4 (the top), 3 and 2, both mod-up modes and
    both roundings: the one mod-down with pi (.) D_c as the addend gives the words of D_c + key_switch_level(D2)_c.  Uniform operands
    and a uniform key; 2 groups of 3 terms; the squares as well; and at one term the words of level_util.mulrelin_level_rns."""
    lb, n, nm, K, alpha = 64, 64, 6, 2, 2
    P, orc = _moduli(lb, nm), oracle_factory(lb, n, nm)
    groups, terms = 2, 3
    blocks = [B.random_batch(P[:level], n, groups * terms, np.uint64, 60 + t) for t in range(4)]
    a0, a1, b0, b1 = (operand(x, groups, terms) for x in blocks)
    dnum = len(digits(nm, K, alpha))
    key = B.random_batch(P, n, 2 * dnum, np.uint64, 70).reshape(dnum, 2, nm, n)
    for centered in (False, True):
        for floor in (False, True):
            for bb in ((b0, b1), (None, None)):
                got = mulrelin_dot_rns(a0, a1, bb[0], bb[1], key, P, K, alpha, level, centered, floor, False, orc)
                want = lazy_two_step(a0, a1, bb[0], bb[1], key, P, K, alpha, level, centered, floor, orc)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (level, centered, floor, bb[0] is None)
    one = mulrelin_dot_rns(a0[:, :1], a1[:, :1], b0[:, :1], b1[:, :1], key, P, K, alpha, level, False, False, level >= 2, orc)
    ref = mulrelin_level_rns(a0[:, 0], a1[:, 0], b0[:, 0], b1[:, 0], key, P, K, alpha, level, False, False, level >= 2, orc)
    assert np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1])


def real_ciphertexts(P, K, alpha, n, terms, orc, seed):
    """a ternary secret s, the key from s^2 to s (|e| <= 8), `terms` pairs of uniform ciphertexts in one group on the L kept moduli, and
    the NTT rows of sum_j (a0_j + a1_j s)(b0_j + b1_j s)"""
    nm = len(P)
    L = nm - K
    rnd = np.random.RandomState(seed)
    s = rnd.randint(-1, 2, size=n).astype(object)
    S = orc.ntt(B.rows_of(s, P, range(nm), np.uint64)[None])[0].astype(object)
    S2 = np.empty_like(S)
    for j, p in enumerate(P):
        S2[j] = S[j] * S[j] % p
    key = relin_key(P, K, alpha, n, S, S2, orc, rnd)
    ops = [B.random_batch(P[:L], n, terms, np.uint64, seed + 1 + t)[None] for t in range(4)]   # (uniform words: any form)
    msg = np.empty((1, L, n), dtype=np.uint64)
    for j in range(L):
        x, y = (u[0, :, j].astype(object) + v[0, :, j].astype(object) * S[j] for u, v in ((ops[0], ops[1]), (ops[2], ops[3])))
        msg[0, j] = ((x * y).sum(axis=0) % P[j]).astype(np.uint64)
    return S, key, ops, msg


def phase_error(o0, o1, S, P, L, msg, ok):
    """|out0 + out1 s - msg|_inf over the kept moduli, centred"""
    r = np.empty_like(msg)
    for j in range(L):
        r[:, j] = ((o0[:, j].astype(object) + o1[:, j].astype(object) * S[j] - msg[:, j].astype(object)) % P[j]).astype(np.uint64)
    return max(abs(int(v)) for v in B.centre(B.crt_rows(ok.intt(r), P, (0, L)), B.prod(P[:L])).ravel())


@pytest.mark.parametrize("terms", [1, 5, 17])
def test_one_key_switch_error_for_the_whole_sum(terms, oracle_factory):
    """(reference only; passes without the feature)  u64/64/5, K = alpha = 2, a real key (ternary s, |e| <= 8, s' = s^2).  D0 + D1 s +
    D2 s^2 is the sum of the products exactly, so out0 + out1 s - sum_j (a0_j + a1_j s)(b0_j + b1_j s) is ONE key switch's error on D2:
    at most n dnum alpha 8 2^alpha + n + 1, whatever `terms` is.  The per-term way -- `terms` multiplications
    summed -- adds that error `terms` times and is allowed `terms` times the bound."""
    lb, n, nm, K, alpha = 64, 64, 5, 2, 2
    L = nm - K
    P, orc, ok = _moduli(lb, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K)
    S, key, (a0, a1, b0, b1), msg = real_ciphertexts(P, K, alpha, n, terms, orc, 900 + terms)
    bound = n * len(key) * alpha * 8 * 2**alpha + n + 1
    o0, o1 = mulrelin_dot_rns(a0, a1, b0, b1, key, P, K, alpha, L, False, False, False, orc)
    lazy = phase_error(o0, o1, S, P, L, msg, ok)
    s0, s1 = (np.zeros((1, L, n), dtype=object) for _ in range(2))
    for j in range(terms):
        t0, t1 = mulrelin_level_rns(a0[:, j], a1[:, j], b0[:, j], b1[:, j], key, P, K, alpha, L, False, False, False, orc)
        s0, s1 = s0 + t0.astype(object), s1 + t1.astype(object)
    per_term = phase_error(s0, s1, S, P, L, msg, ok)
    print("terms = %d: |out0 + out1 s - sum of products|_inf = %d lazily, %d term by term, bound %d" % (terms, lazy, per_term, bound))
    assert 0 < lazy <= bound
    assert 0 < per_term <= terms * bound


# ---- these need the feature ----

def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    for meth in ("tensor_dot_ntt", "h_tensor_dot_ntt", "tensor_dot_strided", "mul_relin_dot_ntt", "h_mul_relin_dot_ntt", "mul_relin_dot_strided"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    import ctypes as C
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(1024, dtype=np.uint64)
    p = [buf.ctypes.data + 1024 * k for k in range(8)]
    ops = [_lib.DotOperand(p[3 + k], 1, 1) for k in range(4)]
    r = [C.byref(o) for o in ops]
    assert L.nflhip_tensor_dot_ntt_dev(None, p[0], p[1], p[2], r[0], r[1], r[2], r[3], 1, 1, 1, 0, None) == _lib.ERR_INVALID == 1   # no device needed
    assert L.nflhip_tensor_dot_ntt(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 0, 1, 0) == _lib.ERR_INVALID
    assert L.nflhip_mulrelin_dot_ntt_dev(None, p[0], p[1], r[0], r[1], r[2], r[3], p[7], 1, 1, 1, 1, 1, 0, None) == _lib.ERR_INVALID
    assert L.nflhip_mulrelin_dot_ntt(None, p[0], p[1], p[3], p[4], p[5], p[6], p[7], 1, 1, 0, 1, 1, 1, 0) == _lib.ERR_INVALID


def test_compiled_kernel_uses_no_scratch_no_lds_and_spills_no_register(tmp_path):
    """the compiler's own resource report for every instance of k_tensor_dot_ntt (hipcc cross-compiles for gfx950 without a GPU): three
    limb widths x (16-byte groups, words) x (general, square).  No scratch memory, no LDS and no spilled register in any of the twelve;
    the vector registers are printed (the table of DESIGN.md 5.25)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_tensor_dot.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_tensor_dot.o")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name":
            cur = kernels.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    mine = {k: v for k, v in kernels.items() if "k_tensor_dot_ntt" in k}
    assert len(mine) == 12, sorted(kernels)
    for name, v in sorted(mine.items()):
        print(name, "VGPRs", v["VGPRs"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
        assert int(v["LDS Size [bytes/block]"]) == 0, name
