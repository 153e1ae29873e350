"""CPU: the gadget decomposition (include/nflhip.h "gadget decomposition").  The restatement of tests/decompose_util.py on a
hand-checked case, its reconstruction and digit ranges for every digit width of every limb width, the exhaustive check of the
top-digit bound at 14 bits, and the key-switching identity against the CPU oracle; the C ABI, the Python binding and the header
surface carry the new entry points.

The tests up to test_sum_of_digit_products_equals_the_oracles_polymul check the restatement itself, not the library: they tie the
reference every GPU test compares against to hand arithmetic and to the CPU oracle, and pass with or without the entry points.
The remaining tests need the entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

from decompose_util import (decompose_ref, digit_polys, digits_of, edge_batch, edge_words, gadget_mul_ref, nbits, ndigits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_decompose")
ENTRIES = ("nflhip_decompose_terms", "nflhip_decompose_dev", "nflhip_decompose", "nflhip_gadget_mul_dev")
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
OP_ADD, OP_MUL = 0, 2


def moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


def test_definition_on_a_small_case():
    # "16-bit limbs": 14-bit moduli, w = 5, B = 32, l = 3.  p = 15361 (the map needs no prime):
    # x = 12345 = 0b 01100 00001 11001 -> unsigned digits 25, 1, 12  (25 + 1 * 32 + 12 * 1024 = 12345)
    # signed: x > (p - 1) / 2 = 7680, c = 12345 - 15361 = -3016.  r0 = -3016: (r0 + 16) mod 32 = -3000 mod 32 = 8 -> d0 = 8 - 16 = -8,
    #   r1 = (-3016 + 8) / 32 = -94;  (r1 + 16) mod 32 = -78 mod 32 = 18 -> d1 = 2, r2 = (-94 - 2) / 32 = -3;  d2 = -3 (the top digit)
    #   -8 + 2 * 32 - 3 * 1024 = -3016
    assert digits_of(12345, 15361, 5, 3, False) == [25, 1, 12]
    assert digits_of(12345, 15361, 5, 3, True) == [-8, 2, -3]
    # x = 7680 = (p - 1) / 2 stays positive: 7680 = 0b 00111 10000 00000.  d0 = 0; r1 = 240: (240 + 16) mod 32 = 0 -> d1 = -16,
    #   r2 = (240 + 16) / 32 = 8;  d2 = 8.   0 - 16 * 32 + 8 * 1024 = 7680
    assert digits_of(7680, 15361, 5, 3, True) == [0, -16, 8]
    assert digits_of(7681, 15361, 5, 3, True) == [0, -16, -7]          # c = -7680: r1 = -240, d1 = -16, r2 = (-240 + 16) / 32 = -7
    # two rows (p = 15361, 13313), one position each; words output spreads a negative digit as p_m' + d
    P = [15361, 13313]
    x = np.array([[[12345], [5]]], dtype=np.uint16)
    got = decompose_ref(x, P, 16, 5, signed=True)
    assert got.shape == (6, 2, 1)
    assert got[:, :, 0].tolist() == [[15361 - 8, 13313 - 8], [2, 2], [15361 - 3, 13313 - 3], [5, 5], [0, 0], [0, 0]]
    assert decompose_ref(x, P, 16, 5, signed=True, fmt="i8")[:, 0].tolist() == [-8, 2, -3, 5, 0, 0]
    assert decompose_ref(x, P, 16, 5)[:, :, 0].tolist() == [[25, 25], [1, 1], [12, 12], [5, 5], [0, 0], [0, 0]]
    g = gadget_mul_ref(x, P, 16, 5)
    assert g[:, :, 0].tolist() == [[12345, 0], [12345 * 32 % 15361, 0], [12345 * 1024 % 15361, 0], [0, 5], [0, 160], [0, 5120]]


@pytest.mark.parametrize("lb", [16, 32, 64])
def test_reconstruction_and_digit_ranges_for_every_width(lb):
    bits = nbits(lb)
    P = moduli(lb, 2)
    for w in range(1, bits):
        l, B = ndigits(lb, w), 1 << w
        assert w * (l - 1) <= bits - 1 and w * l >= bits                     # 2^(w t) < p for every t < l
        for p in P:
            assert (1 << (w * (l - 1))) < p
            for x in edge_words(p, lb, w) + [int(v) for v in np.random.RandomState(w).randint(0, 1 << 30, size=8) % p]:
                assert 0 <= x < p
                u, s = digits_of(x, p, w, l, False), digits_of(x, p, w, l, True)
                assert sum(d << (w * t) for t, d in enumerate(u)) == x
                assert all(0 <= d < B for d in u)
                c = x if x <= (p - 1) // 2 else x - p
                assert sum(d * (1 << (w * t)) for t, d in enumerate(s)) == c and (c - x) % p == 0
                assert all(-B // 2 <= d < B // 2 for d in s[:-1])
                assert abs(s[-1]) <= B // 2                                    # the top digit takes the carry
                assert abs(s[-1]) < p                                          # ... and is below every modulus (w <= bits - 1)


def test_top_digit_bound_exhaustively_at_14_bits():
    p = moduli(16, 1)[0]
    assert p.bit_length() == 14
    x = np.arange(p, dtype=np.uint16).reshape(1, 1, p)
    for w in range(1, 14):
        l, B = ndigits(16, w), 1 << w
        d = digit_polys(x, [p], 16, w, signed=True)
        assert d.shape == (1, l, p)
        for t in range(l - 1):
            assert -B // 2 <= d[0, t].min() and d[0, t].max() < B // 2
        assert -B // 2 <= d[0, l - 1].min() and d[0, l - 1].max() <= B // 2
        c = np.where(x[0, 0].astype(object) <= (p - 1) // 2, x[0, 0].astype(object), x[0, 0].astype(object) - p)
        assert np.array_equal(sum(d[0, t] * (1 << (w * t)) for t in range(l)), c)


def test_row_version_equals_the_scalar_definition():
    P = moduli(64, 2)
    x = edge_batch(P, 64, 64, 20, 1, 3)
    for signed in (False, True):
        d = digit_polys(x, P, 64, 20, signed)
        l = ndigits(64, 20)
        for m, p in enumerate(P):
            for i in range(64):
                assert [d[0, m * l + t, i] for t in range(l)] == digits_of(x[0, m, i], p, 20, l, signed)


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 2), (32, 64, 3), (16, 128, 2)])
@pytest.mark.parametrize("signed", [False, True])
def test_sum_of_digit_products_equals_the_oracles_polymul(lb, n, nm, signed, oracle_factory):
    """sum_j NTT(D_j(x)) (.) NTT(G_j(y)), inverse-transformed, equals the oracle's polymul(x, y) bit for bit"""
    P, o = moduli(lb, nm), oracle_factory(lb, n, nm)
    bits = nbits(lb)
    for w in sorted({1, min(7, bits - 1), min(20, bits - 1), bits - 1}):
        x = edge_batch(P, n, lb, w, 1, 5 + w)[:2]
        y = np.ascontiguousarray(o.fill_uniform(len(x), 9, 1))
        D = o.ntt(decompose_ref(x, P, lb, w, signed))
        G = o.ntt(gadget_mul_ref(y, P, lb, w))
        terms = nm * ndigits(lb, w)
        acc = np.zeros_like(x)
        for j in range(terms):
            prod = o.pointwise(OP_MUL, np.ascontiguousarray(D[j::terms]), np.ascontiguousarray(G[j::terms]))
            acc = o.pointwise(OP_ADD, acc, prod)
        assert np.array_equal(o.intt(acc), o.polymul(x, y)), (w, signed)


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_DECOMP_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in ("SIGNED", "COMPOSED", "FUSED")}
    assert len(set(flags.values())) == 3 and all(v & (v - 1) == 0 and v > 1 for v in flags.values())   # single bits, clear of NFLHIP_FORM_*
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert (_lib.DECOMP_SIGNED, _lib.DECOMP_COMPOSED, _lib.DECOMP_FUSED) == (flags["SIGNED"], flags["COMPOSED"], flags["FUSED"])
    for meth in ("decompose", "h_decompose", "gadget_mul", "decompose_terms"):
        assert callable(getattr(Engine, meth))
    hdr = open(os.path.join(ROOT, "include", "nfl_hip", "poly_p.hpp")).read() + open(os.path.join(ROOT, "include", "nfl_hip", "batch.hpp")).read()
    for name in ("gadget_terms", "decompose", "decompose_ntt", "gadget_mul", "assign_decompose", "assign_gadget_mul"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    assert L.nflhip_decompose_dev(None, p, 0, p + 256, 1, 8, 0, None) == _lib.ERR_INVALID == 1     # NULL context: no device needed
    assert L.nflhip_decompose_dev(None, p, 0, p + 256, 1, 0, 0, None) == _lib.ERR_INVALID          # ... and w = 0
    assert L.nflhip_decompose(None, p, 0, p + 256, 1, 8, 0) == _lib.ERR_INVALID
    assert L.nflhip_gadget_mul_dev(None, p, p + 256, 1, 8, None) == _lib.ERR_INVALID
    assert L.nflhip_decompose_terms(None, 8) == 0
    assert not buf.any()


def build_cpp(out_dir, eager=False):
    """the C++ program of tests/cpp_decompose, two translation units, with the g++ line of tests/cpp/Makefile"""
    exe = os.path.join(out_dir, "decompose_test" + ("_eager" if eager else ""))
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-DNFL_HIP_NO_GMP"]
    if eager:
        cmd.append("-DNFL_HIP_EAGER")
    cmd += ["-o", exe, os.path.join(SRC, "decompose_main.cpp"), os.path.join(SRC, "decompose_tu2.cpp"),
            "-L" + os.path.join(ROOT, "nfllib_amd"), "-lnflhip", "-Wl,-rpath," + os.path.join(ROOT, "nfllib_amd"),
            "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu(), reason="CPU-only behaviour")
def test_cpp_program_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build_cpp(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout[-2000:]
