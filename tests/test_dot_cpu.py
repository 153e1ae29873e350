"""CPU: sums of products across polynomials (include/nflhip.h "sums of products").  The restatement of tests/dot_util.py on a
hand-checked case and against a chain of the CPU oracle's point-wise multiply and add; the C ABI, the Python binding and the
header surface carry the three new entry points.

test_definition_on_a_small_case and test_restatement_equals_a_chain_of_oracle_multiplies_and_adds check the restatement itself,
not the library: they tie the reference every GPU test compares against to hand arithmetic and to the CPU oracle, and pass
with or without the entry points.  The remaining tests need the entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

from dot_util import dot_ref, edge_polys, full_polys, random_polys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_dot")
ENTRIES = ("nflhip_dot_dev", "nflhip_dot_ptrs_dev", "nflhip_dot")
SHAPES = [(16, 128, 2), (32, 1024, 3), (64, 64, 4), (64, 1024, 94)]
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
OP_ADD, OP_MUL = 0, 2


def moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


def test_definition_on_a_small_case():
    # moduli 5, 7; two groups of three terms, one position per row.
    #   group 0, row 0 (mod 5): 2*3 + 4*4 + 1*0 = 22 = 2;  with addend 4: 26 = 1
    #   group 0, row 1 (mod 7): 6*6 + 5*2 + 3*3 = 55 = 6;  with addend 6: 61 = 5
    #   group 1, row 0 (mod 5): 4*4 + 4*4 + 4*4 = 48 = 3;  with addend 0: 3
    #   group 1, row 1 (mod 7): 0*1 + 1*0 + 6*6 = 36 = 1;  with addend 1: 2
    P = [5, 7]
    a = np.array([[[[2], [6]], [[4], [5]], [[1], [3]]], [[[4], [0]], [[4], [1]], [[4], [6]]]], dtype=np.uint64)
    b = np.array([[[[3], [6]], [[4], [2]], [[0], [3]]], [[[4], [1]], [[4], [0]], [[4], [6]]]], dtype=np.uint64)
    add = np.array([[[4], [6]], [[0], [1]]], dtype=np.uint64)
    assert a.shape == (2, 3, 2, 1)
    assert dot_ref(a, b, P).tolist() == [[[2], [6]], [[3], [1]]]
    assert dot_ref(a, b, P, add).tolist() == [[[1], [5]], [[3], [2]]]
    # a shared second operand: group 1 against group 0's b.  row 0: 4*3 + 4*4 + 4*0 = 28 = 3; row 1: 0*6 + 1*2 + 6*3 = 20 = 6
    assert dot_ref(a, b[0], P)[1].tolist() == [[3], [6]]
    assert dot_ref(a, b, P, rows=[1]).tolist() == [[[6]], [[1]]]


@pytest.mark.parametrize("lb,n,nm", SHAPES)
def test_restatement_equals_a_chain_of_oracle_multiplies_and_adds(lb, n, nm, oracle_factory):
    P = moduli(lb, nm)
    o = oracle_factory(lb, n, nm)
    groups, terms = (1, 3) if nm > 8 else (3, 5)
    a = edge_polys(P, n, groups * terms, _NP[lb], 3).reshape(groups, terms, nm, n)
    b = random_polys(P, n, groups * terms, _NP[lb], 4).reshape(groups, terms, nm, n)
    b[:, 1] = full_polys(P, n, groups, _NP[lb])            # (p - 1)^2 where a's second polynomial is all p - 1
    add = random_polys(P, n, groups, _NP[lb], 5)
    acc0, acc1 = np.zeros_like(add), add.copy()
    for j in range(terms):
        prod = o.pointwise(OP_MUL, np.ascontiguousarray(a[:, j]), np.ascontiguousarray(b[:, j]))
        acc0, acc1 = o.pointwise(OP_ADD, acc0, prod), o.pointwise(OP_ADD, acc1, prod)
    assert np.array_equal(dot_ref(a, b, P), acc0)
    assert np.array_equal(dot_ref(a, b, P, add), acc1)
    for i, p in enumerate(P):
        assert int(acc1[:, i].max()) < p


def test_header_declares_and_binding_binds_the_three_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    assert re.search(r"#define\s+NFLHIP_DOT_UNTILED\s+0x100\b", code) and re.search(r"#define\s+NFLHIP_DOT_MAX_POINTERS\s+16\b", code)
    assert re.search(r"typedef\s+struct\s+nflhip_dot_operand\s*\{[^}]*ptr;[^}]*group_stride;[^}]*term_stride;[^}]*\}\s*nflhip_dot_operand;", code)
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert _lib.DOT_UNTILED == 0x100 and _lib.DOT_MAX_POINTERS == 16
    assert [f[0] for f in _lib.DotOperand._fields_] == ["ptr", "group_stride", "term_stride"]
    for meth in ("dot", "matvec", "dot_strided", "dot_list", "h_dot"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    import ctypes as C
    from nfllib_amd import _lib
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    a, b = _lib.DotOperand(p + 64, 1, 1), _lib.DotOperand(p + 128, 1, 1)
    assert _lib.lib.nflhip_dot_dev(None, p, C.byref(a), C.byref(b), None, 1, 1, 0, None) == _lib.ERR_INVALID == 1   # NULL context: no device needed
    ptrs = (C.c_void_p * 1)(p + 64)
    assert _lib.lib.nflhip_dot_ptrs_dev(None, p, ptrs, ptrs, 1, None, None) == _lib.ERR_INVALID
    assert _lib.lib.nflhip_dot(None, p, p + 64, p + 128, 1, 1, 0) == _lib.ERR_INVALID


def build_cpp(out_dir, eager=False):
    """the C++ program of tests/cpp_dot, two translation units, with the g++ line of tests/cpp/Makefile"""
    exe = os.path.join(out_dir, "dot_test" + ("_eager" if eager else ""))
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-DNFL_HIP_NO_GMP"]
    if eager:
        cmd.append("-DNFL_HIP_EAGER")
    cmd += ["-o", exe, os.path.join(SRC, "dot_main.cpp"), os.path.join(SRC, "dot_tu2.cpp"),
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
