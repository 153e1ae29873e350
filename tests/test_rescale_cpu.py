"""CPU: the RNS rescale by the last modulus (include/nflhip.h "RNS rescale").  The two restatements of tests/rescale_util.py
agree with each other on random and edge inputs; the exact one agrees with a lift by the real reference's CRT (oracle/_ref,
where built; else the CPU oracle's); the NTT-form identity holds through the oracle's transforms; the C ABI, the Python
binding and the header surface carry the two new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from rescale_util import crt_combine, divide_round, edge_batch, random_batch, rescale_exact, rescale_ntt, rescale_rns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_rescale")
ENTRIES = ("nflhip_rescale_dev", "nflhip_rescale")
SHAPES = [(16, 128, 2), (32, 1024, 3), (64, 64, 4), (64, 1024, 94)]
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}


def moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


def test_definition_on_a_small_case():
    # moduli 5, 7, 11: q = 11, h = 5, Q' = 35.  X = 100: (100 + 5) // 11 = 9.  X = 384 = Q - 1: (389) // 11 = 35 = 0 mod 35.
    P = [5, 7, 11]
    for X, Y in ((100, 9), (384, 0), (0, 0), (5, 0), (6, 1), (16, 1), (17, 2)):
        a = np.array([[X % 5], [X % 7], [X % 11]], dtype=np.uint64)
        assert crt_combine(a, P).tolist() == [X]
        assert rescale_exact(a, P).tolist() == [[Y % 5], [Y % 7]], X
        assert rescale_rns(a, P).tolist() == [[Y % 5], [Y % 7]], X


@pytest.mark.parametrize("lb,n,nm", SHAPES)
def test_exact_and_row_formula_agree(lb, n, nm):
    P = moduli(lb, nm)
    a = np.concatenate([random_batch(P, n, 2, _NP[lb], 7), edge_batch(P, n, _NP[lb])])
    want = rescale_exact(a, P)
    assert np.array_equal(want, rescale_rns(a, P))
    assert not want[2].any() and not want[3].any()                      # every word 0, and every word p_i - 1: X = Q - 1 rounds up to Q' = 0
    for i, p in enumerate(P[:-1]):
        assert int(want[:, i].max()) < p          # canonical words


# (the last four are shapes the reference build instantiates, as is u64/1024/94: there the lift is the real reference's)
@pytest.mark.parametrize("lb,n,nm", SHAPES + [(32, 1024, 2), (64, 64, 3), (64, 4096, 4), (64, 16, 40)])
def test_exact_agrees_with_the_reference_lift(lb, n, nm, oracle_factory):
    """the integer behind the residues comes from Reference.crt_lift (the real reference's CRT) where oracle/_ref is built
    and instantiates the shape, else from Oracle.crt_lift; it feeds the same (X + h) // q % Q' formula"""
    P = moduli(lb, nm)
    o = oracle_factory(lb, n, nm)
    a = np.concatenate([o.fill_uniform(2, 5, 0), edge_batch(P, n, _NP[lb])])
    limbs = None
    if O.ref_available():
        try:
            limbs = O.Reference(lb, n, nm).crt_lift(a, o.crt_limbs)
        except KeyError:   # the reference build has no instance of this shape
            limbs = None
    if limbs is None:
        limbs = o.crt_lift(a)
    X = np.empty(limbs.shape[:2], dtype=object)
    for b in range(limbs.shape[0]):
        for j in range(limbs.shape[1]):
            X[b, j] = int.from_bytes(limbs[b, j].tobytes(), "little")
    assert np.array_equal(divide_round(X, P, _NP[lb]), rescale_exact(a, P))


@pytest.mark.parametrize("lb,n,nm", [(16, 128, 2), (32, 1024, 3), (64, 64, 4), (64, 4096, 2)])
def test_ntt_form_identity_through_the_oracle(lb, n, nm, oracle_factory):
    """with r = (intt_q(X_L) + h) mod q and d_i = (h - r) mod p_i:  (X_i + ntt_i(d_i)) q^-1 mod p_i == ntt_i(rescale_coeff(x)_i)"""
    P = moduli(lb, nm)
    q, h = P[-1], (P[-1] - 1) // 2
    big, small, last = oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - 1), O.Oracle(lb, n, 1, _Last(lb, nm))
    x = np.concatenate([big.fill_uniform(2, 9, 1), edge_batch(P, n, _NP[lb], combos=False)])
    X = big.ntt(x)
    want = rescale_ntt(X, P, big, small)
    assert np.array_equal(small.intt(want), rescale_rns(x, P))
    r = (last.intt(np.ascontiguousarray(X[:, nm - 1:, :]))[:, 0, :].astype(object) + h) % q
    d = np.empty_like(want)
    for i, p in enumerate(P[:-1]):
        d[:, i, :] = ((h - r) % p).astype(_NP[lb])
    D = small.ntt(d)
    for i, p in enumerate(P[:-1]):
        y = ((X[:, i, :].astype(object) + D[:, i, :].astype(object)) * pow(q % p, -1, p)) % p
        assert np.array_equal(y.astype(_NP[lb]), want[:, i, :]), i


class _Last:
    """the parameter tables of a limb width, cut down to the nm-th modulus alone"""

    def __init__(self, lb, nm):
        from nfllib_amd.params import params
        pr = params(lb)
        for k, v in vars(pr).items():
            setattr(self, k, v)
        self.P, self.Pn, self.primitive_roots, self.invkmax = (np.ascontiguousarray(t[nm - 1:nm])
                                                               for t in (pr.P, pr.Pn, pr.primitive_roots, pr.invkmax))
        self.max_moduli = 1


def test_header_declares_and_binding_binds_the_two_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    for meth in ("rescale", "h_rescale"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    assert _lib.lib.nflhip_rescale_dev(None, p, p + 64, 1, 0, None) == _lib.ERR_INVALID == 1   # NULL context: no device needed
    assert _lib.lib.nflhip_rescale(None, p, p + 64, 1, 0) == _lib.ERR_INVALID


def build_cpp(out_dir, eager=False):
    """the C++ program of tests/cpp_rescale, two translation units, with the g++ line of tests/cpp/Makefile"""
    exe = os.path.join(out_dir, "rescale_test" + ("_eager" if eager else ""))
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-DNFL_HIP_NO_GMP"]
    if eager:
        cmd.append("-DNFL_HIP_EAGER")
    cmd += ["-o", exe, os.path.join(SRC, "rescale_main.cpp"), os.path.join(SRC, "rescale_tu2.cpp"),
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
