"""CPU: ciphertext multiplication with relinearisation (include/nflhip.h "ciphertext multiplication").
  * the C ABI, the Python binding and the Engine carry the new names, the flag values are pinned; a NULL context is refused without a
    device;
  * identity 1 of DESIGN.md 5.19 on the restatement of tests/mulrelin_util.py: with pi (.) d_c as the addend of the key-switch sums,
    ONE mod-down gives the words of tensor + key switch + addition, in both mod-up modes and both roundings;
  * it IS a multiplication: with a real relinearisation key the result decrypts to the product with the noise the mathematics allows,
    without and with the rescale in the same rounding;
  * the compiler's resource report for every instance of the new kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from mulrelin_util import mulrelin_rns, relin_key, tensor_rns, two_step
from rescale_util import rescale_ntt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_tensor_ntt_dev", "nflhip_tensor_ntt", "nflhip_mulrelin_ntt_dev", "nflhip_mulrelin_ntt")
FLAGS = {"CENTERED": 0x100, "FLOOR": 0x200, "RESCALE": 0x400, "FUSED": 0x800, "SEQUENCE": 0x1000, "MERGED": 0x2000}


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_MULRELIN_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in FLAGS}
    assert flags == FLAGS
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert {k: getattr(_lib, "MULRELIN_" + k) for k in FLAGS} == FLAGS
    for meth in ("tensor_ntt", "h_tensor_ntt", "mul_relin_ntt", "h_mul_relin_ntt"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(1024, dtype=np.uint64)
    p = [buf.ctypes.data + 1024 * k for k in range(8)]
    for flags in (0,) + tuple(FLAGS.values()):
        assert L.nflhip_mulrelin_ntt_dev(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 1, flags, None) == _lib.ERR_INVALID == 1
        assert L.nflhip_mulrelin_ntt(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 1, flags) == _lib.ERR_INVALID
    assert L.nflhip_tensor_ntt_dev(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 0, None) == _lib.ERR_INVALID   # no device needed
    assert L.nflhip_tensor_ntt(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 0) == _lib.ERR_INVALID


def _setup(lb, n, nm, K, oracle_factory):
    from nfllib_amd.params import params
    P = [int(v) for v in params(lb).P[:nm]]
    return P, oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K)


@pytest.mark.parametrize("K,alpha", [(2, 2), (2, 1), (1, 3)])
def test_one_mod_down_with_the_addend_gives_the_words_of_the_two_step_way(K, alpha, oracle_factory):
    """u64/64/5.  mod_down(acc + E(pi d)) = mod_down(acc) + d word for word: the special rows are untouched by the addend, and on a kept
    row (pi_j d) P^-1 = d mod p_j.  Uniform operands and a uniform key (the identity does not need a real one); the square as well."""
    lb, n, nm = 64, 64, 5
    L = nm - K
    P, orc, ok = _setup(lb, n, nm, K, oracle_factory)
    a0, a1, b0, b1 = (B.random_batch(P[:L], n, 2, np.uint64, 40 + t) for t in range(4))
    dnum = len(digits(nm, K, alpha))
    key = B.random_batch(P, n, 2 * dnum, np.uint64, 50).reshape(dnum, 2, nm, n)
    for centered in (False, True):
        for floor in (False, True):
            for bb in ((b0, b1), (None, None)):
                got = mulrelin_rns(a0, a1, bb[0], bb[1], key, P, K, alpha, centered, floor, False, orc, ok)
                want = two_step(a0, a1, bb[0], bb[1], key, P, K, alpha, centered, floor, orc, ok)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (centered, floor, bb[0] is None)


def _ciphertexts(P, K, alpha, n, orc, ok, seed):
    """a ternary secret, the key from s^2 to s, two uniform ciphertexts and the NTT rows of (a0 + a1 s)(b0 + b1 s) on the kept moduli"""
    nm = len(P)
    L = nm - K
    rnd = np.random.RandomState(seed)
    s = rnd.randint(-1, 2, size=n).astype(object)
    S = orc.ntt(B.rows_of(s, P, range(nm), np.uint64)[None])[0].astype(object)
    S2 = np.empty_like(S)
    for j, p in enumerate(P):
        S2[j] = S[j] * S[j] % p                                                   # s' = s^2, negacyclic, in NTT form
    key = relin_key(P, K, alpha, n, S, S2, orc, rnd)
    a0, a1, b0, b1 = (ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed + 1 + t)) for t in range(4))
    msg = np.empty_like(a0)
    for j in range(L):
        x, y = (u[:, j].astype(object) + v[:, j].astype(object) * S[j] for u, v in ((a0, a1), (b0, b1)))
        msg[:, j] = (x * y % P[j]).astype(np.uint64)
    return S, key, (a0, a1, b0, b1), msg


def _phase(o0, o1, S, P):
    r = np.empty_like(o0)
    for j in range(o0.shape[1]):
        r[:, j] = ((o0[:, j].astype(object) + o1[:, j].astype(object) * S[j]) % P[j]).astype(np.uint64)
    return r


@pytest.mark.parametrize("K,alpha", [(1, 1), (2, 2)])
@pytest.mark.parametrize("centered", [False, True])
def test_it_is_a_multiplication(K, alpha, centered, oracle_factory):
    """u64/64/5, keys as in tests/test_keyswitch_cpu.py with s' = s^2.  out0 + out1 s - (a0 + a1 s)(b0 + b1 s) is the key switch's own
    error on d2 (d0 + d1 s + d2 s^2 is the product exactly): at most n dnum alpha 8 2^alpha + n + 1, the bound of DESIGN.md 5.16."""
    lb, n, nm = 64, 64, 5
    L = nm - K
    P, orc, ok = _setup(lb, n, nm, K, oracle_factory)
    S, key, (a0, a1, b0, b1), msg = _ciphertexts(P, K, alpha, n, orc, ok, 300 * K + centered)
    Q = B.prod(P[:L])
    o0, o1 = mulrelin_rns(a0, a1, b0, b1, key, P, K, alpha, centered, False, False, orc, ok)
    ph = _phase(o0, o1, S, P)
    r = np.empty_like(ph)
    for j in range(L):
        r[:, j] = ((ph[:, j].astype(object) - msg[:, j].astype(object)) % P[j]).astype(np.uint64)
    norm = max(abs(int(v)) for v in B.centre(B.crt_rows(ok.intt(r), P, (0, L)), Q).ravel())
    bound = n * len(key) * alpha * 8 * 2**alpha + n + 1
    print("K = alpha = %d, centred %d: |out0 + out1 s - (a0 + a1 s)(b0 + b1 s)|_inf = %d, bound %d" % (K, centered, norm, bound))
    assert 0 < norm <= bound


@pytest.mark.parametrize("K,alpha", [(1, 1), (2, 2)])
def test_with_the_rescale_in_the_same_rounding(K, alpha, oracle_factory):
    """u64/64/5, rounding mode.  A_c = P (d_c + ks_c) + (the key's errors); the mod-down by P q returns y_c within 1 of A_c / (P q)
    coefficient by coefficient, so q (y_0 + y_1 s) - (a0 + a1 s)(b0 + b1 s) is the key-switch error (before its
    division by P: n dnum alpha 8 2^alpha covers it) plus q times the two rounding errors, the second multiplied by the ternary s:
        | . |_inf <= n dnum alpha 8 2^alpha + q (n + 1).
    The two-step way -- the product without the rescale, then the rescale of both components -- is printed next to it."""
    lb, n, nm = 64, 64, 5
    L = nm - K
    P, orc, ok = _setup(lb, n, nm, K, oracle_factory)
    okm = oracle_factory(lb, n, L - 1)
    S, key, (a0, a1, b0, b1), msg = _ciphertexts(P, K, alpha, n, orc, ok, 700 * K)
    Q, q = B.prod(P[:L]), P[L - 1]
    M = B.crt_rows(ok.intt(msg), P, (0, L))

    def residue(o0, o1):
        assert o0.shape == o1.shape == (2, L - 1, n)
        Y = B.crt_rows(okm.intt(_phase(o0, o1, S, P)), P, (0, L - 1))
        return max(abs(int(v)) for v in B.centre((q * Y - M) % Q, Q).ravel())

    one = residue(*mulrelin_rns(a0, a1, b0, b1, key, P, K, alpha, False, False, True, orc, ok, okm))
    t0, t1 = mulrelin_rns(a0, a1, b0, b1, key, P, K, alpha, False, False, False, orc, ok)
    two = residue(rescale_ntt(t0, P[:L], ok, okm), rescale_ntt(t1, P[:L], ok, okm))
    bound = n * len(key) * alpha * 8 * 2**alpha + q * (n + 1)
    print("K = alpha = %d: |q (out0 + out1 s) - product|_inf / q = %.3f in one rounding, %.3f in two steps, bound %.3f"
          % (K, one / q, two / q, bound / q))
    assert 0 < one <= bound
    # the two-step way: its first rounding errs by at most 1 / q of the quotient's unit and its second by a half, so each coefficient is
    # within 1 of the quotient as well and the same bound holds
    assert 0 < two <= bound


def test_compiled_kernel_uses_no_scratch_and_spills_no_register(tmp_path):
    """the compiler's own resource report for every instance of k_tensor_ntt (hipcc cross-compiles for gfx950 without a GPU): three limb
    widths x (16-byte groups, words) x (general, square), no LDS; and of k_tensor_modup_dot_fused: three limb widths, up to 1024
    threads per workgroup, which leaves it 128 vector registers.  No scratch memory and no spilled register, vector or scalar, in any
    of the fifteen (the one-launch kernel reads its pointers from the kernel-argument segment where it uses them, which is what keeps
    its scalar registers from spilling into vector lanes)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_mulrelin.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_mulrelin.o")], capture_output=True, text=True, timeout=1200)
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
    mine = {k: v for k, v in kernels.items() if "k_tensor_ntt" in k}
    fused = {k: v for k, v in kernels.items() if "k_tensor_modup_dot_fused" in k}
    assert len(mine) == 12 and len(fused) == 3, sorted(kernels)
    for name, v in sorted(mine.items()) + sorted(fused.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
    for name, v in mine.items():
        assert int(v["LDS Size [bytes/block]"]) == 0, name
    for name, v in fused.items():                                                 # up to 1024 threads per workgroup: 128 vector registers
        assert int(v["VGPRs"]) <= 128, name
