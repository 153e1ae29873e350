"""CPU: slot linear transforms and the weighted sum of automorphisms (include/nflhip.h "slot linear transforms", "weighted sums of
automorphisms").
  * the C ABI, the Python binding and the Engine carry the new names; a NULL context is refused without a device;
  * a REAL linear transform on the restatement of tests/lintrans_util.py alone: with Galois keys of the header's convention and
    ternary diagonals, out0 + out1 s is sum_m pt_m sigma_{k_m}(c0 + c1 s) up to the noise the mathematics allows, and no more than
    the weighted sum of hoisted rotations leaves;
  * the compiler's resource report for every instance of k_permute_mac_ntt."""
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from automorph_util import sigma_ntt
from keyswitch_util import digits
from lintrans_util import lintrans_rns, mac_rns
from rotate_util import rotate_rns
from test_rotate_cpu import _resource_report, _rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_automorphism_mac_dev", "nflhip_automorphism_mac", "nflhip_lintrans_ntt_dev", "nflhip_lintrans_ntt")
FLAGS = {"CENTERED": 0x100, "FLOOR": 0x200, "SEQUENCE": 0x1000, "HOISTED": 0x2000}


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_LINTRANS_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in FLAGS}
    assert flags == FLAGS
    assert re.search(r"#define\s+NFLHIP_LINTRANS_MAX_TERMS\s+16\b", code) and re.search(r"#define\s+NFLHIP_MAC_MAX_TERMS\s+16\b", code)
    # the definition, and that it is NOT the weighted sum of rotations
    for phrase in ("A_c     = sum_{keyed m} w_m (.) sigma^NTT_{k_m}(S_{m,c})", "Y_c     = nflhip_moddown_ntt_dev(A_c, k_special)",
                   "out1    = Y_1 + sum_{unkeyed m} w_m (.) c1", "THESE ARE NOT THE WORDS OF sum_m w_m (.) nflhip_rotate_hoisted_ntt_dev",
                   "out[g][j][i] = addend[g][j][i] + sum_{t < terms} w_t[j][i] * in_t[g][j][src_{k_t}(i)]"):
        assert phrase in txt, phrase
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert {k: getattr(_lib, "LINTRANS_" + k) for k in FLAGS} == FLAGS
    assert _lib.LINTRANS_MAX_TERMS == 16 and _lib.MAC_MAX_TERMS == 16
    for meth in ("automorphism_mac", "h_automorphism_mac", "linear_transform_ntt", "h_linear_transform_ntt"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    import ctypes as C
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    keys, ws, ks = (C.c_void_p * 1)(p + 192), (C.c_void_p * 1)(p + 256), (C.c_uint64 * 1)(5)
    for flags in (0,) + tuple(FLAGS.values()):
        assert L.nflhip_lintrans_ntt_dev(None, p, p + 64, None, p + 128, keys, ws, ks, 1, 1, 1, 1, flags, None) == _lib.ERR_INVALID == 1   # no device needed
        assert L.nflhip_lintrans_ntt(None, p, p + 64, None, p + 128, keys, ws, ks, 1, 1, 1, 1, flags) == _lib.ERR_INVALID
    for flags in (0, _lib.MAC_DOUBLE_BUFFER):
        assert L.nflhip_automorphism_mac_dev(None, p, None, keys, ws, ks, 1, 1, 1, flags, None) == _lib.ERR_INVALID
        assert L.nflhip_automorphism_mac(None, p, None, keys, ws, ks, 1, 1, 1, flags) == _lib.ERR_INVALID


def test_the_restated_primitive_is_the_automorphism_followed_by_products():
    """mac_rns against the formula written out slot by slot with automorph_util.ntt_source"""
    from automorph_util import ntt_source
    from nfllib_amd.params import params
    n, rows = 16, 2
    P = [int(v) for v in params(64).P[:3]]
    ins = [B.random_batch(P[:rows], n, 2, np.uint64, 1 + t) for t in range(3)]
    ws = [B.random_batch(P, n, 1, np.uint64, 10 + t)[0] for t in range(3)]
    add = B.random_batch(P[:rows], n, 2, np.uint64, 20)
    ks = [1, 2 * n - 1, 5]
    got = mac_rns(ins, ws, ks, P[:rows], addend=add)
    for g in range(2):
        for j in range(rows):
            for i in range(n):
                v = int(add[g, j, i]) + sum(int(ws[t][j, i]) * int(ins[t][g, j, ntt_source(n, ks[t])[i]]) for t in range(3))
                assert int(got[g, j, i]) == v % P[j]


@pytest.mark.parametrize("K,alpha", [(1, 1), (2, 2), (2, 1)])
@pytest.mark.parametrize("centered", [False, True])
def test_the_definition_is_a_linear_transform(K, alpha, centered, oracle_factory):
    """u64/64/5, ternary s, key noise |e| <= 8, four ternary diagonals pt_m (T = 1), k = 5, 2n - 1, 1 (no key: the unrotated
    diagonal), 25.  Every keyed term's key switch leaves, before the division by P, a noise that the product with pt_m multiplies
    by at most n T; the one rounding of the mod-down is smaller than any of the `keyed` roundings the bound B of one key switch
    (tests/test_rotate_cpu.py) pays for.  So
        0 < | out0 + out1 s - sum_m pt_m sigma_{k_m}(c0 + c1 s) |_inf  <=  keyed n T B,   B = n dnum alpha 8 2^alpha + n + 1,
    and the residue is no larger than that of sum_m pt_m (.) (hoisted rotation m) on the same inputs, plus n + 1 (one rounding
    against a ternary s).  Measured, fast / centred (the weighted sum of rotations in brackets), against the bound:
        K 1 alpha 1:  1763 / 1016  (1781 / 1016)   798912
        K 2 alpha 2:   834 /  329  ( 866 /  337)  1585344
        K 2 alpha 1:     5 /    5  (  56 /   58)   602304"""
    from nfllib_amd.params import params
    lb, n, nm, T = 64, 64, 5, 1
    L = nm - K
    P = [int(v) for v in params(lb).P[:nm]]
    orc, ok = oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    rnd = np.random.RandomState(2000 * K + 20 * alpha + centered)
    Q, Ps = B.prod(P[:L]), B.prod(P[L:])
    S = digits(nm, K, alpha)
    dnum = len(S)
    ks = [5, 2 * n - 1, 1, 25]
    s = rnd.randint(-1, 2, size=n).astype(object)
    S_ntt = orc.ntt(_rows(s, P, np.uint64)[None])[0]
    keys = []
    for m, k in enumerate(ks):
        if k == 1:
            keys.append(None)
            continue
        Sinv_ntt = sigma_ntt(S_ntt, pow(k, -1, 2 * n)).astype(object)          # sigma_(k^-1)(s), NTT form
        key = np.empty((dnum, 2, nm, n), dtype=np.uint64)
        for d, (s0, kd) in enumerate(S):
            Qd = B.prod(P[s0:s0 + kd])
            g = (Q // Qd) * pow((Q // Qd) % Qd, -1, Qd)
            a_ntt = B.random_batch(P, n, 1, np.uint64, 7 + 10 * m + d)[0]        # uniform mod Q P, taken in NTT form
            e_ntt = orc.ntt(_rows(rnd.randint(-8, 9, size=n).astype(object), P, np.uint64)[None])[0]
            for j, p in enumerate(P):
                key[d, 0, j] = ((e_ntt[j].astype(object) - a_ntt[j].astype(object) * Sinv_ntt[j] + (Ps * g) % p * S_ntt[j].astype(object)) % p).astype(np.uint64)
            key[d, 1] = a_ntt
        keys.append(key)
    keyed = sum(k is not None for k in keys)
    weights = [orc.ntt(_rows(rnd.randint(-T, T + 1, size=n).astype(object), P, np.uint64)[None])[0] for _ in ks]
    c0, c1 = (ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed)) for seed in (5, 6))   # a ciphertext, uniform mod Q
    So = S_ntt.astype(object)

    def residue(out0, out1):
        msg = np.empty_like(c0)                                                   # c0 + c1 s
        for j in range(L):
            msg[:, j] = ((c0[:, j].astype(object) + c1[:, j].astype(object) * So[j]) % P[j]).astype(np.uint64)
        want = mac_rns([msg] * len(ks), weights, ks, P[:L])
        r = np.empty_like(c0)
        for j in range(L):
            r[:, j] = ((out0[:, j].astype(object) + out1[:, j].astype(object) * So[j] - want[:, j].astype(object)) % P[j]).astype(np.uint64)
        err = B.centre(B.crt_rows(ok.intt(r), P, (0, L)), Q)
        return max(abs(int(v)) for v in err.ravel())

    norm = residue(*lintrans_rns(c0, c1, keys, weights, ks, P, K, alpha, centered, False, orc, ok))
    # the previous way: the hoisted rotations of the keyed terms, then the weighted sums of the rotated (and the unrotated) ciphertexts
    rot = iter(rotate_rns(c0, c1, [k for k in keys if k is not None], [k for k, key in zip(ks, keys) if key is not None], P, K, alpha, centered,
                          False, orc, ok))
    cts = [next(rot) if key is not None else (c0, c1) for key in keys]
    ones = [1] * len(ks)
    prev = residue(mac_rns([ct[0] for ct in cts], weights, ones, P[:L]), mac_rns([ct[1] for ct in cts], weights, ones, P[:L]))
    bound = keyed * n * T * (n * dnum * alpha * 8 * 2**alpha + n + 1)
    print("K %d alpha %d centred %d: |out0 + out1 s - sum pt sigma(c0 + c1 s)|_inf = %d (weighted sum of rotations: %d), bound %d"
          % (K, alpha, centered, norm, prev, bound))
    assert keyed == 3
    assert 0 < norm <= bound
    assert norm <= prev + n + 1


def test_compiled_kernel_uses_no_scratch_and_spills_no_register(tmp_path):
    """the compiler's own resource report for every instance of k_permute_mac_ntt (hipcc cross-compiles for gfx950 without a GPU):
    three limb widths x (16-byte groups, words) x (one staging buffer, two); no scratch memory, no spilled register; the LDS is
    sized at launch"""
    kernels = _resource_report(tmp_path, "kernels_lintrans")
    mine = {k: v for k, v in kernels.items() if "k_permute_mac_ntt" in k}
    assert len(mine) == 12, sorted(kernels)
    for name, v in sorted(mine.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
        assert int(v["LDS Size [bytes/block]"]) == 0, name
