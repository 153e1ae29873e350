"""CPU: hoisted rotations and slot linear transforms below the top level with the ONE top-level Galois key per rotation and the ONE
top-level diagonal per term (include/nflhip.h "rotations and linear transforms at a level").
  * the C ABI, the Python binding and the Engine carry the new names; without a device every entry refuses a NULL context, whatever
    the level -- which is all a machine without a GPU can ask of them: the level checks themselves need a context and are exercised
    in tests/test_gpu_level_rotate.py;
  * the compiler's resource report: no scratch and no spilled register, vector or scalar, in any kernel instance of
    kernels_level_rotate.hip, and the instances of the two kernels on the dense layout at the register counts DESIGN.md records;
  * THE REFERENCE ONLY -- these two pass without the feature, on the restatement of tests/level_rotate_util.py alone, and say that
    the definition of a level call is the right one: a Galois key generated ONCE at the top level rotates a ciphertext at every
    level with the noise the mathematics allows, and one relinearisation key, one set of Galois keys and one set of top-level
    diagonals serve a chain product -> linear transform -> product down the modulus chain."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from automorph_util import sigma_ntt
from level_rotate_util import lintrans_level_rns, rotate_level_rns
from level_util import RowsOracle, level_digits, mulrelin_level_rns
from lintrans_util import mac_rns
from mulrelin_util import relin_key
from test_level_cpu import _demangled, _resource_report, _secret, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_rotate_hoisted_level_ntt_dev", "nflhip_rotate_hoisted_level_ntt", "nflhip_lintrans_level_ntt_dev", "nflhip_lintrans_level_ntt")


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code                                 # entries are added, the number stays
    assert "rotations and linear transforms at a level" in txt                    # the header comment states the definition
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    import inspect
    for meth in ("rotate_hoisted_ntt", "h_rotate_hoisted_ntt", "linear_transform_ntt", "h_linear_transform_ntt"):
        assert inspect.signature(getattr(Engine, meth)).parameters["level"].default is None, meth


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(1024, dtype=np.uint64)
    p = buf.ctypes.data
    o0, o1, keys, ws, ks = (C.c_void_p * 1)(p), (C.c_void_p * 1)(p + 64), (C.c_void_p * 1)(p + 192), (C.c_void_p * 1)(p + 4096), (C.c_uint64 * 1)(5)
    # a NULL context is NFLHIP_ERR_INVALID before any device use, with a level of 0, past any L and 1 alike: the refusal is the NULL
    # context's; the level checks themselves need a context (tests/test_gpu_level_rotate.py)
    for level in (0, 2**64 - 1, 1):
        for flags in (0, _lib.ROTATE_SEQUENCE, _lib.ROTATE_HOISTED | _lib.ROTATE_CENTERED):
            assert L.nflhip_rotate_hoisted_level_ntt_dev(None, o0, o1, None, p + 128, keys, ks, 1, 1, 1, 1, level, flags, None) == _lib.ERR_INVALID == 1
            assert L.nflhip_rotate_hoisted_level_ntt(None, o0, o1, None, p + 128, keys, ks, 1, 1, 1, 1, level, flags) == _lib.ERR_INVALID
            assert L.nflhip_lintrans_level_ntt_dev(None, p, p + 64, None, p + 128, keys, ws, ks, 1, 1, 1, 1, level, flags, None) == _lib.ERR_INVALID
            assert L.nflhip_lintrans_level_ntt(None, p, p + 64, None, p + 128, keys, ws, ks, 1, 1, 1, 1, level, flags) == _lib.ERR_INVALID


def test_new_kernel_instances_use_no_scratch_and_spill_no_register(tmp_path):
    """every kernel of kernels_level_rotate.hip (hipcc cross-compiles for gfx950 without a GPU): k_dot_multi on the level keys, three
    limb widths x (16-byte groups, words) x (tile 2, 1) x (register, streaming); k_permute_mac_ntt on the level diagonals, three limb
    widths x (16-byte groups, words), one staging buffer.  The u16 instances have no context that reaches them (two moduli, no level
    below the top): this report is their whole cover."""
    kernels = _resource_report(tmp_path, "kernels_level_rotate")
    names = _demangled(kernels)
    dot = {k: v for k, v in kernels.items() if "k_dot_multi<" in names[k] and "DotMultiArgsLevel" in names[k]}
    mac = {k: v for k, v in kernels.items() if "k_permute_mac_ntt<" in names[k] and "MacTermsLevel" in names[k]}
    assert len(dot) == 24 and len(mac) == 6 and len(kernels) == 30, sorted(names.values())
    assert all(", false, nflhip::MacTermsLevel" in names[k] for k in mac)          # one staging buffer only
    for name, v in sorted(kernels.items()):
        print(names[name].split("(")[0], "VGPRs", v["VGPRs"], "SGPRs", v["TotalSGPRs"], "LDS", v["LDS Size [bytes/block]"], "Occupancy",
              v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
    for name, v in dot.items():
        assert int(v["LDS Size [bytes/block]"]) == 0, name


def test_untouched_instances_keep_their_registers(tmp_path):
    """the instances on the dense layout are the same templates with another parameter and must compile to what they compiled to
    before: the u64 vector-register counts DESIGN.md 5.17 and 5.18 record, in the order (16-byte, words) x (tile 2, 1) x (register,
    streaming) for k_dot_multi and (16-byte, words) x (one, two buffers) for k_permute_mac_ntt; the u16 16-byte one-buffer instance
    of k_permute_mac_ntt stays at 234; nothing spilled"""
    dm = _resource_report(tmp_path, "kernels_dot_multi")
    names = _demangled(dm)

    def vgprs(report, names, prefix):
        got = [int(v["VGPRs"]) for k, v in report.items() if names[k].startswith("void nflhip::" + prefix)]
        assert len(got) == 1, (prefix, got)
        return got[0]
    got = [vgprs(dm, names, "k_dot_multi<unsigned long, %d, %d, %d" % (V, G, R)) for V in (2, 1) for G in (2, 1) for R in (1, 0)]
    assert got == [114, 72, 64, 48, 64, 52, 38, 36], got
    assert sum("k_dot_multi<" in n for n in names.values()) == 24
    lt = _resource_report(tmp_path, "kernels_lintrans")
    names = _demangled(lt)
    got = [vgprs(lt, names, "k_permute_mac_ntt<unsigned long, %s, %s" % (vec, db)) for vec in ("true", "false") for db in ("false", "true")]
    assert got == [130, 170, 160, 176], got
    assert vgprs(lt, names, "k_permute_mac_ntt<unsigned short, true, false") == 234
    assert sum("k_permute_mac_ntt<" in n for n in names.values()) == 12
    for report in (dm, lt):
        assert all(int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0 and int(v["ScratchSize [bytes/lane]"]) == 0 for v in report.values())


# ---- the reference: these validate tests/level_rotate_util.py and would pass without the feature ----
def _galois_key(P, K, alpha, n, S, k, orc, rnd, seed):
    """the header's convention: from s to sigma_(k^-1)(s), generated over the FULL context --
    key[d][0] = -a_d sigma_(k^-1)(s) + e_d + P g_d s, key[d][1] = a_d"""
    Sinv = sigma_ntt(S.astype(np.uint64), pow(k, -1, 2 * n)).astype(object)
    return relin_key(P, K, alpha, n, Sinv, S, orc, rnd, seed=seed)


def _phase(c0, c1, S, P, level, orc):
    """c0 + c1 s over Q_l as NTT-form rows"""
    r = np.empty_like(c0)
    for j in range(level):
        r[:, j] = ((c0[:, j].astype(object) + c1[:, j].astype(object) * S[j]) % P[j]).astype(np.uint64)
    return r


def _norm(rows, P, level, orc):
    """the infinity norm of the centred CRT lift of NTT-form rows over Q_l"""
    kept = RowsOracle(orc, len(P), range(level))
    return max(abs(int(v)) for v in B.centre(B.crt_rows(kept.intt(rows), P, (0, level)), B.prod(P[:level])).ravel())


def _sub(x, y, P, level):
    r = np.empty_like(x)
    for j in range(level):
        r[:, j] = ((x[:, j].astype(object) - y[:, j].astype(object)) % P[j]).astype(np.uint64)
    return r


@pytest.mark.parametrize("K,alpha", [(2, 2), (1, 1)])
@pytest.mark.parametrize("centered", [False, True])
def test_one_top_level_galois_key_rotates_at_every_level(K, alpha, centered, oracle_factory):
    """VALIDATES THE REFERENCE ONLY.  u64/64/6, the Galois keys of tests/test_rotate_cpu.py for k = 5 and 2n - 1 generated once over
    the full context.  On a live row j < l the gadget factor g_d is 1 when j is in digit d and 0 otherwise, whatever the level, so the
    rows [0, l) and [L, nm) of such a key are a Galois key of C_l with the digits cut at l.  At every level
        0 < | out0 + out1 s - sigma_k(c0 + c1 s) |_inf <= n dnum_l alpha 8 2^alpha + n + 1
    over Q_l: the bound of DESIGN.md 5.17 with the level's digit count.  (alpha <= K: hybrid switching needs P >= Q_d.)"""
    lb, n, nm = 64, 64, 6
    L = nm - K
    P, orc = _setup(lb, n, nm, oracle_factory)
    rnd = np.random.RandomState(300 * K + centered)
    S = _secret(P, n, orc, rnd)
    ks = [5, 2 * n - 1]
    keys = [_galois_key(P, K, alpha, n, S, k, orc, rnd, 7 + 10 * m) for m, k in enumerate(ks)]
    for level in range(1, L + 1):
        kept = RowsOracle(orc, nm, range(level))
        c0, c1 = (kept.ntt(B.random_batch(P[:level], n, 2, np.uint64, seed + level)) for seed in (5, 60))
        outs = rotate_level_rns(c0, c1, keys, ks, P, K, alpha, level, centered, False, orc)
        msg = _phase(c0, c1, S, P, level, orc)
        for k, (out0, out1) in zip(ks, outs):
            assert out0.shape == out1.shape == c0.shape
            norm = _norm(_sub(_phase(out0, out1, S, P, level, orc), sigma_ntt(msg, k), P, level), P, level, orc)
            bound = n * level_digits(level, alpha) * alpha * 8 * 2**alpha + n + 1
            print("K = alpha = %d, centred %d, level %d, k %d: |out0 + out1 s - sigma_k(c0 + c1 s)|_inf = %d, bound %d" % (K, centered, level, k, norm, bound))
            assert 0 < norm <= bound


@pytest.mark.parametrize("K,alpha", [(2, 2), (1, 1)])
def test_one_set_of_keys_and_diagonals_serves_a_chain(K, alpha, oracle_factory):
    """VALIDATES THE REFERENCE ONLY.  u64/64/6, s ternary: ONE relinearisation key, ONE Galois key per rotation (k = 5, 2n - 1) and ONE
    set of three ternary diagonals pt_m (T = 1; the third term is the unrotated one, no key), each diagonal encoded once as its
    residues under all nm moduli.  Two small plaintexts are multiplied with the rescale at the top level l = L; the linear transform
    runs at l - 1; its result is squared with the rescale.  With m_x the phase c0 + c1 s of a step's input over its Q_l:
        product at l, q = p_(l-1):   | q (out0 + out1 s) - m_a m_b |_inf <= n dnum_l alpha 8 2^alpha + q (n + 1)      
        transform at l:              | out0 + out1 s - sum_m pt_m sigma_(k_m)(m_x) |_inf <= keyed n T (n dnum_l alpha 8 2^alpha + n + 1)
                                                                                                                        
    each with the level's digit count, and each positive (there is noise)."""
    lb, n, nm, T = 64, 64, 6, 1
    L = nm - K
    P, orc = _setup(lb, n, nm, oracle_factory)
    rnd = np.random.RandomState(700 + K)
    S = _secret(P, n, orc, rnd)
    S2 = np.empty_like(S)
    for j, p in enumerate(P):
        S2[j] = S[j] * S[j] % p
    rkey = relin_key(P, K, alpha, n, S, S2, orc, rnd)
    ks = [5, 2 * n - 1, 1]
    gkeys = [_galois_key(P, K, alpha, n, S, k, orc, rnd, 40 + 10 * m) if k != 1 else None for m, k in enumerate(ks)]
    weights = [orc.ntt(B.rows_of(rnd.randint(-T, T + 1, size=n).astype(object), P, range(nm), np.uint64)[None])[0] for _ in ks]
    top = RowsOracle(orc, nm, range(L))

    def encrypt(seed):
        m = top.ntt(B.rows_of(rnd.randint(-4, 5, size=(2, n)).astype(object), P, range(L), np.uint64))
        c1 = top.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed))
        c0 = np.empty_like(c1)
        for j in range(L):
            c0[:, j] = ((m[:, j].astype(object) - c1[:, j].astype(object) * S[j]) % P[j]).astype(np.uint64)
        return c0, c1

    def product_step(a, b, level):
        q = P[level - 1]
        ma, mb = _phase(a[0], a[1], S, P, level, orc), _phase(b[0], b[1], S, P, level, orc)
        prod = np.empty_like(ma)
        for j in range(level):
            prod[:, j] = (ma[:, j].astype(object) * mb[:, j].astype(object) % P[j]).astype(np.uint64)
        out = mulrelin_level_rns(a[0], a[1], b[0], b[1], rkey, P, K, alpha, level, False, False, True, orc)
        assert out[0].shape == out[1].shape == (2, level - 1, n)
        Q = B.prod(P[:level])
        kept, lower = RowsOracle(orc, nm, range(level)), RowsOracle(orc, nm, range(level - 1))
        M = B.crt_rows(kept.intt(prod), P, (0, level))
        Y = B.crt_rows(lower.intt(_phase(out[0], out[1], S, P, level - 1, orc)), P, (0, level - 1))
        norm = max(abs(int(v)) for v in B.centre((q * Y - M) % Q, Q).ravel())
        bound = n * level_digits(level, alpha) * alpha * 8 * 2**alpha + q * (n + 1)
        print("K = alpha = %d, product %d -> %d: |q (out0 + out1 s) - m_a m_b|_inf / q = %.3f, bound %.3f" % (K, level, level - 1, norm / q, bound / q))
        assert 0 < norm <= bound
        return out

    a, b = encrypt(11), encrypt(12)
    c = product_step(a, b, L)
    level = L - 1
    d = lintrans_level_rns(c[0], c[1], gkeys, weights, ks, P, K, alpha, level, False, False, orc)
    assert d[0].shape == d[1].shape == (2, level, n)
    msg = _phase(c[0], c[1], S, P, level, orc)
    want = mac_rns([msg] * len(ks), weights, ks, P[:level])
    norm = _norm(_sub(_phase(d[0], d[1], S, P, level, orc), want, P, level), P, level, orc)
    bound = 2 * n * T * (n * level_digits(level, alpha) * alpha * 8 * 2**alpha + n + 1)
    print("K = alpha = %d, transform at %d: |out0 + out1 s - sum pt sigma(m)|_inf = %d, bound %d" % (K, level, norm, bound))
    assert 0 < norm <= bound
    if level >= 2:
        product_step(d, d, level)
