"""CPU: key switching and multiplication below the top level with the ONE top-level key (include/nflhip.h "leveled key switching").
  * the C ABI, the Python binding and the Engine carry the new names; without a device every entry refuses a NULL context, whatever
    the level -- which is all a machine without a GPU can ask of them: the level-0, level-above-L and RESCALE-at-level-1 checks and
    the digit counts of nflhip_keyswitch_level_digits need a context and are exercised in tests/test_gpu_level.py;
  * the compiler's resource report: no scratch and no spilled register, vector or scalar, in any kernel instance of
    kernels_level.hip, and the instances this change must not disturb at the register counts DESIGN.md records;
  * THE REFERENCE ONLY -- these two pass without the feature, on the restatement of tests/level_util.py alone, and say that the
    definition of a level call is the right one: a key generated ONCE at the top level switches a ciphertext component at every
    level with the noise the mathematics allows, and one relinearisation key serves a chain of rescaling products from level L
    down to level 1."""
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from level_util import RowsOracle, keyswitch_level_rns, level_digits, mulrelin_level_rns
from mulrelin_util import relin_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_keyswitch_level_digits", "nflhip_keyswitch_level_ntt_dev", "nflhip_keyswitch_level_ntt", "nflhip_mulrelin_level_ntt_dev",
           "nflhip_mulrelin_level_ntt")


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code                                 # entries are added, the number stays
    assert "leveled key switching" in txt and "phys(r)" in txt                    # the header comment states the definition
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    import inspect
    for meth in ("key_switch_ntt", "h_key_switch_ntt", "mul_relin_ntt", "h_mul_relin_ntt", "keyswitch_digits"):
        assert inspect.signature(getattr(Engine, meth)).parameters["level"].default is None, meth
    assert callable(Engine.level_engine) and callable(Engine.level_rows)


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(1024, dtype=np.uint64)
    p = [buf.ctypes.data + 1024 * k for k in range(8)]
    # a NULL context is NFLHIP_ERR_INVALID before any device use, with a level of 0, past any L, and the rescale at level 1 alike: the
    # refusal is the NULL context's; the level checks themselves need a context (tests/test_gpu_level.py)
    for level, flags in ((0, 0), (2**64 - 1, 0), (1, _lib.MULRELIN_RESCALE), (1, 0)):
        assert L.nflhip_mulrelin_level_ntt_dev(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 1, level, flags, None) == _lib.ERR_INVALID == 1
        assert L.nflhip_mulrelin_level_ntt(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1, 1, 1, level, flags) == _lib.ERR_INVALID
    for level in (0, 2**64 - 1, 1):
        assert L.nflhip_keyswitch_level_ntt_dev(None, p[0], p[1], p[2], p[3], 1, 1, 1, level, 0, None) == _lib.ERR_INVALID
        assert L.nflhip_keyswitch_level_ntt(None, p[0], p[1], p[2], p[3], 1, 1, 1, level, 0) == _lib.ERR_INVALID
        assert L.nflhip_keyswitch_level_digits(None, 1, 1, level) == 0             # (the counts on a context: tests/test_gpu_level.py)
    assert [level_digits(lv, 2) for lv in (1, 2, 3, 4)] == [1, 1, 2, 2]       # (the restatement's own count, what the GPU test compares the entry with)


def _resource_report(tmp_path, stem):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", stem + ".hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / (stem + ".o"))], capture_output=True, text=True, timeout=1200)
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
    return kernels


def _demangled(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def test_new_kernel_instances_use_no_scratch_and_spill_no_register(tmp_path):
    """every kernel of kernels_level.hip (hipcc cross-compiles for gfx950 without a GPU): k_dot with the level key as its second
    operand, three limb widths x (16-byte groups, words) x (G = 4, 1); the one-launch kernel on the level key for the multiplication
    and for the key switch, three limb widths each, up to 1024 threads per workgroup (128 vector registers)"""
    kernels = _resource_report(tmp_path, "kernels_level")
    dot = {k: v for k, v in kernels.items() if "k_dot" in k and "DotKeyLevel" in k}
    mr = {k: v for k, v in kernels.items() if "k_tensor_modup_dot_fused" in k and "MrFusedArgsLevel" in k and "KsFusedArgsLevel" not in k}
    ks = {k: v for k, v in kernels.items() if "k_tensor_modup_dot_fused" in k and "KsFusedArgsLevel" in k}
    assert len(dot) == 12 and len(mr) == 3 and len(ks) == 3 and len(kernels) == 18, sorted(kernels)
    for name, v in sorted(kernels.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs", v["TotalSGPRs"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
    for name, v in list(mr.items()) + list(ks.items()):
        assert int(v["VGPRs"]) <= 128, name
    for name, v in dot.items():
        assert int(v["LDS Size [bytes/block]"]) == 0, name


def test_untouched_instances_keep_their_registers(tmp_path):
    """the instances on the context's own key layout are the same templates with another parameter and must compile to what they
    compiled to before: the u64 vector-register counts DESIGN.md records (5.12: k_dot 76 - 112 over its four strided u64 instances;
    5.16: k_modup_dot_fused 91; 5.19: k_tensor_modup_dot_fused 123, 5 short of its limit), nothing spilled that was not"""
    dot = _resource_report(tmp_path, "kernels_dot")
    names = _demangled(dot)
    u64 = sorted(int(v["VGPRs"]) for k, v in dot.items() if "k_dot<unsigned long" in names[k] and "DotStrided" in names[k])
    assert sum("k_dot<" in names[k] for k in dot) == 18 and u64 == [54, 76, 76, 112], u64
    assert all(int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0 and int(v["ScratchSize [bytes/lane]"]) == 0 for v in dot.values())
    ksw = _resource_report(tmp_path, "kernels_keyswitch")
    names = _demangled(ksw)
    got = [int(v["VGPRs"]) for k, v in ksw.items() if names[k].startswith("void nflhip::k_modup_dot_fused<unsigned long>")]
    assert got == [91], got
    mr = _resource_report(tmp_path, "kernels_mulrelin")
    names = _demangled(mr)
    got = [(int(v["VGPRs"]), int(v["SGPRs Spill"])) for k, v in mr.items() if "k_tensor_modup_dot_fused<unsigned long" in names[k]]
    assert got == [(123, 0)], got


# ---- the reference: these validate tests/level_util.py and would pass without the feature ----
def _setup(lb, n, nm, oracle_factory):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]], oracle_factory(lb, n, nm)


def _secret(P, n, orc, rnd):
    s = rnd.randint(-1, 2, size=n).astype(object)
    return orc.ntt(B.rows_of(s, P, range(len(P)), np.uint64)[None])[0].astype(object)


@pytest.mark.parametrize("K,alpha", [(2, 2), (1, 1)])
@pytest.mark.parametrize("centered", [False, True])
def test_one_top_level_key_switches_at_every_level(K, alpha, centered, oracle_factory):
    """VALIDATES THE REFERENCE ONLY.  u64/64/6, the key of tests/test_keyswitch_cpu.py generated once over the full context:
        key[d][0] = -a_d s + e_d + P g_d s',  key[d][1] = a_d,  g_d = (Q / Q_d) ((Q / Q_d)^-1 mod Q_d),  Q the TOP-level product.
    On a live row j < l, g_d is 1 when j is in digit d and 0 otherwise, whatever the level, so the rows [0, l) and [L, nm) of this key
    are a key of C_l with the digits cut at l.  |out0 + out1 s - in s'|_inf over Q_l is positive and within the bound of DESIGN.md
    5.16 with the level's digit count: n dnum_l alpha 8 2^alpha + n + 1.  (alpha <= K: hybrid switching needs P >= Q_d.)"""
    lb, n, nm = 64, 64, 6
    L = nm - K
    P, orc = _setup(lb, n, nm, oracle_factory)
    rnd = np.random.RandomState(100 * K + centered)
    S, S2 = _secret(P, n, orc, rnd), _secret(P, n, orc, rnd)
    key = relin_key(P, K, alpha, n, S, S2, orc, rnd)
    for level in range(1, L + 1):
        kept = RowsOracle(orc, nm, range(level))
        x = kept.ntt(B.random_batch(P[:level], n, 2, np.uint64, 5 + level))
        out0, out1 = keyswitch_level_rns(x, key, P, K, alpha, level, centered, False, orc)
        assert out0.shape == out1.shape == x.shape
        r = np.empty_like(x)
        for j in range(level):
            r[:, j] = ((out0[:, j].astype(object) + out1[:, j].astype(object) * S[j] - x[:, j].astype(object) * S2[j]) % P[j]).astype(np.uint64)
        norm = max(abs(int(v)) for v in B.centre(B.crt_rows(kept.intt(r), P, (0, level)), B.prod(P[:level])).ravel())
        bound = n * level_digits(level, alpha) * alpha * 8 * 2**alpha + n + 1
        print("K = alpha = %d, centred %d, level %d: |out0 + out1 s - in s'|_inf = %d, bound %d" % (K, centered, level, norm, bound))
        assert 0 < norm <= bound


@pytest.mark.parametrize("K,alpha", [(2, 2), (1, 1)])
def test_one_relinearisation_key_serves_a_chain_down_to_level_one(K, alpha, oracle_factory):
    """VALIDATES THE REFERENCE ONLY.  u64/64/6, s ternary, ONE key from s^2 to s.  Two small plaintexts are encrypted at the top level,
    multiplied with the rescale, and the product is squared with the rescale level by level down to level 1.  At every step, with
    q = p_(l-1) the dropped modulus and m_a, m_b the phases c0 + c1 s of the step's inputs over Q_l,
        | q (out0 + out1 s) - m_a m_b |_inf <= n dnum_l alpha 8 2^alpha + q (n + 1)        (with the level's digits)."""
    lb, n, nm = 64, 64, 6
    L = nm - K
    P, orc = _setup(lb, n, nm, oracle_factory)
    rnd = np.random.RandomState(900 + K)
    S = _secret(P, n, orc, rnd)
    S2 = np.empty_like(S)
    for j, p in enumerate(P):
        S2[j] = S[j] * S[j] % p
    key = relin_key(P, K, alpha, n, S, S2, orc, rnd)
    top = RowsOracle(orc, nm, range(L))

    def encrypt(seed):
        m = top.ntt(B.rows_of(rnd.randint(-4, 5, size=(2, n)).astype(object), P, range(L), np.uint64))
        c1 = top.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed))
        c0 = np.empty_like(c1)
        for j in range(L):
            c0[:, j] = ((m[:, j].astype(object) - c1[:, j].astype(object) * S[j]) % P[j]).astype(np.uint64)
        return c0, c1

    def phase(c0, c1, level):
        r = np.empty_like(c0)
        for j in range(level):
            r[:, j] = ((c0[:, j].astype(object) + c1[:, j].astype(object) * S[j]) % P[j]).astype(np.uint64)
        return B.crt_rows(RowsOracle(orc, nm, range(level)).intt(r), P, (0, level))

    a, b = encrypt(11), encrypt(12)
    for level in range(L, 1, -1):
        Q, q = B.prod(P[:level]), P[level - 1]
        ma, mb = (RowsOracle(orc, nm, range(level)).ntt(B.rows_of(phase(*c, level), P, range(level), np.uint64)) for c in (a, b))
        prod = np.empty_like(ma)
        for j in range(level):
            prod[:, j] = (ma[:, j].astype(object) * mb[:, j].astype(object) % P[j]).astype(np.uint64)
        M = B.crt_rows(RowsOracle(orc, nm, range(level)).intt(prod), P, (0, level))   # the negacyclic product m_a m_b over Q_l
        out = mulrelin_level_rns(a[0], a[1], b[0], b[1], key, P, K, alpha, level, False, False, True, orc)
        assert out[0].shape == out[1].shape == (2, level - 1, n)
        Y = phase(out[0], out[1], level - 1)
        norm = max(abs(int(v)) for v in B.centre((q * Y - M) % Q, Q).ravel())
        bound = n * level_digits(level, alpha) * alpha * 8 * 2**alpha + q * (n + 1)
        print("K = alpha = %d, level %d -> %d: |q (out0 + out1 s) - m_a m_b|_inf / q = %.3f, bound %.3f" % (K, level, level - 1, norm / q, bound / q))
        assert 0 < norm <= bound
        a = b = out
