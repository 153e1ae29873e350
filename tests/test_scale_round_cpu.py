"""CPU: the RNS scale-and-round by t/Q and the BFV product built on it (include/nflhip.h "BFV multiplication").
  * the row formulas of tests/scale_round_util.py (which define the words) against the exact statement through the integer, outside
    the two bands and -- with each band's own rule -- inside them, on random words and on values planted at both roundings; v - u
    reaches 0 and 1 in each stage.  These two validate the REFERENCE only;
  * a toy BFV encrypt -> tensor -> scale-round -> decrypt recovers m1 m2 mod t under the stated bound;
  * the table record of host_tables.cpp (tests/cpp_scale_round/record_main.cpp, under -fsanitize=address,undefined) against its
    definition on Python integers, and the builder's refusals;
  * the C ABI, the Python binding and the Engine carry the new names; the library exports them and validates without a device;
  * the compiler's resource report of kernels_scale_round.hip: no register-plan variant uses scratch or LDS or spills a VGPR."""
import os
import re
import subprocess

import numpy as np
import pytest

import baseconv_util as B
import scale_round_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nflhip_scale_round_dev", "nflhip_scale_round", "nflhip_scale_round_ntt_dev", "nflhip_scale_round_ntt",
           "nflhip_bfv_tensor_ntt_dev", "nflhip_bfv_tensor_ntt")
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
N = 16
SHAPES = [(64, 5, 2, 65537), (64, 9, 4, 2**58 + 12345), (32, 5, 2, 257), (32, 3, 1, 2**29 - 1), (16, 2, 1, 257)]


def moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


def planted(P, lb, ks, t, seed=3, n=N):
    """three polynomials of random full-range words; the values that put z on the edges and the band of the first rounding in
    polynomial 0, those that put Y on the edges and the band of the second conversion in polynomial 1"""
    a = B.random_batch(P, n, 3, _NP[lb], seed)
    S.plant_integers(a, P, S.first_round_values(P, ks, t, lb), b=0)
    S.plant_integers(a, P, S.second_round_values(P, ks, t, lb), b=1)
    return a


def test_definition_on_a_small_case():
    # moduli 5, 7 | 11, 13: Q = 35, B = 143, t = 3.  (the exact statement alone: the toy moduli are not two bits below a word)
    P, t = [5, 7, 11, 13], 3
    for X, Y in ((0, 0), (1, 0), (6, 1), (-6, -1), (17, 1), (18, 2), (-18, -2), (700, 60), (-705, -60)):   # |Y| < B / 2
        assert Y == (2 * t * X + 35) // 70
        a = S.integers_to_rows(np.array([[X]], dtype=object), P, np.uint64)
        assert S.scale_round_exact(a, P, 2, t, keep=True)[0, :, 0].tolist() == [Y % 11, Y % 13]
        assert S.scale_round_exact(a, P, 2, t)[0, :, 0].tolist() == [Y % 5, Y % 7]


@pytest.mark.parametrize("lb,nm,ks,t", SHAPES)
def test_row_formulas_equal_the_exact_statement(lb, nm, ks, t):
    P = moduli(lb, nm)
    kd = nm - ks
    a = planted(P, lb, ks, t)
    z, Yf = S.stages(a, P, ks, t)
    _, u1, v1 = B.parts(z, P, (0, ks))
    _, u2, v2 = B.parts(Yf, P, (ks, kd))
    d1, d2 = (v1 - u1).astype(int), (v2 - u2).astype(int)
    band1, band2 = B.in_band(z, P, (0, ks)), B.in_band(Yf, P, (ks, kd))
    assert set(np.unique(d1).tolist()) == {0, 1} and set(np.unique(d2).tolist()) == {0, 1}      # both roundings reach both sides
    assert lb == 16 or (band1.any() and band2.any())                 # (14-bit moduli: the bands hold no integer)
    keep1, keep2 = band1 & (d1 == 0), band2 & (d2 == 0)
    got, kept = S.scale_round_rns(a, P, ks, t), S.scale_round_rns(a, P, ks, t, keep=True)
    assert got.shape == (3, ks, N) and kept.shape == (3, kd, N)
    # with each band's own rule the two statements agree everywhere
    assert np.array_equal(kept, S.scale_round_exact(a, P, ks, t, keep=True, keep1=keep1))
    assert np.array_equal(got, S.scale_round_exact(a, P, ks, t, keep1=keep1, keep2=keep2))
    # outside the bands the exact statement has no freedom
    free = ~band1
    assert np.array_equal(np.where(free[:, None, :], kept, 0), np.where(free[:, None, :], S.scale_round_exact(a, P, ks, t, keep=True), 0))
    free = ~band1 & ~band2
    assert np.array_equal(np.where(free[:, None, :], got, 0), np.where(free[:, None, :], S.scale_round_exact(a, P, ks, t), 0))
    assert free.sum() > free.size // 2
    # the floor mode: floor(t X / Q) - u, then the centred conversion with its own band
    _, Yff = S.stages(a, P, ks, t, floor=True)
    _, uf, vf = B.parts(Yff, P, (ks, kd))
    keepf = B.in_band(Yff, P, (ks, kd)) & ((vf - uf).astype(int) == 0)
    assert np.array_equal(S.scale_round_rns(a, P, ks, t, floor=True, keep=True), S.scale_round_exact(a, P, ks, t, floor=True, keep=True))
    assert np.array_equal(S.scale_round_rns(a, P, ks, t, floor=True), S.scale_round_exact(a, P, ks, t, floor=True, keep2=keepf))
    for out, rows in ((got, range(ks)), (kept, range(ks, nm))):
        for k, j in enumerate(rows):
            assert int(out[:, k].max()) < P[j]


@pytest.mark.parametrize("lb,nm,ks,t", SHAPES)
def test_planted_values_land_where_the_recipe_says(lb, nm, ks, t):
    P = moduli(lb, nm)
    Q, Bp = B.prod(P[:ks]), B.prod(P[ks:])
    first, second = S.first_round_values(P, ks, t, lb), S.second_round_values(P, ks, t, lb)
    want_z = B.edge_values(P, (0, ks)) + B.band_values(P, (0, ks), lb)
    want_y = B.edge_values(P, (ks, nm - ks)) + B.band_values(P, (ks, nm - ks), lb)
    assert [(t * X) % Q for X in first] == want_z
    assert [((t * X) // Q) % Bp for X in second] == want_y and all(2 * abs(X) < Q * Bp for X in second)
    assert [((2 * t * X + Q) // (2 * Q)) % Bp for X in second] == want_y              # the rounding gives y too
    a = S.plant_integers(np.zeros((1, nm, len(second)), dtype=_NP[lb]), P, second)
    assert [int(x) for x in B.crt_rows(S.stages(a, P, ks, t)[1], P, (ks, nm - ks))[0]] == want_y


def test_the_result_does_not_depend_on_the_representative():
    """the rows of X and of X + m Q B are the same words, and the kept rows are round(t X_c / Q) of the CENTRED integer behind them,
    negative ones and ones next to +- Q B / 2 included"""
    P, ks, t = moduli(64, 5), 2, 65537
    QB = B.prod(P)
    Q = B.prod(P[:2])
    X = np.array([[123456789 * 10**20, -987654321 * 10**15, QB // 2 - Q // 4, -(QB // 2) + Q // 4]], dtype=object)   # (t X / Q: fractions near 3/4, 1/4)
    a, b = S.integers_to_rows(X, P, np.uint64), S.integers_to_rows(X + 3 * QB, P, np.uint64)
    assert np.array_equal(a, b)
    Y = (2 * t * X + Q) // (2 * Q)
    assert np.array_equal(S.scale_round_rns(a, P, ks, t, keep=True), B.rows_of(Y, P, range(2, 5), np.uint64))


def test_toy_bfv_product_decrypts():
    """n = 16, u32, L = 2, kb = 3, t = 257, ternary secret, noise in [-3, 3]: n Q^2 / 2 < Q B / 2 and t n Q / 2 + 1 < B / 2"""
    lb, L, kb, t, n = 32, 2, 3, 257, 16
    P = moduli(lb, L + kb)
    Q, Bp = B.prod(P[:L]), B.prod(P[L:])
    assert n * Q * Q // 2 < Q * Bp // 2 and t * n * Q // 2 + 1 < Bp // 2
    rnd = np.random.RandomState(12)
    s = S.bfv_keygen(n, rnd)
    m1, m2 = [int(x) for x in rnd.randint(0, t, size=n)], [int(x) for x in rnd.randint(0, t, size=n)]
    c1, c2 = S.bfv_encrypt(m1, s, Q, t, rnd), S.bfv_encrypt(m2, s, Q, t, rnd)
    assert S.bfv_decrypt(c1, s, Q, t) == m1 and S.bfv_decrypt(c2, s, Q, t) == m2
    want = [x % t for x in S.negacyclic(m1, m2)]
    for b, name in ((c2, "product"), (c1, "square")):
        tens = S.bfv_tensor_integers(c1, b, Q)
        assert all(2 * abs(x) < Q * Bp for comp in tens for x in comp)
        d = [S.rows_to_list(S.scale_round_rns(S.lists_to_rows(comp, P, np.uint32), P, L, t)[0], P[:L]) for comp in tens]
        assert S.bfv_decrypt(d, s, Q, t) == (want if name == "product" else [x % t for x in S.negacyclic(m1, m1)]), name
        # ... and the scaled components are round(t d / Q) exactly: no position is near either band
        for comp, got in zip(tens, d):
            assert got == [((2 * t * x + Q) // (2 * Q)) % Q for x in comp]


@pytest.fixture(scope="module")
def record_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("cpp_scale_round")), "record")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "cpp_scale_round", "record_main.cpp"), os.path.join(ROOT, "nfllib_amd", "csrc", "host_tables.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_record(exe, lb, P, ks, t):
    text = "%d\n%s\n" % (len(P), " ".join(str(p) for p in P))
    r = subprocess.run([exe, str(lb), str(ks), str(t)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rc, _, err = lines[0].partition(" ")
    return int(rc), err, [int(w) for w in lines[1:]]


@pytest.mark.parametrize("lb,nm,ks,t", SHAPES + [(32, 36, 17, 257)])
def test_table_record_equals_its_definition(lb, nm, ks, t, record_exe):
    """the (S -> D) record with t folded into the source constants and Q^-1, t on the destination rows; padded to 32 bytes; then the
    plain (D -> S) record of the base conversion"""
    P = moduli(lb, nm)
    rc, err, rec = run_record(record_exe, lb, P, ks, t)
    assert rc == 0, err
    kd = nm - ks
    recip = 2**124 if lb == 64 else 2**60
    want = []
    Q = B.prod(P[:ks])
    for p in P[:ks]:
        w = t * pow(Q // p % p, -1, p) % p
        want += [w, (w << lb) // p, p, recip // p]
    for p in P[ks:]:
        Qj, inv = Q % p, pow(Q % p, -1, p)
        want += [p, Qj, (Qj << lb) // p, inv, (inv << lb) // p, t, (t << lb) // p, 0]
    for pj in P[ks:]:
        want += [Q // p % pj for p in P[:ks]]
    want += [0] * (-len(want) % 4)
    Bp = B.prod(P[ks:])
    for p in P[ks:]:
        inv = pow(Bp // p % p, -1, p)
        want += [inv, (inv << lb) // p, p, recip // p]
    for p in P[:ks]:
        want += [p, Bp % p, ((Bp % p) << lb) // p, 0, 0, 0, 0, 0]
    for pi in P[:ks]:
        want += [Bp // p % pi for p in P[ks:]]
    assert rec == want


def test_table_builder_refusals(record_exe):
    P = moduli(64, 4)
    for ks, t in ((0, 3), (4, 3), (5, 3), (2, 0), (2, 2**61)):
        rc, err, _ = run_record(record_exe, 64, P, ks, t)
        assert rc == 1 and err, (ks, t)
    assert run_record(record_exe, 64, P, 2, 2**61 - 1)[0] == 0 and run_record(record_exe, 32, moduli(32, 3), 1, 2**29)[0] == 1
    for dup, ks in (([P[0], P[0], P[1]], 2), ([P[0], P[1], P[1]], 1), ([P[0], P[1], P[0]], 1), ([P[0], P[1], P[0]], 2)):
        rc, err, _ = run_record(record_exe, 64, dup, ks, 3)
        assert rc == 1 and "repeats" in err, (dup, ks)


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    for flag, val in (("FLOOR", 0x100), ("KEEP", 0x200), ("TWO_PASS", 0x400)):
        assert re.search(r"#define NFLHIP_SCALE_ROUND_%s 0x%x\b" % (flag, val), code), flag
    from nfllib_amd import Engine, _lib
    assert (_lib.SCALE_ROUND_FLOOR, _lib.SCALE_ROUND_KEEP, _lib.SCALE_ROUND_TWO_PASS) == (0x100, 0x200, 0x400)
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    for meth in ("scale_round", "h_scale_round", "bfv_tensor_ntt", "h_bfv_tensor_ntt", "bfv_mul_relin_ntt"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    assert L.nflhip_scale_round_dev(None, p, p + 256, 1, 1, 3, 0, None) == _lib.ERR_INVALID == 1   # NULL context: no device needed
    assert L.nflhip_scale_round(None, p, p + 256, 1, 1, 3, 0) == _lib.ERR_INVALID
    assert L.nflhip_scale_round_ntt_dev(None, p, p + 256, 1, 1, 3, 0, None) == _lib.ERR_INVALID
    assert L.nflhip_scale_round_ntt(None, p, p + 256, 1, 1, 3, 0) == _lib.ERR_INVALID
    assert L.nflhip_bfv_tensor_ntt_dev(None, p, p, p, p, p, None, None, 1, 1, 3, 0, None) == _lib.ERR_INVALID
    assert L.nflhip_bfv_tensor_ntt(None, p, p, p, p, p, None, None, 1, 1, 3, 0) == _lib.ERR_INVALID


def test_compiled_kernels_use_no_scratch_no_lds_and_spill_no_vector_register(tmp_path):
    """the compiler's own resource report for every variant of k_scale_round (hipcc cross-compiles for gfx950 without a GPU): the
    register plans keep nm source words, the kd words Y and their y_j per position, which a compiler update could push into scratch --
    this is where that would show.  Scalar registers parked in VGPR lanes are reported, not memory."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_scale_round.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_scale_round.o")], capture_output=True, text=True, timeout=1200)
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
    variants = {k: v for k, v in kernels.items() if "k_scale_round" in k}
    assert len(variants) == 18                       # three limb widths x (16-byte groups, words) x (<4, 5>, <8, 9>, chunked)
    for name, v in sorted(variants.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0, name
        assert int(v["LDS Size [bytes/block]"]) == 0, name
        assert int(v["VGPRs"]) <= 256, name
