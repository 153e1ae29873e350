"""CPU: the RNS base conversion and the mod-down by the last k moduli (include/nflhip.h "RNS base conversion").
  * the row formulas of tests/baseconv_util.py (which define the words) against the exact statement through the integer behind the
    residues, outside the band and -- with the band's own rule -- inside it; the bound on the fixed-point image; v - u in {0, 1};
  * the mod-down against floor(X / P), the nearest integer and, for k = 1, tests/rescale_util.py; one tie to the reference's lift;
  * the kernel's per-position arithmetic, compiled for the CPU (tests/cpp_baseconv/baseconv_pos_main.cpp, under
    -fsanitize=address,undefined), and the table records of host_tables.cpp, against Python integers;
  * the C ABI, the Python binding and the Engine carry the new names."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import baseconv_util as B
import rescale_util as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_baseconv")
ENTRIES = ("nflhip_baseconv_dev", "nflhip_baseconv", "nflhip_moddown_dev", "nflhip_moddown")
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
N = 16
# (limb_bits, nm, [(src, dst), ...]): prefix to suffix, suffix to prefix, middle to all, ks = 1, kd = 1, S = D
CASES = [(64, 4, [((0, 2), (2, 2)), ((2, 2), (0, 2)), ((1, 2), (0, 4)), ((3, 1), (0, 4)), ((0, 3), (3, 1)), ((0, 4), (0, 4))]),
         (32, 3, [((0, 2), (2, 1)), ((1, 2), (0, 1)), ((1, 1), (0, 3)), ((0, 3), (0, 3))]),
         (16, 2, [((0, 1), (1, 1)), ((1, 1), (0, 2)), ((0, 2), (0, 2))]),
         (64, 96, [((80, 16), (0, 20)), ((0, 17), (90, 6)), ((60, 33), (58, 38))])]


def moduli(lb, nm):
    from nfllib_amd.params import params
    return [int(v) for v in params(lb).P[:nm]]


def planted(P, lb, src, seed=3):
    """two random polynomials; the edge values in polynomial 0, the band values in polynomial 1"""
    a = B.random_batch(P, N, 2, _NP[lb], seed)
    B.plant(a, P, src, B.edge_values(P, src), b=0)
    B.plant(a, P, src, B.band_values(P, src, lb), b=1)
    return a


def test_definition_on_a_small_case():
    # moduli 5, 7 -> 11: Q = 35.  x = 17 = Q // 2: centred 17; x = 18: centred -17 = 5 mod 11.  (the words, not the fixed point, are
    # checked here: the toy moduli are not two bits below a word)
    P = [5, 7, 11]
    for x, c in ((0, 0), (1, 1), (17, 17 % 11), (18, (18 - 35) % 11), (34, (34 - 35) % 11)):
        a = np.array([[[x % 5], [x % 7], [0]]], dtype=np.uint64)
        assert B.crt_rows(a, P, (0, 2)).tolist() == [[x]]
        assert B.baseconv_exact(a, P, (0, 2), (2, 1), centered=True)[0, 2, 0] == c, x
        y, u, _ = B.parts(a, P, (0, 2))
        assert sum(int(yi[0, 0]) * (35 // p) for yi, p in zip(y, P)) == x + int(u[0, 0]) * 35 and 0 <= int(u[0, 0]) < 2


@pytest.mark.parametrize("lb,nm,pairs", CASES)
def test_row_formula_equals_the_exact_statement(lb, nm, pairs):
    P = moduli(lb, nm)
    for src, dst in pairs:
        a = planted(P, lb, src)
        _, u, v = B.parts(a, P, src)
        d = (v - u).astype(int)
        band = B.in_band(a, P, src)
        assert set(np.unique(d).tolist()) <= {0, 1}, (src, dst)
        fast = B.baseconv_rns(a, P, src, dst)
        assert np.array_equal(fast, B.baseconv_exact(a, P, src, dst))
        cen = B.baseconv_rns(a, P, src, dst, centered=True)
        # outside the band the exact statement has no freedom; inside it the output is x (v = u) or x - Q (v = u + 1)
        assert np.array_equal(cen, B.baseconv_exact(a, P, src, dst, centered=True, keep=band & (d == 0)))
        x = B.crt_rows(a, P, src)
        Q = B.prod(P[src[0]:src[0] + src[1]])
        below = np.frompyfunc(lambda t: bool(2 * t < Q), 1, 1)(x).astype(bool)
        assert not d[below].any() and d[~below & ~band].all(), (src, dst)
        for out in (fast, cen):
            keep = [j for j in range(nm) if not dst[0] <= j < dst[0] + dst[1]]
            assert np.array_equal(out[:, keep], a[:, keep])                         # rows outside D untouched
            both = [j for j in range(dst[0], dst[0] + dst[1]) if src[0] <= j < src[0] + src[1]]
            assert np.array_equal(out[:, both], a[:, both])                         # for j in S the formula gives x_j
            for j in range(dst[0], dst[0] + dst[1]):
                assert int(out[:, j].max()) < P[j]


@pytest.mark.parametrize("lb,idx", [(32, [0, 1, 290]), (64, [0, 1, 91, 92, 93, 95, 999])])
def test_fixed_point_bound_sampled(lb, idx):
    """0 <= 2^60 y / p - f < e on sampled words and y = p - 1, the large-delta 62-bit moduli past the 92nd included"""
    from nfllib_amd.params import params
    e = Fraction(5, 4) if lb == 64 else Fraction(2**(lb - 2))
    rnd = np.random.RandomState(11)
    for i in idx:
        p = int(params(lb).P[i])
        ys = [0, 1, 2, p // 2, p - 2, p - 1] + [int(rnd.randint(0, 2**31)) * int(rnd.randint(0, 2**31)) % p for _ in range(2000)]
        for y in ys:
            f = B.fixed(y, p, lb)
            assert 0 <= Fraction(2**60 * y, p) - f < e and 0 <= f < 2**60, (i, y)


def test_fixed_point_bound_exhaustive_14_bits():
    p = moduli(16, 1)[0]
    assert 2**13 < p < 2**14
    worst = max(Fraction(2**60 * y, p) - B.fixed(y, p, 16) for y in range(p))
    assert 0 <= worst < 2**14
    assert all(Fraction(2**60 * y, p) >= B.fixed(y, p, 16) for y in range(p))


@pytest.mark.parametrize("lb,nm,src", [(64, 4, (0, 2)), (64, 4, (3, 1)), (64, 96, (60, 33)), (32, 3, (0, 2)), (32, 3, (2, 1)), (16, 2, (0, 2))])
def test_v_minus_u_inside_and_at_both_edges_of_the_band(lb, nm, src):
    P = moduli(lb, nm)
    vals = B.band_values(P, src, lb)
    a = B.plant(np.zeros((1, nm, len(vals)), dtype=_NP[lb]), P, src, vals)
    _, u, v = B.parts(a, P, src)
    d = (v - u).astype(int)[0]
    Q, w = B.prod(P[src[0]:src[0] + src[1]]), B.band(P, src, lb)
    for x, dx in zip(vals, d.tolist()):
        assert dx in (0, 1)
        if 2 * x < Q:
            assert dx == 0, x
        elif Fraction(x, Q) >= Fraction(1, 2) + w:
            assert dx == 1, x
    assert d[0] == 0 and d[-1] == 1                     # just below and just above
    assert w < Fraction(1, 2)                            # ks e / 2^60 < 1/2: the rounding cannot skip an integer


@pytest.mark.parametrize("lb,nm,ks", [(64, 4, 1), (64, 4, 2), (64, 4, 3), (32, 3, 2), (32, 3, 1), (16, 2, 1), (64, 96, 17)])
def test_mod_down_against_python_integers(lb, nm, ks):
    P = moduli(lb, nm)
    src = (nm - ks, ks)
    a = planted(P, lb, src, seed=5)
    band = B.in_band(a, P, src)
    got, flo = B.moddown_rns(a, P, ks), B.moddown_rns(a, P, ks, floor=True)
    assert np.array_equal(flo, B.moddown_exact(a, P, ks, "approx"))
    near, down = B.moddown_exact(a, P, ks, "nearest"), B.moddown_exact(a, P, ks, "floor")
    out = ~band
    assert np.array_equal(np.where(out[:, None, :], got, 0), np.where(out[:, None, :], near, 0))
    # everywhere: floor(X / P) or floor(X / P) + 1
    up = np.all(got == near, axis=1) | np.all(got == down, axis=1)
    assert up.all()
    # inside the band the fraction is at least 1/2: "nearest" is floor + 1, the result may be either
    assert np.all(np.all(got == down, axis=1)[band] | np.all(got == near, axis=1)[band])


@pytest.mark.parametrize("lb,nm", [(64, 4), (32, 3), (16, 2)])
def test_mod_down_by_one_modulus_is_rescale_outside_the_band(lb, nm):
    P = moduli(lb, nm)
    a = planted(P, lb, (nm - 1, 1), seed=8)
    band = B.in_band(a, P, (nm - 1, 1))
    got, want = B.moddown_rns(a, P, 1), R.rescale_rns(a, P)
    assert np.array_equal(np.where(band[:, None, :], 0, got), np.where(band[:, None, :], 0, want))
    assert (~band).sum() > band.size // 2


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 4), (32, 1024, 3)])
def test_exact_statement_agrees_with_the_reference_lift(lb, n, nm, oracle_factory):
    """the integer behind ALL rows from Reference.crt_lift (the real reference's CRT) where oracle/_ref is built and instantiates
    the shape, else from Oracle.crt_lift: it equals crt_rows over every row, and its centred residues are the conversion's"""
    P = moduli(lb, nm)
    o = oracle_factory(lb, n, nm)
    a = o.fill_uniform(2, 5, 0)
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
    assert np.array_equal(X, B.crt_rows(a, P, (0, nm)))
    Q = B.prod(P)
    assert not B.in_band(a, P, (0, nm)).any()
    assert np.array_equal(B.rows_of(B.centre(X, Q), P, range(nm), _NP[lb]), B.baseconv_rns(a, P, (0, nm), (0, nm), centered=True))
    k = 1
    Pk = P[-1]
    Y = X // Pk + (2 * (X % Pk) >= Pk).astype(object)
    assert np.array_equal(B.rows_of(Y % (Q // Pk), P, range(nm - k), _NP[lb]), B.moddown_rns(a, P, k))


# ---- the kernel's per-position arithmetic and the table records, compiled for the CPU ----
@pytest.fixture(scope="module")
def pos_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("cpp_baseconv")), "baseconv_pos")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(SRC, "shim"), "-o", exe, os.path.join(SRC, "baseconv_pos_main.cpp"),
           os.path.join(ROOT, "nfllib_amd", "csrc", "host_tables.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_conv(exe, lb, P, a, src, dst, mode, plan):
    """a = [nm, npos] words of one polynomial -> [kd, npos]"""
    nm, npos = a.shape
    text = "%d\n%s\n" % (nm, " ".join(str(p) for p in P)) + "".join(" ".join(str(int(a[i, t])) for i in range(nm)) + "\n" for t in range(npos))
    r = subprocess.run([exe, "conv", str(lb), str(src[0]), str(src[1]), str(dst[0]), str(dst[1]), str(mode), str(plan), str(npos)],
                       input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.array([[int(w) for w in line.split()] for line in r.stdout.splitlines()], dtype=object).T


@pytest.mark.parametrize("lb,nm,pairs", CASES)
def test_kernel_arithmetic_on_the_cpu_equals_the_restatement(lb, nm, pairs, pos_exe):
    P = moduli(lb, nm)
    for src, dst in pairs:
        a = planted(P, lb, src)
        # the largest accumulators: every source word p_i - 1, and every y_i = p_i - 1
        a[0, src[0]:src[0] + src[1], N - 1] = [p - 1 for p in P[src[0]:src[0] + src[1]]]
        a[0, src[0]:src[0] + src[1], N - 2] = B.all_y_max(P, src)
        flat = np.concatenate([a[0], a[1]], axis=1)
        for centred in (0, 1):
            want = B.baseconv_rns(flat[None], P, src, dst, centered=bool(centred))[0, dst[0]:dst[0] + dst[1]].astype(object)
            for plan in ([0, 1] if src[1] <= 16 else [0]):
                got = run_conv(pos_exe, lb, P, flat, src, dst, centred, plan)
                assert np.array_equal(got, want), (src, dst, centred, plan)
    for k in sorted({1, nm - 1, min(17, nm - 1)}):
        a = planted(P, lb, (nm - k, k), seed=9)
        flat = np.concatenate([a[0], a[1]], axis=1)
        for floor in (0, 1):
            want = B.moddown_rns(flat[None], P, k, floor=bool(floor))[0].astype(object)
            got = run_conv(pos_exe, lb, P, flat, (nm - k, k), (0, nm - k), 2 | (0 if floor else 1), 1 if k <= 16 else 0)
            assert np.array_equal(got, want), (k, floor)


def run_record(exe, lb, P, src, dst, moddown):
    text = "%d\n%s\n" % (len(P), " ".join(str(p) for p in P))
    r = subprocess.run([exe, "record", str(lb), str(src[0]), str(src[1]), str(dst[0]), str(dst[1]), str(int(moddown))], input=text,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rc, _, err = lines[0].partition(" ")
    return int(rc), err, [int(w) for w in lines[1:]]


@pytest.mark.parametrize("lb,nm,pairs", CASES)
def test_table_records_equal_their_definitions(lb, nm, pairs, pos_exe):
    P = moduli(lb, nm)
    todo = [(s, d, False) for s, d in pairs] + [((nm - k, k), (0, nm - k), True) for k in sorted({1, nm - 1})]
    for src, dst, down in todo:
        rc, err, rec = run_record(pos_exe, lb, P, src, dst, down)
        assert rc == 0, err
        (s0, ks), (d0, kd) = src, dst
        Ps = P[s0:s0 + ks]
        Q = B.prod(Ps)
        want = []
        for p in Ps:
            inv = pow(Q // p % p, -1, p)
            want += [inv, (inv << lb) // p, p, (2**124 if lb == 64 else 2**60) // p]
        for j in range(d0, d0 + kd):
            p = P[j]
            Qj = Q % p
            inv = pow(Qj, -1, p) if down else 0
            want += [p, Qj, (Qj << lb) // p, inv, (inv << lb) // p, 0, 0, 0]
        for j in range(d0, d0 + kd):
            want += [Q // p % P[j] for p in Ps]
        assert rec == want, (src, dst, down)


def test_table_builder_refusals(pos_exe):
    P = moduli(64, 4)
    for src, dst, down in (((0, 0), (0, 1), False), ((0, 1), (0, 0), False), ((3, 2), (0, 1), False), ((0, 1), (4, 1), False),
                           ((0, 5), (0, 1), False), ((1, 2), (0, 1), True), ((2, 2), (0, 1), True)):
        rc, err, _ = run_record(pos_exe, 64, P, src, dst, down)
        assert rc == 1 and err, (src, dst, down)
    dup = [P[0], P[1], P[0]]
    assert run_record(pos_exe, 64, dup, (0, 3), (0, 3), False)[:2] == (1, "baseconv: a source modulus repeats")
    assert run_record(pos_exe, 64, dup, (0, 2), (2, 1), False)[0] == 0           # a destination may repeat a source modulus
    assert run_record(pos_exe, 64, dup, (2, 1), (0, 2), True)[:2] == (1, "moddown: a kept modulus repeats a dropped one")


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    assert "#define NFLHIP_BASECONV_CENTERED" in code and "#define NFLHIP_MODDOWN_FLOOR" in code
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    for meth in ("baseconv", "mod_up", "mod_down", "h_baseconv", "h_mod_down"):
        assert callable(getattr(Engine, meth))


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    assert _lib.lib.nflhip_baseconv_dev(None, p, p, 1, 0, 1, 0, 1, 0, None) == _lib.ERR_INVALID == 1   # NULL context: no device needed
    assert _lib.lib.nflhip_baseconv(None, p, p, 1, 0, 1, 0, 1, 0) == _lib.ERR_INVALID
    assert _lib.lib.nflhip_moddown_dev(None, p, p + 64, 1, 1, 0, None) == _lib.ERR_INVALID
    assert _lib.lib.nflhip_moddown(None, p, p + 64, 1, 1, 0) == _lib.ERR_INVALID


def test_compiled_kernels_use_no_scratch_no_lds_and_spill_no_vector_register(tmp_path):
    """the compiler's own resource report for every variant of k_baseconv (hipcc cross-compiles for gfx950 without a GPU): the
    kernel keeps its scalar operands out of the grid-stride loop's invariants by hand (kernels_baseconv.hip), which a compiler
    update could undo -- this is where that would show.  Scalar registers parked in VGPR lanes are reported, not memory."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_baseconv.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_baseconv.o")], capture_output=True, text=True, timeout=1200)
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
    variants = {k: v for k, v in kernels.items() if "k_baseconv" in k}
    assert len(variants) == 18                       # three limb widths x (16-byte groups, words) x (K = 4, 16, 0)
    for name, v in sorted(variants.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0, name
        assert int(v["LDS Size [bytes/block]"]) == 0, name
        assert int(v["VGPRs"]) <= 256, name
