"""CPU: the hybrid key switch in NTT form (include/nflhip.h "hybrid key switching").
  * the C ABI, the Python binding and the Engine carry the new names; a NULL context is refused without a device;
  * a REAL key switch on the restatement of tests/keyswitch_util.py alone: a key built from secrets s, s' and small errors switches
    a ciphertext component with the noise the mathematics allows -- the layout and the digit convention against the definition of a
    hybrid key switch, not only against ourselves;
  * the compiler's resource report for every kernel of kernels_keyswitch.hip;
  * the header layer (include/nfl_hip), through the program of tests/cpp_keyswitch against the CPU stand-in of tests/cpp/mock with a
    toy version of the new entry."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits, keyswitch_rns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_keyswitch")
ENTRIES = ("nflhip_keyswitch_ntt_dev", "nflhip_keyswitch_ntt", "nflhip_keyswitch_digits")
FLAGS = {"CENTERED": 0x100, "FLOOR": 0x200, "COMPOSED": 0x400, "FUSED": 0x800, "SEQUENCE": 0x1000}


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_KEYSWITCH_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in FLAGS}
    assert flags == FLAGS
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert {k: getattr(_lib, "KEYSWITCH_" + k) for k in FLAGS} == FLAGS
    for meth in ("key_switch_ntt", "h_key_switch_ntt", "keyswitch_digits"):
        assert callable(getattr(Engine, meth))
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("key_switch_ntt", "key_switch_into", "assign_key_switch"):
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
    for flags in (0,) + tuple(FLAGS.values()):
        assert L.nflhip_keyswitch_ntt_dev(None, p, p + 64, p + 128, p + 192, 1, 1, 1, flags, None) == _lib.ERR_INVALID == 1   # no device needed
        assert L.nflhip_keyswitch_ntt(None, p, p + 64, p + 128, p + 192, 1, 1, 1, flags) == _lib.ERR_INVALID
    assert L.nflhip_keyswitch_digits(None, 1, 1) == 0


def _ternary(rnd, n):
    return rnd.randint(-1, 2, size=n).astype(object)


def _rows(x, P, dtype):
    """residues of the integer polynomial x (object array [n]) under every modulus of P: [len(P), n]"""
    return B.rows_of(np.asarray(x, dtype=object), P, range(len(P)), dtype)


@pytest.mark.parametrize("K,alpha", [(1, 1), (2, 2)])
@pytest.mark.parametrize("centered", [False, True])
def test_a_real_key_switch_has_the_noise_the_mathematics_allows(K, alpha, centered, oracle_factory):
    """u64/64/5.  Q = the first L moduli, P = the last K, Q_d the digits' products, g_d = (Q/Q_d) ((Q/Q_d)^-1 mod Q_d).  With
        key[d][0] = -a_d s + e_d + P g_d s',   key[d][1] = a_d        mod Q P,  s, s' ternary, |e_d| <= 8,
    out0 + out1 s - in s' = (sum_d U_d e_d) / P + (the two roundings) mod Q.  U_d < alpha Q_d (fast: x + u Q_d, u < alpha; centred:
    |U_d| <= Q_d), Q_d < 2^(62 alpha), P > 2^(61 alpha), a negacyclic product of n terms, dnum digits, and each rounding is off by
    at most a half unit (a unit inside the band), one of them multiplied by the ternary s:
        | . |_inf <= n dnum alpha 8 2^alpha + n + 1."""
    from nfllib_amd.params import params
    lb, n, nm = 64, 64, 5
    L = nm - K
    P = [int(v) for v in params(lb).P[:nm]]
    orc, ok = oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    rnd = np.random.RandomState(100 * K + centered)
    Q, Ps = B.prod(P[:L]), B.prod(P[L:])
    S = digits(nm, K, alpha)
    dnum = len(S)
    s, s2 = _ternary(rnd, n), _ternary(rnd, n)
    S_ntt, S2_ntt = (orc.ntt(_rows(v, P, np.uint64)[None])[0].astype(object) for v in (s, s2))
    key = np.empty((dnum, 2, nm, n), dtype=np.uint64)
    for d, (s0, ks) in enumerate(S):
        Qd = B.prod(P[s0:s0 + ks])
        g = (Q // Qd) * pow((Q // Qd) % Qd, -1, Qd)
        a_ntt = B.random_batch(P, n, 1, np.uint64, 7 + d)[0]                      # uniform mod Q P, taken in NTT form
        e_ntt = orc.ntt(_rows(rnd.randint(-8, 9, size=n).astype(object), P, np.uint64)[None])[0]
        for j, p in enumerate(P):
            key[d, 0, j] = ((e_ntt[j].astype(object) - a_ntt[j].astype(object) * S_ntt[j] + (Ps * g) % p * S2_ntt[j]) % p).astype(np.uint64)
        key[d, 1] = a_ntt
    x_ntt = ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, 5))                     # the component to switch, uniform mod Q
    out0, out1 = keyswitch_rns(x_ntt, key, P, K, alpha, centered, False, orc, ok)
    r = np.empty_like(x_ntt)
    for j in range(L):
        p = P[j]
        r[:, j] = ((out0[:, j].astype(object) + out1[:, j].astype(object) * S_ntt[j] - x_ntt[:, j].astype(object) * S2_ntt[j]) % p).astype(np.uint64)
    err = B.centre(B.crt_rows(ok.intt(r), P, (0, L)), Q)
    norm = max(abs(int(v)) for v in err.ravel())
    bound = n * dnum * alpha * 8 * 2**alpha + n + 1
    print("K = alpha = %d, centred %d: |out0 + out1 s - in s'|_inf = %d, bound %d" % (K, centered, norm, bound))
    assert norm <= bound
    assert norm > 0                                                              # (the errors are there: the key is not exact)


def test_compiled_kernels_use_no_scratch_and_spill_no_vector_register(tmp_path):
    """the compiler's own resource report for every kernel of kernels_keyswitch.hip (hipcc cross-compiles for gfx950 without a GPU):
    the one-launch kernel runs up to 1024 threads per workgroup, which leaves it 128 vector registers; the streaming kernel uses no
    LDS"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_keyswitch.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_keyswitch.o")], capture_output=True, text=True, timeout=1200)
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
    fused = {k: v for k, v in kernels.items() if "k_modup_dot_fused" in k}
    stream = {k: v for k, v in kernels.items() if "k_modup_digits" in k}
    assert len(fused) == 3 and len(stream) == 18       # three limb widths; x (16-byte groups, words) x (K = 4, 16, 0)
    for name, v in sorted(kernels.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0, name
    for name, v in fused.items():
        assert int(v["VGPRs"]) <= 128, name
    for name, v in stream.items():
        assert int(v["LDS Size [bytes/block]"]) == 0, name


# ---- the header layer ----
def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_keyswitch: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock
    generated into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's
    failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "keyswitch_main.cpp")
    exe = os.path.join(out_dir, "keyswitch_test")
    if gpu:
        cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + inc, "-DNFL_HIP_NO_GMP", "-o", exe, main,
               "-L" + os.path.join(ROOT, "nfllib_amd"), "-lnflhip", "-Wl,-rpath," + os.path.join(ROOT, "nfllib_amd"), "-Wl,-rpath,/opt/rocm/lib"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return exe
    c = os.path.join(out_dir, "mock_backend.c")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "cpp", "mock", "make_mock_backend.py"), c], stdout=subprocess.DEVNULL)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + inc, "-o", os.path.join(out_dir, "libnflhip.so"), c, "-lpthread"])
    objs = []
    for toy in (os.path.join(SRC, "toy_keyswitch.c"), os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"),
                os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")):
        objs.append(os.path.join(out_dir, os.path.basename(toy)[:-2] + ".o"))
        subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-c", toy, "-o", objs[-1]])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-DNFL_HIP_NO_GMP", "-o", exe, main] + objs +
                          ["-L" + out_dir, "-lnflhip", "-Wl,-rpath," + out_dir])
    return exe


@pytest.fixture(scope="module")
def mock_exe(tmp_path_factory):
    return build_cpp(str(tmp_path_factory.mktemp("cpp_keyswitch")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other and with the sequence written by hand through
    the existing header calls"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # the key gathered in another order than [term][component]
    ("static_cast<char *>(kbuf) + t * pb, held[t]->dev_ro()", "static_cast<char *>(kbuf) + t * pb, held[t ^ 1]->dev_ro()"),
    # the outputs swapped
    ("nflhip_keyswitch_ntt_dev(ctx_t::get(), o0, o1, s, kbuf, 1,", "nflhip_keyswitch_ntt_dev(ctx_t::get(), o1, o0, s, kbuf, 1,"),
    # a batch call that forgets a mode
    ("const int flags = (centered ? NFLHIP_KEYSWITCH_CENTERED : 0) | (floor ? NFLHIP_KEYSWITCH_FLOOR : 0);\n    detail::check(key.ctx()",
     "const int flags = (floor ? NFLHIP_KEYSWITCH_FLOOR : 0);\n    detail::check(key.ctx()"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad):
    """mutants of the header must fail: the CPU stand-in keeps what the layer's correctness depends on"""
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hit = 0
    for hdr in (inc / "nfl_hip" / "batch.hpp", inc / "nfl_hip" / "poly_p.hpp"):
        text = hdr.read_text()
        hit += good in text
        hdr.write_text(text.replace(good, bad))
    assert hit == 1
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                           os.path.join(SRC, "keyswitch_main.cpp")] + [os.path.join(out, o) for o in ("toy_keyswitch.o", "toy_baseconv_ntt.o", "toy_baseconv.o")] +
                          ["-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
