"""CPU: hoisted rotations and the several-output sum of products (include/nflhip.h "hoisted rotations", "sums of products, several
outputs").
  * the C ABI, the Python binding and the Engine carry the new names; a NULL context is refused without a device;
  * a REAL rotation on the restatement of tests/rotate_util.py alone: Galois keys built by the header's convention (from s to
    sigma_(k^-1)(s)) rotate a ciphertext with the noise the mathematics allows -- the convention and the order "permutation last"
    against the definition of a rotation, not only against ourselves;
  * the compiler's resource report for every instance of k_dot_multi and k_permute_add_ntt;
  * the header layer (include/nfl_hip), through the program of tests/cpp_rotate against the CPU stand-in of tests/cpp/mock with toy
    versions of the new entries, and mutants of the header that the program must notice."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import baseconv_util as B
from automorph_util import sigma_ntt
from keyswitch_util import digits
from rotate_util import rotate_rns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_rotate")
ENTRIES = ("nflhip_dot_multi_dev", "nflhip_rotate_hoisted_ntt_dev", "nflhip_rotate_hoisted_ntt")
FLAGS = {"CENTERED": 0x100, "FLOOR": 0x200, "SEQUENCE": 0x1000, "HOISTED": 0x2000}


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_ROTATE_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in FLAGS}
    assert flags == FLAGS
    assert re.search(r"#define\s+NFLHIP_ROTATE_MAX_OUTPUTS\s+16\b", code) and re.search(r"#define\s+NFLHIP_DOT_MULTI_MAX_OUTPUTS\s+32\b", code)
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert {k: getattr(_lib, "ROTATE_" + k) for k in FLAGS} == FLAGS
    assert _lib.ROTATE_MAX_OUTPUTS == 16 and _lib.DOT_MULTI_MAX_OUTPUTS == 32
    for meth in ("dot_multi", "rotate_hoisted_ntt", "h_rotate_hoisted_ntt"):
        assert callable(getattr(Engine, meth))
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("rotate_hoisted_ntt", "rotate_into", "assign_rotations"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


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
    o0, o1, keys, ks = (C.c_void_p * 1)(p), (C.c_void_p * 1)(p + 64), (C.c_void_p * 1)(p + 192), (C.c_uint64 * 1)(5)
    for flags in (0,) + tuple(FLAGS.values()):
        assert L.nflhip_rotate_hoisted_ntt_dev(None, o0, o1, None, p + 128, keys, ks, 1, 1, 1, 1, flags, None) == _lib.ERR_INVALID == 1   # no device needed
        assert L.nflhip_rotate_hoisted_ntt(None, o0, o1, None, p + 128, keys, ks, 1, 1, 1, 1, flags) == _lib.ERR_INVALID
    a = _lib.DotOperand(p + 128, 1, 1)
    for flags in (0, _lib.DOT_UNTILED):
        assert L.nflhip_dot_multi_dev(None, o0, C.byref(a), keys, 1, 1, 1, 1, flags, None) == _lib.ERR_INVALID


def _rows(x, P, dtype):
    """residues of the integer polynomial x (object array [n]) under every modulus of P: [len(P), n]"""
    return B.rows_of(np.asarray(x, dtype=object), P, range(len(P)), dtype)


@pytest.mark.parametrize("K,alpha,k", [(1, 1, 5), (2, 2, 127), (2, 1, 25)])
@pytest.mark.parametrize("centered", [False, True])
def test_a_real_rotation_has_the_noise_the_mathematics_allows(K, alpha, k, centered, oracle_factory):
    """u64/64/5 (k = 127 is 2n - 1).  With the keys of the header's convention,
        key[d][0] = -a_d sigma_(k^-1)(s) + e_d + P g_d s,   key[d][1] = a_d        mod Q P,  s ternary, |e_d| <= 8,
    the key switch of c1 gives d0 + d1 sigma_(k^-1)(s) = c1 s + noise, so y0 + d1 sigma_(k^-1)(s) = c0 + c1 s + noise and, sigma_k
    being a ring automorphism applied LAST, out0 + out1 s = sigma_k(c0 + c1 s) + sigma_k(noise): the noise of one key switch,
    permuted and signed, which keeps its infinity norm -- the bound of tests/test_keyswitch_cpu.py,
        0 < | . |_inf <= n dnum alpha 8 2^alpha + n + 1        (K >= alpha: a valid hybrid parameter set)."""
    from nfllib_amd.params import params
    lb, n, nm = 64, 64, 5
    assert k % 2 == 1 and K >= alpha and (k != 127 or k == 2 * n - 1)
    L = nm - K
    P = [int(v) for v in params(lb).P[:nm]]
    orc, ok = oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    rnd = np.random.RandomState(1000 * K + 10 * alpha + centered)
    Q, Ps = B.prod(P[:L]), B.prod(P[L:])
    S = digits(nm, K, alpha)
    dnum = len(S)
    kinv = pow(k, -1, 2 * n)
    s = rnd.randint(-1, 2, size=n).astype(object)
    S_ntt = orc.ntt(_rows(s, P, np.uint64)[None])[0]
    Sinv_ntt = sigma_ntt(S_ntt, kinv).astype(object)          # sigma_(k^-1)(s), NTT form
    S_ntt = S_ntt.astype(object)
    key = np.empty((dnum, 2, nm, n), dtype=np.uint64)
    for d, (s0, ks) in enumerate(S):
        Qd = B.prod(P[s0:s0 + ks])
        g = (Q // Qd) * pow((Q // Qd) % Qd, -1, Qd)
        a_ntt = B.random_batch(P, n, 1, np.uint64, 7 + d)[0]                      # uniform mod Q P, taken in NTT form
        e_ntt = orc.ntt(_rows(rnd.randint(-8, 9, size=n).astype(object), P, np.uint64)[None])[0]
        for j, p in enumerate(P):
            key[d, 0, j] = ((e_ntt[j].astype(object) - a_ntt[j].astype(object) * Sinv_ntt[j] + (Ps * g) % p * S_ntt[j]) % p).astype(np.uint64)
        key[d, 1] = a_ntt
    c0, c1 = (ok.ntt(B.random_batch(P[:L], n, 2, np.uint64, seed)) for seed in (5, 6))   # a ciphertext, uniform mod Q
    (out0, out1), = rotate_rns(c0, c1, [key], [k], P, K, alpha, centered, False, orc, ok)
    m = np.empty_like(c0)                                                         # c0 + c1 s
    for j in range(L):
        m[:, j] = ((c0[:, j].astype(object) + c1[:, j].astype(object) * S_ntt[j]) % P[j]).astype(np.uint64)
    want = sigma_ntt(m, k)
    r = np.empty_like(c0)
    for j in range(L):
        r[:, j] = ((out0[:, j].astype(object) + out1[:, j].astype(object) * S_ntt[j] - want[:, j].astype(object)) % P[j]).astype(np.uint64)
    err = B.centre(B.crt_rows(ok.intt(r), P, (0, L)), Q)
    norm = max(abs(int(v)) for v in err.ravel())
    bound = n * dnum * alpha * 8 * 2**alpha + n + 1
    print("K %d alpha %d k %d centred %d: |out0 + out1 s - sigma_k(c0 + c1 s)|_inf = %d, bound %d" % (K, alpha, k, centered, norm, bound))
    assert 0 < norm <= bound


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


@pytest.mark.parametrize("stem,kernel,instances,lds", [
    ("kernels_dot_multi", "k_dot_multi", 24, 0),          # three limb widths x (16-byte groups, words) x (tile 2, 1) x (register, streaming)
    ("kernels_rotate", "k_permute_add_ntt", 6, None),     # three limb widths x (16-byte groups, words); the LDS is sized at launch
])
def test_compiled_kernels_use_no_scratch_and_spill_no_vector_register(tmp_path, stem, kernel, instances, lds):
    """the compiler's own resource report for every instance of the two new kernels (hipcc cross-compiles for gfx950 without a GPU):
    no scratch memory, no spilled register -- the register form of k_dot_multi holds the tile's 8 terms of `a` in vector registers"""
    kernels = _resource_report(tmp_path, stem)
    mine = {k: v for k, v in kernels.items() if kernel in k}
    assert len(mine) == instances, sorted(kernels)
    for name, v in sorted(mine.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, name
        if lds is not None:
            assert int(v["LDS Size [bytes/block]"]) == lds, name


# ---- the header layer ----
TOYS = [os.path.join(SRC, "toy_rotate.c"), os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"), os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_rotate: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated
    into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "rotate_main.cpp")
    exe = os.path.join(out_dir, "rotate_test")
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
    for toy in TOYS:
        objs.append(os.path.join(out_dir, os.path.basename(toy)[:-2] + ".o"))
        subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-c", toy, "-o", objs[-1]])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-DNFL_HIP_NO_GMP", "-o", exe, main] + objs +
                          ["-L" + out_dir, "-lnflhip", "-Wl,-rpath," + out_dir])
    return exe


@pytest.fixture(scope="module")
def mock_exe(tmp_path_factory):
    return build_cpp(str(tmp_path_factory.mktemp("cpp_rotate")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other and with the definition written by hand through
    the existing header calls"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # the gathered keys read with the wrong stride
    ("kp[m] = static_cast<char *>(kbuf) + m * kpolys * pb;", "kp[m] = static_cast<char *>(kbuf) + m * dnum * pb;"),
    # c0 dropped by the batch call
    ("c0 ? c0->d_ : nullptr, c1.d_, kp, ks, count, c1.n_,", "nullptr, c1.d_, kp, ks, count, c1.n_,"),
    # ks and keys paired off by one
    ("kp[m] = keys[m]->cdata();", "kp[m] = keys[(m + 1) % count]->cdata();"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad):
    """mutants of the header must fail: the CPU stand-in keeps what the layer's correctness depends on"""
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hit = 0
    for hdr in (inc / "nfl_hip" / "batch.hpp", inc / "nfl_hip" / "poly_p.hpp"):
        text = hdr.read_text()
        hit += text.count(good)
        hdr.write_text(text.replace(good, bad))
    assert hit == 1
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                           os.path.join(SRC, "rotate_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                          ["-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
