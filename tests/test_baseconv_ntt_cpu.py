"""CPU: the NTT-form base conversion and mod-down (include/nflhip.h "RNS base conversion and mod-down, NTT form").
  * the C ABI, the Python binding and the Engine carry the new names; a NULL context is refused without a device;
  * the compiler's resource report for every kernel of kernels_baseconv_ntt.hip;
  * the statement the GPU tests compare against, on numpy with the oracle: oracle.intt of the NTT-form `want` is the coefficient-form
    restatement of tests/baseconv_util.py on the planted inputs;
  * the header layer (include/nfl_hip), through the program of tests/cpp_baseconv_ntt against the CPU stand-in of tests/cpp/mock with
    eight virtual devices and toy versions of the new entries."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import baseconv_util as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_baseconv_ntt")
ENTRIES = ("nflhip_baseconv_ntt_dev", "nflhip_baseconv_ntt", "nflhip_moddown_ntt_dev", "nflhip_moddown_ntt")
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}


def test_header_declares_and_binding_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "nflhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "#define NFLHIP_ABI_VERSION 6" in code
    flags = {k: int(re.search(r"#define\s+NFLHIP_BASECONV_NTT_%s\s+(0x[0-9a-fA-F]+)\b" % k, code).group(1), 16) for k in ("COMPOSED", "FUSED")}
    assert flags == {"COMPOSED": 0x200, "FUSED": 0x400}
    from nfllib_amd import Engine, _lib
    assert set(ENTRIES) <= {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert hasattr(_lib.lib, name)
    assert (_lib.BASECONV_NTT_COMPOSED, _lib.BASECONV_NTT_FUSED) == (flags["COMPOSED"], flags["FUSED"])
    assert not (flags["COMPOSED"] | flags["FUSED"]) & (_lib.BASECONV_CENTERED | _lib.MODDOWN_FLOOR)
    for meth in ("baseconv_ntt", "mod_up_ntt", "mod_down_ntt", "h_baseconv_ntt", "h_mod_down_ntt"):
        assert callable(getattr(Engine, meth))
    hdr = open(os.path.join(ROOT, "include", "nfl_hip", "poly_p.hpp")).read() + open(os.path.join(ROOT, "include", "nfl_hip", "batch.hpp")).read()
    for name in ("base_convert_ntt", "mod_down_ntt"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert hdr.count("bool ntt_form = false") >= 4


def test_library_exports_the_entries_and_validates_without_a_device():
    lib = os.path.join(ROOT, "nfllib_amd", "libnflhip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    from nfllib_amd import _lib
    L = _lib.lib
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    for flags in (0, 0x100, 0x200, 0x400, 0x600):
        assert L.nflhip_baseconv_ntt_dev(None, p, p, 1, 0, 1, 0, 1, flags, None) == _lib.ERR_INVALID == 1   # NULL context: no device needed
        assert L.nflhip_baseconv_ntt(None, p, p, 1, 0, 1, 0, 1, flags) == _lib.ERR_INVALID
        assert L.nflhip_moddown_ntt_dev(None, p, p + 64, 1, 1, flags, None) == _lib.ERR_INVALID
        assert L.nflhip_moddown_ntt(None, p, p + 64, 1, 1, flags) == _lib.ERR_INVALID


def test_compiled_kernels_use_no_scratch_and_spill_no_vector_register(tmp_path):
    """the compiler's own resource report for every kernel of kernels_baseconv_ntt.hip (hipcc cross-compiles for gfx950 without a
    GPU): the one-launch kernel runs 1024 threads per workgroup, which leaves it 128 vector registers; the streaming kernel uses no
    LDS"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build's compiler"
    src = os.path.join(ROOT, "nfllib_amd", "csrc", "kernels_baseconv_ntt.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "kernels_baseconv_ntt.o")], capture_output=True, text=True, timeout=1200)
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
    fused = {k: v for k, v in kernels.items() if "k_bconv_ntt_fused" in k}
    stream = {k: v for k, v in kernels.items() if "k_moddown_ntt_combine" in k}
    assert len(fused) == 3 and len(stream) == 6       # three limb widths; x (16-byte groups, words)
    assert not [k for k in kernels if "k_baseconv" in k]   # (tests/test_baseconv_cpu.py counts those of kernels_baseconv.hip)
    for name, v in sorted(kernels.items()):
        print(name, "VGPRs", v["VGPRs"], "SGPRs Spill", v["SGPRs Spill"], "LDS", v["LDS Size [bytes/block]"], "Occupancy", v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0, name
        assert int(v["VGPRs Spill"]) == 0, name
    for name, v in fused.items():
        assert int(v["VGPRs"]) <= 128, name
    for name, v in stream.items():
        assert int(v["LDS Size [bytes/block]"]) == 0, name


CASES = [(64, 64, 4, [((0, 2), (2, 2)), ((1, 2), (0, 4)), ((3, 1), (0, 4)), ((0, 4), (0, 4))], [1, 2, 3]),
         (32, 128, 3, [((0, 2), (2, 1)), ((1, 1), (0, 3))], [2]),
         (16, 4, 2, [((0, 1), (1, 1)), ((1, 1), (0, 2))], [1]),
         (64, 64, 96, [((70, 17), (60, 36))], [17])]


@pytest.mark.parametrize("lb,n,nm,pairs,ks", CASES)
def test_the_ntt_form_statement_restated_through_the_oracle(lb, n, nm, pairs, ks, oracle_factory):
    """want = oracle.ntt(baseconv_rns(a)) is what the GPU tests compare against, for the input oracle.ntt(a): the oracle's inverse
    transform takes both back, so the statement is `intt(out) == baseconv(intt(in))` row for row, and the rows outside D of `want`
    are the input's.  The same for the mod-down with the oracle over the first nm - k moduli."""
    from nfllib_amd.params import params
    P = [int(v) for v in params(lb).P[:nm]]
    orc = oracle_factory(lb, n, nm)
    for src, dst in pairs:
        a = B.random_batch(P, n, 3, _NP[lb], 3)
        B.plant(a, P, src, B.edge_values(P, src)[-n:], b=0)
        B.plant(a, P, src, B.band_values(P, src, lb)[:n], b=1)
        A = orc.ntt(a)
        assert np.array_equal(orc.intt(A), a)
        rows = list(range(dst[0], dst[0] + dst[1]))
        other = [j for j in range(nm) if j not in rows]
        for centered in (False, True):
            coeff = B.baseconv_rns(a, P, src, dst, centered=centered)
            want = orc.ntt(coeff)
            assert np.array_equal(orc.intt(want), coeff)
            assert np.array_equal(want[:, other], A[:, other])                   # rows outside D: the input's
            both = [j for j in rows if src[0] <= j < src[0] + src[1]]
            assert np.array_equal(want[:, both], A[:, both])                     # rows of D in S: the input's (canonical words)
    for k in ks:
        kept = oracle_factory(lb, n, nm - k)
        a = B.random_batch(P, n, 3, _NP[lb], 6)
        B.plant(a, P, (nm - k, k), B.band_values(P, (nm - k, k), lb)[:n], b=1)
        for floor in (False, True):
            coeff = B.moddown_rns(a, P, k, floor=floor)
            want = kept.ntt(coeff)
            assert want.shape == (3, nm - k, n) and np.array_equal(kept.intt(want), coeff)
            # the row formula in NTT form: Y_j = (x_j - NTT_j(conv_j)) P^-1, the transform being linear in every row
            conv = kept.ntt(np.ascontiguousarray(B.baseconv_rns(a, P, (nm - k, k), (0, nm - k), centered=not floor)[:, :nm - k]))
            A = orc.ntt(a)
            Pk = B.prod(P[nm - k:])
            for j in range(nm - k):
                y = ((A[:, j].astype(object) - conv[:, j].astype(object)) * pow(Pk % P[j], -1, P[j])) % P[j]
                assert np.array_equal(y.astype(_NP[lb]), want[:, j]), (k, floor, j)


# ---- the header layer ----
def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_baseconv_ntt: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock
    generated into out_dir, with the toy entries of both forms linked into the program itself, where they take precedence over
    the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "baseconv_ntt_main.cpp")
    exe = os.path.join(out_dir, "baseconv_ntt_test")
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
    for toy in (os.path.join(SRC, "toy_baseconv_ntt.c"), os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")):
        objs.append(os.path.join(out_dir, os.path.basename(toy)[:-2] + ".o"))
        subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-c", toy, "-o", objs[-1]])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-DNFL_HIP_NO_GMP", "-o", exe, main] + objs +
                          ["-L" + out_dir, "-lnflhip", "-Wl,-rpath," + out_dir])
    return exe


@pytest.fixture(scope="module")
def mock_exe(tmp_path_factory):
    return build_cpp(str(tmp_path_factory.mktemp("cpp_baseconv_ntt")))


@pytest.mark.parametrize("devs,batch,ndev", [
    ("0,1,2,3,4,5,6,7", 37, 8),      # 8 virtual GPUs, a batch that does not divide
    ("0,1,2,3,4,5,6,7", 3, 8),       # more devices than polynomials: empty shards
    ("5,0,3", 10, 8),                # any subset, any order
    ("0,0,0", 5, 1),                 # several shards on one device
    ("0", 5, 1),                     # the degenerate split
])
def test_header_layer_on_virtual_devices(mock_exe, devs, batch, ndev):
    """poly, poly_p with copy-on-write sharers, device_batch, and a sharded_batch equal to one device_batch; the default
    ntt_form = false reaches the coefficient-form entries"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES=str(ndev))
    r = subprocess.run([mock_exe, devs, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # a fan-out that hands shard r the neighbour's source
    ("shards_[r].assign_mod_down(src.shard(r), floor, true);", "shards_[r].assign_mod_down(src.shard((r + 1) % shards()), floor, true);"),
    ("shards_[r].assign_base_convert(src.shards_[r], s0, ks, d0, kd, centered, true);",
     "shards_[r].assign_base_convert(src.shards_[(r + 1) % shards()], s0, ks, d0, kd, centered, true);"),
    # an NTT-form call that reaches the coefficient-form entry
    ("nflhip_moddown_ntt_dev(src.ctx(), d_, src.data(), n_,", "nflhip_moddown_dev(src.ctx(), d_, src.data(), n_,"),
    ("poly_p<T, D, M>::base_convert_into(p, s0, ks, d0, kd, centered, true);", "poly_p<T, D, M>::base_convert_into(p, s0, ks, d0, kd, centered, false);"),
])
def test_the_virtual_devices_notice_a_broken_header(tmp_path, mock_exe, good, bad):
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
                           os.path.join(SRC, "baseconv_ntt_main.cpp"), os.path.join(out, "toy_baseconv_ntt.o"), os.path.join(out, "toy_baseconv.o"),
                           "-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="8")
    r = subprocess.run([exe, "0,1,2,3,4,5,6,7", "37"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
