"""CPU: the header layer of the calls below the top level (include/nfl_hip: nfl::key_switch_level_ntt<K>, nfl::mul_relin_level_ntt<K>,
nfl::square_relin_level_ntt<K> and nfl::mul_relin_rescale_level_ntt<K> on poly and poly_p, device_batch::assign_key_switch_level<K> /
assign_mul_relin_level<K>), through the program of tests/cpp_level against the CPU stand-in of tests/cpp/mock with toy versions of the
new entries, and mutants of the header that the program must notice.  Of the four mutants the issue names, three are here: dnum_L
key polynomials gathered where dnum_l are needed (the program's dead key polynomials are moved from, and the layer refuses an empty
polynomial it touches), K and the level swapped (in the resident, the batch and the staged call) and the rescaled outputs' type.
The fourth, phys(r) without the hole, has no place in this layer: it hands WHOLE key polynomials of the parent ring to the entry,
which finds phys(r) itself (tests/test_gpu_level.py checks the hole there, against the restatement and with the dead rows
poisoned).  In its stead: the live key's stride in the gathered buffer, and the batch call that forgets the rescale flag."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_level")
TOYS = [os.path.join(SRC, "toy_level.c"), os.path.join(ROOT, "tests", "cpp_mulrelin", "toy_mulrelin.c"),
        os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"), os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("key_switch_level_ntt", "mul_relin_level_ntt", "square_relin_level_ntt", "mul_relin_rescale_level_ntt", "key_switch_level_into",
                 "mul_relin_level_into", "assign_key_switch_level", "assign_mul_relin_level"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_level: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated into
    out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "level_main.cpp")
    exe = os.path.join(out_dir, "level_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_level")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other, with the C entries on raw pointers and, at the
    top level, with the existing calls"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad,hits", [
    # K and the level swapped: by the resident key switch, by the batch key switch, by the staged multiplication
    ("o0, o1, s, kgat, 1, K, alpha, LO, flags,", "o0, o1, s, kgat, 1, LO, alpha, K, flags,", 1),
    ("key.data(), src.n_, K, alpha, P::nmoduli, flags,", "key.data(), src.n_, P::nmoduli, alpha, K, flags,", 1),
    ("key->cdata(), 1, K, alpha, Lv, flags);\n  if (rc == 0) {\n    std::memcpy(static_cast<void *>(out0.data())",
     "key->cdata(), 1, Lv, alpha, K, flags);\n  if (rc == 0) {\n    std::memcpy(static_cast<void *>(out0.data())", 1),
    # dnum_L key polynomials gathered where dnum_l are needed (both resident calls): the dead ones are moved from in the program
    ("const size_t live = 2 * ((LO + alpha - 1) / alpha), pb", "const size_t live = 2 * ((NbModuli - K + alpha - 1) / alpha), pb", 2),
    # the live key polynomials gathered with the wrong stride (both resident calls)
    ("static_cast<char *>(kgat) + t * pb, kept[t]->dev_ro()", "static_cast<char *>(kgat) + t * (pb / 2), kept[t]->dev_ro()", 2),
    # the rescaled outputs typed as the inputs' ring: the program's call no longer matches, the build fails
    ("void mul_relin_rescale_level_ntt(poly_p<T, D, Lv - 1> &out0, poly_p<T, D, Lv - 1> &out1,",
     "void mul_relin_rescale_level_ntt(poly_p<T, D, Lv> &out0, poly_p<T, D, Lv> &out1,", 1),
    # the batch call that forgets the rescale
    ("if (O::nmoduli != P::nmoduli) flags |= NFLHIP_MULRELIN_RESCALE;", "", 1),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad, hits):
    """mutants of the header must fail -- to build, or the program's checks: the CPU stand-in keeps what the layer's correctness
    depends on"""
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hit = 0
    for hdr in (inc / "nfl_hip" / "batch.hpp", inc / "nfl_hip" / "poly_p.hpp"):
        text = hdr.read_text()
        hit += text.count(good)
        hdr.write_text(text.replace(good, bad))
    assert hit == hits
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    b = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                        os.path.join(SRC, "level_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                       ["-L" + out, "-lnflhip", "-Wl,-rpath," + out], capture_output=True, text=True)
    if b.returncode != 0:
        assert "mul_relin_rescale_level_ntt" in b.stderr, b.stderr[-2000:]
        return
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
