"""The header layer of the sums of ciphertext products (include/nfl_hip/poly_p.hpp: nfl::tensor_dot_ntt, nfl::mul_relin_dot_level_ntt<K>,
nfl::square_relin_dot_level_ntt<K> on poly and poly_p; batch.hpp: device_batch::assign_mul_relin_dot_level<K>), through the program of
tests/cpp_mulrelin_dot: on the CPU against the stand-in of tests/cpp/mock with toy versions of the new entries, with mutants of the
headers that the program must notice; on the GPU the same program against the library."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_mulrelin_dot")
TOYS = [os.path.join(SRC, "toy_mulrelin_dot.c"), os.path.join(ROOT, "tests", "cpp_level", "toy_level.c"),
        os.path.join(ROOT, "tests", "cpp_mulrelin", "toy_mulrelin.c"), os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"), os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = open(os.path.join(ROOT, "include", "nfl_hip", "poly_p.hpp")).read()
    for name in ("tensor_dot_ntt", "tensor_dot_into", "mul_relin_dot_level_ntt", "square_relin_dot_level_ntt", "mul_relin_dot_level_into"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"\bassign_mul_relin_dot_level\s*\(", open(os.path.join(ROOT, "include", "nfl_hip", "batch.hpp")).read())


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_mulrelin_dot: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock
    generated into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's
    failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "mulrelin_dot_main.cpp")
    exe = os.path.join(out_dir, "mulrelin_dot_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_mulrelin_dot")))


def test_header_layer_on_the_stand_in(mock_exe):
    """poly, poly_p and device_batch agree with each other, with the raw entries and with the per-term header calls"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("header,good,bad", [
    # b0 and b1 swapped by the resident path
    ("poly_p.hpp", "b0 ? &op[2] : nullptr, b0 ? &op[3] : nullptr, kgat, 1, terms, K,", "b0 ? &op[3] : nullptr, b0 ? &op[2] : nullptr, kgat, 1, terms, K,"),
    # the number of terms not passed by the staged path
    ("poly_p.hpp", "key->cdata(), 1, terms, 0, K, alpha, Lv, flags);", "key->cdata(), 1, 1, 0, K, alpha, Lv, flags);"),
    # a shared b read with the group stride of a dense one
    ("batch.hpp", "y0 = {b0 ? b0->d_ : nullptr, b_shared ? 0 : terms, 1}", "y0 = {b0 ? b0->d_ : nullptr, terms, 1}"),
    # the level not passed: the key ring's ordinary moduli instead
    ("poly_p.hpp", "kgat, 1, terms, K, alpha, LO, flags,", "kgat, 1, terms, K, alpha, NbModuli - K, flags,"),
    # the rescale flag dropped in the batch call
    ("batch.hpp", "const int rescale = O::nmoduli != P::nmoduli ? NFLHIP_MULRELIN_RESCALE : 0;", "const int rescale = 0;"),
    # the gathered key laid out with the operands' pitch
    ("poly_p.hpp", "kpos + t * pb, kept[t]->dev_ro()", "kpos + t * qb, kept[t]->dev_ro()"),
    # the operands gathered term-minor
    ("poly_p.hpp", "op[k].ptr = gat + (k < nin ? k : 0) * terms * qb", "op[k].ptr = gat + (k < nin ? k : 0) * qb"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, header, good, bad):
    """mutants of the headers must fail -- to build, or the program's checks: the CPU stand-in keeps what the layer's correctness
    depends on"""
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hdr = inc / "nfl_hip" / header
    text = hdr.read_text()
    assert text.count(good) == 1, good
    hdr.write_text(text.replace(good, bad))
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    b = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                        os.path.join(SRC, "mulrelin_dot_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                       ["-L" + out, "-lnflhip", "-Wl,-rpath," + out], capture_output=True, text=True)
    if b.returncode != 0:
        assert "mul_relin_dot" in b.stderr, b.stderr[-2000:]
        return
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
def test_cpp_surface_on_the_gpu(tmp_path):
    """the same program against the real library"""
    exe = build_cpp(str(tmp_path), gpu=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
