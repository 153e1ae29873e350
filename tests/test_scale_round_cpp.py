"""The header layer of BFV multiplication (include/nfl_hip/poly_p.hpp: nfl::scale_round, nfl::scale_round_ntt, nfl::bfv_tensor_ntt<KB>
and nfl::bfv_square_ntt<KB> on poly and poly_p), through the program of tests/cpp_scale_round: on the CPU against the stand-in of
tests/cpp/mock with toy versions of the new entries, with mutants of the header that the program must notice; on the GPU the same
program against the library."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_scale_round")
TOYS = [os.path.join(SRC, "toy_scale_round.c"), os.path.join(ROOT, "tests", "cpp_mulrelin", "toy_mulrelin.c"),
        os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"), os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = open(os.path.join(ROOT, "include", "nfl_hip", "poly_p.hpp")).read()
    for name in ("scale_round", "scale_round_ntt", "scale_round_into", "bfv_tensor_ntt", "bfv_square_ntt", "bfv_tensor_into"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_scale_round: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock
    generated into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's
    failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "scale_round_main.cpp")
    exe = os.path.join(out_dir, "scale_round_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_scale_round")))


def test_header_layer_on_the_stand_in(mock_exe):
    """poly and poly_p with copy-on-write sharers agree with each other, with the raw entries and with the four steps written by hand"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # ks taken from the wrong type: the input's moduli less the output's
    ('nflhip_scale_round_dev(ctx_t::get(), d, s, 1, KS, t,', 'nflhip_scale_round_dev(ctx_t::get(), d, s, 1, NbModuli - KS, t,'),
    # b0 and b1 swapped by the resident path
    ("o0, o1, o2, p_a0, p_a1, p_b0, p_b1, 1, L, t,", "o0, o1, o2, p_a0, p_a1, p_b1, p_b0, 1, L, t,"),
    # t not passed through: the resident NTT-form scale-round, the staged tensor product
    ('nflhip_scale_round_ntt_dev(ctx_t::get(), d, s, 1, KS, t,', 'nflhip_scale_round_ntt_dev(ctx_t::get(), d, s, 1, KS, 1,'),
    ("b1 ? b1->cdata() : nullptr, 1, L, t, floor", "b1 ? b1->cdata() : nullptr, 1, L, 1, floor"),
    # the floor mode dropped by the resident tensor product
    ("p_b0, p_b1, 1, L, t, floor ? NFLHIP_SCALE_ROUND_FLOOR : 0,", "p_b0, p_b1, 1, L, t, 0,"),
    # the extended ring taken as the ciphertexts' own
    ("poly_p<T, D, L + KB>::template bfv_tensor_into<L>(d0, d1, d2, a0, a1, &b0, &b1, t, floor);", "poly_p<T, D, L + KB - 1>::template bfv_tensor_into<L>(d0, d1, d2, a0, a1, &b0, &b1, t, floor);"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad):
    """mutants of the header must fail -- to build, or the program's checks: the CPU stand-in keeps what the layer's correctness
    depends on"""
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hdr = inc / "nfl_hip" / "poly_p.hpp"
    text = hdr.read_text()
    assert text.count(good) == 1, good
    hdr.write_text(text.replace(good, bad))
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    b = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                        os.path.join(SRC, "scale_round_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                       ["-L" + out, "-lnflhip", "-Wl,-rpath," + out], capture_output=True, text=True)
    if b.returncode != 0:
        assert "bfv_tensor" in b.stderr, b.stderr[-2000:]
        return
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
def test_cpp_surface_on_the_gpu(tmp_path):
    """the same program against the real library: the header layer's calls equal the raw entries and the four steps of the definition
    through the existing header calls"""
    exe = build_cpp(str(tmp_path), gpu=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
