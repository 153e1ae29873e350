"""CPU: the header layer of the ciphertext multiplication (include/nfl_hip: nfl::tensor_ntt, nfl::mul_relin_ntt, nfl::square_relin_ntt and
nfl::mul_relin_rescale_ntt on poly and poly_p, device_batch::assign_mul_relin), through the program of tests/cpp_mulrelin against the
CPU stand-in of tests/cpp/mock with toy versions of the new entries, and mutants of the header that the program must notice."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_mulrelin")
TOYS = [os.path.join(SRC, "toy_mulrelin.c"), os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"), os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("tensor_ntt", "tensor_into", "mul_relin_ntt", "square_relin_ntt", "mul_relin_rescale_ntt", "mul_relin_into", "assign_mul_relin"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_mulrelin: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated
    into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "mulrelin_main.cpp")
    exe = os.path.join(out_dir, "mulrelin_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_mulrelin")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other and with the sequence written by hand"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # b0 and b1 swapped, by the resident path and by the batch call
    ("o0, o1, p_a0, p_a1, p_b0, p_b1, kbuf, 1,", "o0, o1, p_a0, p_a1, p_b1, p_b0, kbuf, 1,"),
    ("a0.d_, a1.d_, b0 ? b0->d_ : nullptr, b1 ? b1->d_ : nullptr,", "a0.d_, a1.d_, b1 ? b1->d_ : nullptr, b0 ? b0->d_ : nullptr,"),
    # the key gathered with the wrong stride
    ("kb + t * pb, held[t]->dev_ro()", "kb + t * (pb / 2), held[t]->dev_ro()"),
    # the rescaled outputs typed as the inputs' ring: the program's call no longer matches, the build fails
    ("void mul_relin_rescale_ntt(poly_p<T, D, L - 1> &out0, poly_p<T, D, L - 1> &out1,", "void mul_relin_rescale_ntt(poly_p<T, D, L> &out0, poly_p<T, D, L> &out1,"),
    # the batch call that forgets the rescale
    ("(O::nmoduli != P::nmoduli ? NFLHIP_MULRELIN_RESCALE : 0);\n    detail::check(key.ctx()", "0;\n    detail::check(key.ctx()"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad):
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
    assert hit == 1
    out = os.path.dirname(mock_exe)
    exe = str(tmp_path / "mutant")
    b = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe,
                        os.path.join(SRC, "mulrelin_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                       ["-L" + out, "-lnflhip", "-Wl,-rpath," + out], capture_output=True, text=True)
    if b.returncode != 0:
        assert "mul_relin_rescale_ntt" in b.stderr, b.stderr[-2000:]
        return
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
