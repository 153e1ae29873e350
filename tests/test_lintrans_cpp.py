"""CPU: the header layer of the slot linear transforms (include/nfl_hip: nfl::linear_transform_ntt on poly and poly_p,
device_batch::assign_linear_transform), through the program of tests/cpp_lintrans against the CPU stand-in of tests/cpp/mock with toy
versions of the new entries, and mutants of the header that the program must notice."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_lintrans")
TOYS = [os.path.join(SRC, "toy_lintrans.c"), os.path.join(ROOT, "tests", "cpp_rotate", "toy_rotate.c"),
        os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"), os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("linear_transform_ntt", "linear_transform_into", "assign_linear_transform"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_lintrans: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated
    into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "lintrans_main.cpp")
    exe = os.path.join(out_dir, "lintrans_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_lintrans")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other and with the sums written by hand"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # the gathered diagonals read from the key's slot
    ("wp[m] = static_cast<char *>(kbuf) + (m * tpolys + kpolys) * pb;", "wp[m] = static_cast<char *>(kbuf) + (m * tpolys) * pb;"),
    # c0 dropped by the batch call
    ("c0 ? c0->d_ : nullptr, c1.d_, kp, wp, ks, count, c1.n_,", "nullptr, c1.d_, kp, wp, ks, count, c1.n_,"),
    # diagonals and terms paired off by one
    ("wp[m] = weight_batches[m]->data();", "wp[m] = weight_batches[(m + 1) % count]->data();"),
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
                           os.path.join(SRC, "lintrans_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                          ["-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
