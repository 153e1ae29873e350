"""CPU: the header layer of BSGS slot linear transforms (include/nfl_hip: nfl::bsgs_linear_transform_ntt<K> on poly and poly_p,
device_batch::assign_bsgs_linear_transform<K>), through the program of tests/cpp_bsgs against the CPU stand-in of tests/cpp/mock with a
toy version of the new entry, and mutants of the header that the program must notice: the baby and the giant keys swapped, the weights
indexed i * n2 + j, and the level not passed (the top level in its place), each in the resident, the batch and the staged call."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_bsgs")
TOYS = [os.path.join(SRC, "toy_bsgs.c"), os.path.join(ROOT, "tests", "cpp_level_rotate", "toy_level_rotate.c"),
        os.path.join(ROOT, "tests", "cpp_lintrans", "toy_lintrans.c"), os.path.join(ROOT, "tests", "cpp_rotate", "toy_rotate.c"),
        os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"), os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("bsgs_linear_transform_ntt", "bsgs_into", "assign_bsgs_linear_transform"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_bsgs: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated into
    out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "bsgs_main.cpp")
    exe = os.path.join(out_dir, "bsgs_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_bsgs")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other and with the C entry on raw pointers"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # the baby and the giant keys swapped: resident, batch, staged
    ("p0, p1, kp, bks, n1, kp + n1, gks, n2, wp, 1, K, alpha, LO, flags,", "p0, p1, kp + n1, bks, n1, kp, gks, n2, wp, 1, K, alpha, LO, flags,"),
    ("c1.d_, bp, bks, n1, gp, gks, n2, wp, c1.n_, K, alpha,", "c1.d_, gp, bks, n1, bp, gks, n2, wp, c1.n_, K, alpha,"),
    ("c1.cdata(), bp, bks, n1, gp, gks, n2, wp, 1, K, alpha, Lv,", "c1.cdata(), gp, bks, n1, bp, gks, n2, wp, 1, K, alpha, Lv,"),
    # the weights indexed i * n2 + j
    ("for (size_t q = 0; q < nw; ++q) held.push_back(weights[q] ? weights[q]->_p : ptr_type());",
     "for (size_t q = 0; q < nw; ++q) held.push_back(weights[(q % n1) * n2 + q / n1] ? weights[(q % n1) * n2 + q / n1]->_p : ptr_type());"),
    ("      const device_batch<Q> *wb = weight_batches[q];", "      const device_batch<Q> *wb = weight_batches[(q % n1) * n2 + q / n1];"),
    ("for (size_t q = 0; q < n1 * n2; ++q) wp[q] = weights[q] ? weights[q]->cdata() : nullptr;",
     "for (size_t q = 0; q < n1 * n2; ++q) wp[q] = weights[(q % n1) * n2 + q / n1] ? weights[(q % n1) * n2 + q / n1]->cdata() : nullptr;"),
    # the level not passed: the top level in its place
    ("kp + n1, gks, n2, wp, 1, K, alpha, LO, flags,", "kp + n1, gks, n2, wp, 1, K, alpha, NbModuli - K, flags,"),
    ("wp, c1.n_, K, alpha,\n                                                 P::nmoduli, flags,", "wp, c1.n_, K, alpha,\n                                                 Q::nmoduli - K, flags,"),
    ("bp, bks, n1, gp, gks, n2, wp, 1, K, alpha, Lv,\n", "bp, bks, n1, gp, gks, n2, wp, 1, K, alpha, M - K,\n"),
])
def test_the_stand_in_notices_a_broken_header(tmp_path, mock_exe, good, bad):
    """mutants of the header must fail the program's checks: the CPU stand-in keeps what the layer's correctness depends on"""
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
                           os.path.join(SRC, "bsgs_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                          ["-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
