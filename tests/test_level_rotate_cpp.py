"""CPU: the header layer of hoisted rotations and slot linear transforms below the top level (include/nfl_hip:
nfl::rotate_hoisted_level_ntt<K> and nfl::linear_transform_level_ntt<K> on poly and poly_p, device_batch::assign_rotations_level<K> /
assign_linear_transform_level<K>), through the program of tests/cpp_level_rotate against the CPU stand-in of tests/cpp/mock with toy
versions of the new entries, and mutants of the header that the program must notice: dnum_L key polynomials gathered where dnum_l are
needed (the program's dead key polynomials are moved from, and the layer refuses an empty polynomial it touches), K and the level
swapped (in the resident, the batch and the staged calls), a diagonal handed over on l + K rows instead of nm (the toy entry reads the
special rows of a diagonal where the parent's layout has them), and the key stride per rotation in the gathered buffer."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_level_rotate")
TOYS = [os.path.join(SRC, "toy_level_rotate.c"), os.path.join(ROOT, "tests", "cpp_lintrans", "toy_lintrans.c"),
        os.path.join(ROOT, "tests", "cpp_rotate", "toy_rotate.c"), os.path.join(ROOT, "tests", "cpp_keyswitch", "toy_keyswitch.c"),
        os.path.join(ROOT, "tests", "cpp_baseconv_ntt", "toy_baseconv_ntt.c"), os.path.join(ROOT, "tests", "cpp_baseconv", "toy_baseconv.c")]


def test_the_headers_carry_the_calls():
    hdr = "".join(open(os.path.join(ROOT, "include", "nfl_hip", f)).read() for f in ("poly.hpp", "poly_p.hpp", "batch.hpp"))
    for name in ("rotate_hoisted_level_ntt", "linear_transform_level_ntt", "rotate_level_into", "linear_transform_level_into", "assign_rotations_level",
                 "assign_linear_transform_level"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def build_cpp(out_dir, gpu=False):
    """the program of tests/cpp_level_rotate: against the real library (gpu=True), or against the CPU stand-in of tests/cpp/mock generated
    into out_dir, with the toy entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    inc = os.path.join(ROOT, "include")
    main = os.path.join(SRC, "level_rotate_main.cpp")
    exe = os.path.join(out_dir, "level_rotate_test")
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
    return build_cpp(str(tmp_path_factory.mktemp("cpp_level_rotate")))


@pytest.mark.parametrize("batch", [1, 5])
def test_header_layer_on_the_stand_in(mock_exe, batch):
    """poly, poly_p with copy-on-write sharers and device_batch agree with each other, with the C entries on raw pointers and, at the
    top level, with the existing calls"""
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="1")
    r = subprocess.run([mock_exe, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # dnum_L key polynomials gathered where dnum_l are needed (the two resident calls): the dead ones are moved from in the program
    ("const size_t rlive = 2 * ((LO + alpha - 1) / alpha), pb", "const size_t rlive = 2 * ((NbModuli - K + alpha - 1) / alpha), pb"),
    ("const size_t tlive = 2 * ((LO + alpha - 1) / alpha), pb", "const size_t tlive = 2 * ((NbModuli - K + alpha - 1) / alpha), pb"),
    # K and the level swapped: the two resident calls, the two batch calls, the two staged calls
    ("p0, p1, kp, ks, count, 1, K, alpha, LO, flags,", "p0, p1, kp, ks, count, 1, LO, alpha, K, flags,"),
    ("p0, p1, kp, wp, ks, count, 1, K, alpha, LO, flags,", "p0, p1, kp, wp, ks, count, 1, LO, alpha, K, flags,"),
    ("kp, ks, count, c1.n_, K, alpha,\n                                                                  P::nmoduli, flags,",
     "kp, ks, count, c1.n_, P::nmoduli, alpha,\n                                                                  K, flags,"),
    ("kp, wp, ks, count, c1.n_, K, alpha,\n                                                          P::nmoduli, flags,",
     "kp, wp, ks, count, c1.n_, P::nmoduli, alpha,\n                                                          K, flags,"),
    ("c1.cdata(), kp, ks, count, 1, K, alpha, Lv, flags);", "c1.cdata(), kp, ks, count, 1, Lv, alpha, K, flags);"),
    ("c1.cdata(), kp, wp, ks, count, 1, K, alpha, Lv,\n", "c1.cdata(), kp, wp, ks, count, 1, Lv, alpha, K,\n"),
    # a diagonal handed over on l + K rows instead of nm
    ("const size_t wbytes = pb;", "const size_t wbytes = sizeof(T) * Degree * (LO + K);"),
    # the key stride per rotation in the gathered buffer
    ("kp[m] = static_cast<char *>(kgat) + m * rlive * pb;", "kp[m] = static_cast<char *>(kgat) + m * (rlive / 2) * pb;"),
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
                           os.path.join(SRC, "level_rotate_main.cpp")] + [os.path.join(out, os.path.basename(t)[:-2] + ".o") for t in TOYS] +
                          ["-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, env=dict(os.environ, NFLHIP_MOCK_DEVICES="1"), timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]
