"""The header layer of the RNS base conversion and mod-down (include/nfl_hip/poly_p.hpp, batch.hpp): nfl::base_convert and
nfl::mod_down on poly and poly_p, device_batch / sharded_batch::assign_base_convert and assign_mod_down, through the C++ program of
tests/cpp_baseconv (two translation units).  Without a GPU the program compiles, links and fails loudly; on the GPU it runs under
both queue executors and with deferred execution off.  sharded_batch over SEVERAL shards (tests/cpp_baseconv/sharded_main.cpp): on
the CPU against tests/cpp/mock with eight virtual devices and the toy entries of toy_baseconv.c, on the GPU against the real
library with several shards on device 0 -- every result equal to the same polynomials in one device_batch."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_baseconv")


def build_cpp(out_dir, eager=False):
    """the C++ program of tests/cpp_baseconv, two translation units, with the g++ line of tests/cpp/Makefile"""
    exe = os.path.join(out_dir, "baseconv_test" + ("_eager" if eager else ""))
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-DNFL_HIP_NO_GMP"]
    if eager:
        cmd.append("-DNFL_HIP_EAGER")
    cmd += ["-o", exe, os.path.join(SRC, "baseconv_main.cpp"), os.path.join(SRC, "baseconv_tu2.cpp"),
            "-L" + os.path.join(ROOT, "nfllib_amd"), "-lnflhip", "-Wl,-rpath," + os.path.join(ROOT, "nfllib_amd"),
            "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu(), reason="CPU-only behaviour")
def test_cpp_program_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build_cpp(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout[-2000:]


@pytest.fixture(scope="module")
def cpp_programs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_baseconv"))
    return build_cpp(out), build_cpp(out, eager=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["thread0", "thread1", "eager_runtime", "eager_build"])
def test_cpp_surface_on_the_gpu(mode, cpp_programs):
    """poly, poly_p (deferred operations pending on both ring types, before and after; a copy-on-write sharer across the in-place
    conversion), device_batch, a one-device sharded_batch -- under both queue executors and with deferred execution off"""
    exe = cpp_programs[1] if mode == "eager_build" else cpp_programs[0]
    env = dict(os.environ)
    env["NFL_HIP_QUEUE_THREAD"] = "0" if mode == "thread0" else "1"
    args = [exe] + (["eager"] if mode == "eager_runtime" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- sharded_batch over several shards ----
def _sharded_sources():
    return os.path.join(SRC, "sharded_main.cpp"), os.path.join(SRC, "toy_baseconv.c")


@pytest.fixture(scope="module")
def sharded_mock_exe(tmp_path_factory):
    """the program against the CPU stand-in of tests/cpp/mock (generated into a directory of this test), with the toy base
    conversion entries linked into the program itself, where they take precedence over the stand-in's failing ones"""
    out = str(tmp_path_factory.mktemp("sharded_baseconv"))
    inc = os.path.join(ROOT, "include")
    c = os.path.join(out, "mock_backend.c")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "cpp", "mock", "make_mock_backend.py"), c], stdout=subprocess.DEVNULL)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + inc, "-o", os.path.join(out, "libnflhip.so"), c, "-lpthread"])
    main, toy = _sharded_sources()
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-c", toy, "-o", os.path.join(out, "toy_baseconv.o")])
    exe = os.path.join(out, "sharded_baseconv")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-DNFL_HIP_NO_GMP", "-o", exe, main,
                           os.path.join(out, "toy_baseconv.o"), "-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    return exe


@pytest.mark.parametrize("devs,batch,ndev", [
    ("0,1,2,3,4,5,6,7", 37, 8),      # 8 virtual GPUs, a batch that does not divide
    ("0,1,2,3,4,5,6,7", 3, 8),       # more devices than polynomials: empty shards
    ("5,0,3", 10, 8),                # any subset, any order
    ("0,0,0", 5, 1),                 # several shards on one device
    ("0", 5, 1),                     # the degenerate split
])
def test_sharded_entries_equal_one_device_batch_on_virtual_devices(sharded_mock_exe, devs, batch, ndev):
    env = dict(os.environ, NFLHIP_MOCK_DEVICES=str(ndev))
    r = subprocess.run([sharded_mock_exe, devs, str(batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("good,bad", [
    # a fan-out that hands shard r the neighbour's source
    ("shards_[r].assign_mod_down(src.shard(r), floor);", "shards_[r].assign_mod_down(src.shard((r + 1) % shards()), floor);"),
    ("shards_[r].assign_base_convert(src.shards_[r], s0, ks, d0, kd, centered);",
     "shards_[r].assign_base_convert(src.shards_[(r + 1) % shards()], s0, ks, d0, kd, centered);"),
])
def test_the_virtual_devices_notice_a_broken_fan_out(tmp_path, sharded_mock_exe, good, bad):
    """mutants of the header must fail: the CPU stand-in keeps what the split's correctness depends on"""
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    hdr = inc / "nfl_hip" / "batch.hpp"
    text = hdr.read_text()
    assert good in text
    hdr.write_text(text.replace(good, bad))
    out = os.path.dirname(sharded_mock_exe)
    exe = str(tmp_path / "sharded_mutant")
    main, _ = _sharded_sources()
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + str(inc), "-DNFL_HIP_NO_GMP", "-o", exe, main,
                           os.path.join(out, "toy_baseconv.o"), "-L" + out, "-lnflhip", "-Wl,-rpath," + out])
    env = dict(os.environ, NFLHIP_MOCK_DEVICES="8")
    r = subprocess.run([exe, "0,1,2,3,4,5,6,7", "37"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, r.stdout[-2000:]


@pytest.fixture(scope="module")
def sharded_gpu_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sharded_baseconv_gpu"))
    exe = os.path.join(out, "sharded_baseconv")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-DNFL_HIP_NO_GMP", "-o", exe,
           _sharded_sources()[0], "-L" + os.path.join(ROOT, "nfllib_amd"), "-lnflhip", "-Wl,-rpath," + os.path.join(ROOT, "nfllib_amd"),
           "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("devs,batch", [("0,0,0", 5), ("0,0,0,0", 3), ("0", 4)])
def test_sharded_entries_on_the_gpu(sharded_gpu_exe, devs, batch):
    """the real library: several shards on device 0, a batch that does not divide, empty shards"""
    r = subprocess.run([sharded_gpu_exe, devs, str(batch)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
