"""CPU: every per-context table nfllib_amd/csrc/host_tables.cpp computes (what api.hip uploads), through the small dump program
of tests/cpp_tables built with g++ -- no HIP, no device.
  * byte for byte against tests/golden/host_tables_sha256.json: the digests of every table, scalar and shape fact the single
    build_tables function of api.hip produced before the tables moved to host_tables.cpp (recorded once, on the host, from that
    function's body with the HIP allocation and copy calls replaced by malloc / memcpy);
  * independently of that file: psi / mc / mc_inc / psi_lm against tests/asm_emu.py device_tables (the tables the emulated
    assembly kernels run on), the CRT constants and the rescale records against their definitions on Python integers, the three
    validation failures, and the reference-layout tables of nflhip_get_table against the reference's own (tests/golden)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import asm_emu
import golden_util as G
from nfllib_amd.params import params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_tables_sha256.json")
_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}
TABLES = ("psi", "psi_lm", "mc", "mc_inc0", "mc_inc1", "resc", "qhat", "qsh", "qparts", "bparts", "qhat_w", "qsh_w",
          "crt_bfrag", "crt_bproj", "crt_coff", "crt_c2048")
INTS = ("proj_K", "crt_Lw", "crt_nsh", "crt_L", "crt_Lacc", "crt_Q0", "small_delta", "nm_small")
HOST = ("h_Q", "h_lifting", "h_phi")

# key -> (limb_bits, n, indices into params(limb_bits), cyclic).  u64 / 4096: 16, 17, 20, 21, 32 straddle the two matrix-core
# thresholds (32: modulus slot 31 is a modulus), 33 takes the limb-serial lift tables, 94 and 90..93 run past the last modulus
# with delta < 2^32 (#91), 0,1,1 repeats its last modulus (no rescale)
SHAPES = {"u16/128/1": (16, 128, [0], 0), "u16/128/2": (16, 128, [0, 1], 0),
          "u32/8/2": (32, 8, [0, 1], 0), "u32/1024/2": (32, 1024, [0, 1], 0), "u32/4096/1": (32, 4096, [0], 0),
          "u64/1024/2": (64, 1024, [0, 1], 0), "u64/4096/4": (64, 4096, list(range(4)), 0)}
SHAPES.update({"u64/4096/%d" % nm: (64, 4096, list(range(nm)), 0) for nm in (16, 17, 20, 21, 32, 33, 94)})
SHAPES.update({"u64/4096/90-93": (64, 4096, [90, 91, 92, 93], 0), "u64/4096/0,1,1": (64, 4096, [0, 1, 1], 0)})
SHAPES.update({"u%d/1024/1/cyclic%d" % (lb, c): (lb, 1024, [0], c) for lb in (64, 32) for c in (1, 2)})


class Sub:
    """params(limb_bits) cut down to the moduli `idx`, in that order"""

    def __init__(self, lb, idx):
        pr = params(lb)
        self.dtype, self.kmax, self.kmax_log2 = pr.dtype, pr.kmax, pr.kmax_log2
        self.P, self.primitive_roots, self.invkmax = (t[list(idx)] for t in (pr.P, pr.primitive_roots, pr.invkmax))


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("cpp_tables")), "tables_dump")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp_tables", "tables_dump.cpp"),
           os.path.join(ROOT, "nfllib_amd", "csrc", "host_tables.cpp")]     # (no ROCm include path: the file is HIP-free)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def records(out):
    """the dump program's output: {name: bytes}"""
    rec, pos = {}, 0
    while pos < len(out):
        eol = out.index(b"\n", pos)
        name, size = out[pos:eol].split()
        rec[name.decode()] = out[eol + 1:eol + 1 + int(size)]
        pos = eol + 1 + int(size)
    return rec


def run_tables(exe, lb, n, P, roots, invk, cyclic, kmax_log2):
    text = "".join("%d %d %d\n" % (int(p), int(r), int(k)) for p, r, k in zip(P, roots, invk))
    r = subprocess.run([exe, "tables", str(lb), str(n), str(len(P)), str(cyclic), str(kmax_log2)], input=text.encode(),
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return records(r.stdout)


def digest(rec):
    """what the golden file holds for one shape"""
    d = {t: hashlib.sha256(rec[t]).hexdigest() if rec[t] else "absent" for t in TABLES + HOST}
    d.update({k: int.from_bytes(rec[k], "little") for k in INTS})
    d["inv_qtop"] = rec["inv_qtop"].hex()
    return d


_CACHE = {}


def shape_records(exe, key):
    if key not in _CACHE:
        lb, n, idx, cyclic = SHAPES[key]
        prm = Sub(lb, idx)
        rec = run_tables(exe, lb, n, prm.P, prm.primitive_roots, prm.invkmax, cyclic, prm.kmax_log2)
        assert int.from_bytes(rec["rc"], "little") == 0, rec.get("error")
        _CACHE[key] = rec
    return _CACHE[key]


@pytest.mark.parametrize("key", list(SHAPES))
def test_every_table_equals_the_recorded_digest(key, dump_exe):
    want = json.load(open(GOLDEN))["shapes"]
    assert set(want) == set(SHAPES)
    got = digest(shape_records(dump_exe, key))
    assert got == want[key], sorted(k for k in got if got[k] != want[key].get(k))


def test_the_shapes_reach_every_branch(dump_exe):
    """what the shape list is there for: each optional table is present in one shape and absent in another"""
    d = {key: digest(shape_records(dump_exe, key)) for key in SHAPES}
    for t in TABLES:
        if t not in ("psi", "mc", "qhat", "qsh"):
            assert {d[k][t] == "absent" for k in d} == {True, False}, t
    assert d["u64/4096/20"]["crt_bfrag"] == "absent" != d["u64/4096/21"]["crt_bfrag"]
    assert d["u64/4096/16"]["crt_bproj"] == "absent" != d["u64/4096/17"]["crt_bproj"]
    assert d["u64/4096/32"]["qhat_w"] == "absent" != d["u64/4096/33"]["qhat_w"] and d["u64/4096/33"]["qparts"] == "absent"
    for key, small in (("u64/4096/94", 92), ("u64/4096/90-93", 2)):
        assert d[key]["small_delta"] == 0 and d[key]["nm_small"] == small
    assert d["u64/4096/0,1,1"]["resc"] == "absent" != d["u64/4096/4"]["resc"]
    assert d["u32/4096/1"]["mc_inc1"] != "absent" == d["u32/4096/1"]["mc_inc0"]


@pytest.mark.parametrize("key", [k for k in SHAPES if not SHAPES[k][3]])
def test_transform_tables_equal_the_emulator_s(key, dump_exe):
    """psi, mc, mc_inc and psi_lm word for word against asm_emu.device_tables (which leaves the two yinv fields zero)"""
    lb, n, idx, _ = SHAPES[key]
    rec, nm, dt = shape_records(dump_exe, key), len(idx), _NP[lb]
    tw = lambda name: np.frombuffer(rec[name], dtype=dt).reshape(nm, n, 2)          # Tw<T>
    mcs = lambda name: np.frombuffer(rec[name], dtype=dt).reshape(nm, 14)            # ModConst<T>
    keep = [c for c in range(14) if c not in (9, 10)]
    psi, mc = asm_emu.device_tables(lb, n, nm, Sub(lb, idx))
    assert np.array_equal(tw("psi"), psi)
    assert np.array_equal(mcs("mc")[:, keep], mc[:, keep])
    if rec["psi_lm"]:
        assert lb == 64 and n >= 4096
        assert np.array_equal(tw("psi_lm"), asm_emu.device_tables(lb, n, nm, Sub(lb, idx), lane_major=True)[0])
    else:
        assert lb != 64 or n < 4096
    small = int.from_bytes(rec["nm_small"], "little")   # (the emulator's level records exist for delta < 2^32: the prefix)
    for level in (1, 2):
        name = "mc_inc%d" % (level - 1)
        if rec[name]:
            assert len(rec[name]) == len(rec["mc"]) and small > 0
            want = asm_emu.device_tables(lb, n, small, Sub(lb, idx[:small]), incomplete=level)[1]
            assert np.array_equal(mcs(name)[:small, keep], want[:, keep]), name
    assert bool(rec["mc_inc1"]) == ((lb == 32 and 1024 <= n <= 4096) or (lb == 64 and n >= 1024 and small > 0))
    assert bool(rec["mc_inc0"]) == (lb == 64 and n >= 1024 and small > 0)


def _limbs(x, count):
    return [(x >> (64 * i)) & (2**64 - 1) for i in range(count)]


@pytest.mark.parametrize("key", [k for k in SHAPES if SHAPES[k][0] == 64])
def test_crt_constants_and_rescale_records_equal_their_definitions(key, dump_exe):
    _, n, idx, cyclic = SHAPES[key]
    rec, nm = shape_records(dump_exe, key), len(idx)
    P = [int(params(64).P[i]) for i in idx]
    u64 = lambda name: [int(v) for v in np.frombuffer(rec[name], dtype=np.uint64)]
    Q = 1
    for p in P:
        Q *= p
    L = (Q.bit_length() + 63) // 64
    assert int.from_bytes(rec["crt_L"], "little") == L and int.from_bytes(rec["crt_Lacc"], "little") == L + 1
    assert int.from_bytes(rec["h_Q"], "little") == Q and len(rec["h_Q"]) == 8 * L
    assert int.from_bytes(rec["crt_Q0"], "little") == Q % 2**64
    yinv = [pow(Q // p % p, p - 2, p) for p in P]       # (Q/p)^-1 mod p (0 for a repeated modulus, as the power gives it)
    lift, pos = u64("h_lifting"), 0
    for cm, p in enumerate(P):
        cnt = lift[pos]
        assert sum(v << (64 * i) for i, v in enumerate(lift[pos + 1:pos + 1 + cnt])) == (Q // p) * yinv[cm], cm
        pos += 1 + cnt
    assert pos == len(lift)
    mc = np.frombuffer(rec["mc"], dtype=np.uint64).reshape(nm, 14)
    assert [int(v) for v in mc[:, 9]] == yinv and [int(v) for v in mc[:, 10]] == [(y << 64) // p for y, p in zip(yinv, P)]
    ok = L + 1 <= 36           # the fixed row stride of qhat / qsh: beyond it the tables stay zero
    qhat, qsh = u64("qhat"), u64("qsh")
    assert len(qhat) == nm * 36 and len(qsh) == 6 * 36
    for cm, p in enumerate(P):
        assert qhat[36 * cm:36 * cm + 36] == (_limbs(Q // p, 36) if ok else [0] * 36), cm
    for k in range(6):
        assert qsh[36 * k:36 * k + 36] == (_limbs((Q << k) % 2**(64 * (L + 1)), 36) if ok else [0] * 36), k
    if rec["qhat_w"]:
        Lw, nsh = int.from_bytes(rec["crt_Lw"], "little"), int.from_bytes(rec["crt_nsh"], "little")
        assert Lw == L + 2 and 2**nsh > nm >= 2**(nsh - 1) and (nm > 32 or not ok)
        assert u64("qhat_w") == [v for p in P for v in _limbs(Q // p, Lw)]
        assert u64("qsh_w") == [v for k in range(nsh) for v in _limbs(Q << k, Lw)]
    else:
        assert nm <= 32 and ok
    coprime = all(P[-1] % p for p in P[:-1])
    if nm >= 2 and not cyclic and coprime:
        q = P[-1]
        want = [[pow(q % p, -1, p), (pow(q % p, -1, p) << 64) // p, (q - 1) // 2, p] for p in P[:-1]]
        assert np.frombuffer(rec["resc"], dtype=np.uint64).reshape(nm - 1, 4).tolist() == want
    else:
        assert not rec["resc"]


def test_the_three_validation_failures(dump_exe):
    for lb in (16, 32, 64):
        pr = params(lb)
        good = [int(pr.P[0]), int(pr.primitive_roots[0]), int(pr.invkmax[0])]
        for col, bad, msg in ((0, good[0] >> 1 | 1, "modulus is not (word-2) bits long"), (0, 2**(lb - 2) + 1, "modulus is not (word-2) bits long"),
                              (1, 1, "primitive root has the wrong order"), (2, good[2] ^ 1, "invkMaxPolyDegree is not the inverse")):
            row = list(good)
            row[col] = bad
            rec = run_tables(dump_exe, lb, 128, [row[0]], [row[1]], [row[2]], 0, pr.kmax_log2)
            assert int.from_bytes(rec["rc"], "little") == 1 and rec["error"].decode() == msg, (lb, col, rec)
            assert set(rec) == {"rc", "error"}
        rec = run_tables(dump_exe, lb, 128, [good[0]], [good[1]], [good[2]], 0, pr.kmax_log2)
        assert int.from_bytes(rec["rc"], "little") == 0


@pytest.mark.parametrize("key", G.shape_keys(G.load()[0], mode="full"))
def test_reference_layout_tables_equal_the_reference_s(key, dump_exe):
    """the host half of nflhip_get_table against the arrays tests/test_oracle_golden.py pins the oracle with (modulus 0)"""
    index, arr = G.load()
    ent = index["shapes"][key]
    lb, n = ent["limb_bits"], ent["degree"]
    pr = params(lb)
    p, phi = int(pr.P[0]), int(pr.primitive_roots[0])
    for _ in range(pr.kmax_log2 - (n.bit_length() - 1)):
        phi = phi * phi % p
    for which, name in ((3, "phis"), (4, "shoupphis"), (5, "invpoly_times_invphis"), (7, "omegas"), (8, "invomegas")):   # NFLHIP_TAB_*
        r = subprocess.run([dump_exe, "reftab", str(lb), str(n), str(pr.kmax_log2), str(which), str(p), str(phi), str(int(pr.invkmax[0]))],
                           capture_output=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.frombuffer(records(r.stdout)["table"], dtype=np.uint64)
        want = np.asarray(arr["%s/table_%s" % (key, name)]).reshape(-1)
        assert got.shape == want.shape and np.array_equal(got, want.astype(np.uint64)), name
        assert int(got.max()) < 2**lb
