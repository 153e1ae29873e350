#!/usr/bin/env python3
"""Calls every launcher family of nfllib_amd/csrc/asm_launch.hip once, at the smallest shape that reaches it.

A launcher that declines (hipErrorNotSupported) hands the call to the compiled kernels, which compute the same words: no
correctness test can see that.  The kernel trace can.  Run

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/asm_launch_families.py
    python tools/asm_launch_families.py --table OUT

on two builds: the tables (kernel name, calls) must be equal.  profiles/r10_asm_launch_trace.txt is that table.

Only the public Engine API is used, plus nflhip_debug_polymul_level for the products on complete (0) and one-stage-short (1)
transforms.  Operands are zeros: valid residues, and the launchers do not look at the data.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(out_dir):
    calls = {}
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    for name in sorted(calls):
        print("%-72s %6d" % (name, calls[name]))
    return 0 if calls else 1


def main():
    import torch
    from nfllib_amd import Engine, _lib

    def level(l):
        _lib.lib.nflhip_debug_polymul_level(l)

    def standard(eng, batch, levels=(2,)):
        """product (coefficient form, per level), pre-transformed product, both transforms"""
        a, b = eng.empty(batch).zero_(), eng.empty(batch).zero_()
        for l in levels:
            level(l)
            eng.polymul(a, b)
        level(2)
        eng.polymul(a, b, b_is_ntt=True)
        eng.ntt_(a)
        eng.intt_(a)

    def fused(eng, batch, formats):
        """the four fused kinds: enc2, fma_fwd, fms_inv, fma_inv; forward inputs in each of `formats`, keys shared by the batch"""
        k, w = eng.empty(1).zero_(), eng.empty(batch).zero_()
        for fmt in formats:
            x = eng.empty_small(batch).zero_() if fmt == "i8" else w
            eng.fwd_fma2(x, k, x, k, x)
            eng.fwd_fma(x, k, x)
        eng.fma_inv(w, k, w, subtract=True)
        eng.fma_inv(w, k, w)

    # 64-bit limbs, rows of 4096: single-row and two-row transforms, the product at every level
    eng = Engine(64, 4096, 2)
    standard(eng, 1, levels=(0, 1, 2))
    standard(eng, 2)
    fused(eng, 2, ("i8",))
    eng.close()
    # ... with moduli past the delta-form prefix: the split between the generated and the compiled family
    eng = Engine(64, 4096, 93)
    standard(eng, 1, levels=(0, 1, 2))
    standard(eng, 2)
    eng.close()
    # rows of 8192 / 16384 words
    for n in (8192, 16384):
        eng = Engine(64, n, 2)
        standard(eng, 1, levels=(0, 2))
        standard(eng, 2)
        fused(eng, 2, ("i8",))
        eng.close()
    # rows of 32768 words: the composed pair (plan forced off), then the one-launch plan (it needs 32 rows)
    os.environ["NFLHIP_XCD"] = "0"
    eng = Engine(64, 32768, 2)
    standard(eng, 2, levels=(0, 2))
    fused(eng, 2, ("i8",))     # int8 forward pipelines, the inverse pipelines
    eng.close()
    del os.environ["NFLHIP_XCD"]
    eng = Engine(64, 32768, 2)
    for l in (0, 2):
        level(l)
        a = eng.empty(16).zero_()
        eng.polymul(a, a)
    eng.close()
    # n = 65536, one modulus: the pipeline kernel (coefficient form at both levels, pre-transformed), the one-launch plan
    eng = Engine(64, 65536, 1)
    standard(eng, 4, levels=(0, 2))
    for l in (0, 2):
        level(l)
        a = eng.empty(32).zero_()
        eng.polymul(a, a)
    eng.close()
    # one row per wave: 64-bit limbs n = 1024 / 2048, 32-bit limbs n = 1024 / 2048 / 4096
    for bits, ns in ((64, (1024, 2048)), (32, (1024, 2048, 4096))):
        for n in ns:
            eng = Engine(bits, n, 2)
            standard(eng, 1, levels=(0, 2))
            fused(eng, 2, ("words", "i8"))
            eng.close()
    # 32-bit limbs n = 8 and 16-bit limbs n = 128: modes 0 - 3
    for bits, n in ((32, 8), (16, 128)):
        eng = Engine(bits, n, 2)
        standard(eng, 1)
        eng.close()
    level(2)
    torch.cuda.synchronize()
    print("asm_launch_families: done")
    return 0


if __name__ == "__main__":
    sys.exit(table(sys.argv[2]) if len(sys.argv) == 3 and sys.argv[1] == "--table" else main())
