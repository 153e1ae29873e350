#!/usr/bin/env python3
"""Time the hybrid key switch in NTT form (nflhip_keyswitch_ntt_dev) in one run.  Per point the plans -- sequence (the existing
entries, run one after the other: what a caller had before this entry), composed, fused where it fits -- the default call and a
hipMemcpyAsync device-to-device copy of the compulsory bytes are alternated block by block: --reps blocks of --iters calls between
two HIP events each, after two warm-up calls of every variant.  Reported per variant: the median of the block means and the spread
(max - min) / median of its blocks in this run.  Compulsory bytes: L rows read, 2 L rows written, the key read once.

usage: tools/keyswitch_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine, NflHipError  # noqa: E402
from nfllib_amd._lib import ERR_UNSUPPORTED  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, k_special, alpha): batch sized to about 1 GiB of compulsory traffic
POINTS = [(64, 1024, 4, 1, 1), (64, 1024, 4, 1, 3), (64, 2048, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 4, 2, 2), (32, 4096, 3, 1, 1)]
PLANS = ("sequence", "composed", "fused")


def timed_alternated(fns, iters, reps):
    """any number of variants alternated block by block in one run: per variant the list of block means in milliseconds"""
    for f in tuple(fns) * 2:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                f()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / iters)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per call the batch is sized to")
    args = ap.parse_args()
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum * nm * row
        batch = max(int(args.gib * GIB - kbytes) // (3 * L * row), 1)
        moved = batch * 3 * L * row + kbytes
        kept = Engine(lb, n, L)                                   # the input's ring: canonical words under the first L moduli
        a = kept.fill_uniform(kept.empty(batch), 1, 0)
        kept.close()
        key = e.fill_uniform(e.empty(2 * dnum), 2, 0)
        out = e.key_switch_ntt(a, key, K, alpha, plan="sequence")
        plans = []
        for p in PLANS:
            try:
                got = e.key_switch_ntt(a, key, K, alpha, plan=p)
            except NflHipError as err:
                if err.code != ERR_UNSUPPORTED:
                    raise
                continue
            assert torch.equal(got[0], out[0]) and torch.equal(got[1], out[1]), (lb, n, nm, K, alpha, p)
            plans.append(p)
        half = moved // 2 // 16 * 16
        cs, cd = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        call = lambda plan: (lambda: e.key_switch_ntt(a, key, K, alpha, out=out, plan=plan))      # noqa: E731
        fns = [call(p) for p in plans] + [call(None), lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))]
        ms = timed_alternated(fns, args.iters, args.reps)
        med = [float(np.median(m)) for m in ms]
        spread = [float((max(m) - min(m)) / np.median(m)) for m in ms]
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "dnum": dnum, "batch": batch, "compulsory_bytes": moved}
        for name, t, s in zip(plans + ["default", "copy"], med, spread):
            rec[name + "_ms"], rec[name + "_spread"] = round(t, 4), round(s, 4)
        seq = rec["sequence_ms"]
        for name in plans[1:] + ["default"]:
            rec["sequence_over_" + name] = round(seq / rec[name + "_ms"], 3)
        rec["default_ratio_to_copy"] = round(rec["copy_ms"] / rec["default_ms"], 3)
        rec["default_TB_per_s"] = round(moved / rec["default_ms"] / 1e9, 3)
        lines.append(json.dumps(rec))
        cell = lambda name: ("%8.3f ms (+-%4.1f%%)" % (rec[name + "_ms"], 100 * rec[name + "_spread"])) if name + "_ms" in rec else "       -- (no fit)  "  # noqa: E731
        rows.append("%-11s K=%d alpha=%d dnum=%d batch %6d  sequence %s  composed %s x%.3f  fused %s %s  default %s x%.3f  copy %s" % (
            rec["shape"], K, alpha, dnum, batch, cell("sequence"), cell("composed"), rec["sequence_over_composed"], cell("fused"),
            ("x%.3f" % rec["sequence_over_fused"]) if "fused" in plans else "      ", cell("default"), rec["sequence_over_default"], cell("copy")))
        del a, key, out, cs, cd, fns
        e.close()
        torch.cuda.empty_cache()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/keyswitch_bench.py --iters %d --reps %d (MI355X): x = sequence / plan (above 1: the plan is faster than the existing entries "
                    "run one after the other); +- = (max - min) / median of the plan's blocks in this run; copy = hipMemcpyAsync D2D of the compulsory "
                    "bytes (L rows read, 2 L written, the key once)\n" % (args.iters, args.reps))
            f.write(text)


if __name__ == "__main__":
    main()
