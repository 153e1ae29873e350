#!/usr/bin/env python3
"""Time the RNS scale-and-round by t/Q (nflhip_scale_round_dev) and the BFV tensor product built on it (nflhip_bfv_tensor_ntt_dev) in
one run.  Per point of the scale-round: the one-pass kernel, the two-pass plan and a hipMemcpyAsync device-to-device copy moving the
compulsory bytes -- nm rows read plus ks written -- alternated block by block; the time, the compulsory bytes over time and the
ratios.  Per point of the tensor product: the one call against its four-step composition through the existing entries (embed and
base-extend each input, tensor product on nm rows, scale-round each component), alternated likewise.
Every figure: one untimed block of every variant, then --iters calls between two HIP events, repeated --reps times; the median and
the spread (min .. max over the blocks) are reported, and for a ratio its extremes (fastest block over slowest and the reverse).

usage: tools/scale_round_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per measurement)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, ks, t): batch sized to about 1 GiB of compulsory traffic
POINTS = [(64, 4096, 9, 4, 65537), (32, 4096, 7, 3, 257)]
# (limb bits, degree, L, kb, t, batch)
BFV_POINTS = [(64, 4096, 4, 5, 65537, 128), (32, 4096, 3, 4, 257, 256)]


def timed_alternated(fns, iters, reps):
    """any number of variants alternated block by block in one run: per variant (median, min, max) milliseconds per call"""
    for f in fns:                                     # the warm-up: one untimed block of every variant (first calls allocate; clocks settle)
        for _ in range(max(iters, 2)):
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
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def scale_round_points(it, rp, lines, rows):
    for lb, n, nm, ks, t in POINTS:
        e = Engine(lb, n, nm)
        row = n * (lb // 8)
        nrows = nm + ks
        batch = max(GIB // (nrows * row), 1)
        moved = batch * nrows * row
        a = e.fill_uniform(e.empty(batch), 1, 0)
        out = e.scale_round(a, ks, t)
        assert torch.equal(out, e.scale_round(a, ks, t, plan="two_pass"))
        half = moved // 2 // 16 * 16
        cs, cd = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        fns = [lambda: e.scale_round(a, ks, t, out=out), lambda: e.scale_round(a, ks, t, out=out, plan="two_pass"),
               lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))]
        (one, one_lo, one_hi), (two, two_lo, two_hi), (cp, cp_lo, cp_hi) = timed_alternated(fns, it, rp)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "what": "scale_round", "ks": ks, "t": t, "batch": batch, "rows_moved": nrows,
               "multiply_adds_per_position": 2 * ks * (nm - ks), "one_pass_ms": round(one, 4), "one_pass_ms_range": [round(one_lo, 4), round(one_hi, 4)],
               "one_pass_TB_per_s": round(moved / one / 1e9, 3), "two_pass_ms": round(two, 4), "two_pass_ms_range": [round(two_lo, 4), round(two_hi, 4)],
               "copy_ms": round(cp, 4), "copy_ms_range": [round(cp_lo, 4), round(cp_hi, 4)], "copy_TB_per_s": round(2 * half / cp / 1e9, 3),
               "one_pass_ratio_to_copy": round(cp / one, 3), "one_pass_ratio_to_copy_range": [round(cp_lo / one_hi, 3), round(cp_hi / one_lo, 3)],
               "two_pass_over_one_pass": round(two / one, 3), "two_pass_over_one_pass_range": [round(two_lo / one_hi, 3), round(two_hi / one_lo, 3)],
               "polys_per_s": round(batch / one * 1e3)}
        lines.append(json.dumps(rec))
        rows.append("%-12s scale_round ks=%d batch %5d  one pass %8.3f ms (%.3f .. %.3f) %5.2f TB/s  x%.3f of copy (%.3f .. %.3f)   two passes %8.3f ms (%.3f .. %.3f)"
                    "  two/one x%.3f (%.3f .. %.3f)   copy %8.3f ms %5.2f TB/s  (%d rows, %d multiply-adds per position)" % (
                        rec["shape"], ks, batch, one, one_lo, one_hi, rec["one_pass_TB_per_s"], rec["one_pass_ratio_to_copy"], cp_lo / one_hi, cp_hi / one_lo,
                        two, two_lo, two_hi, rec["two_pass_over_one_pass"], two_lo / one_hi, two_hi / one_lo, cp, rec["copy_TB_per_s"], nrows,
                        rec["multiply_adds_per_position"]))
        del a, out, cs, cd, fns
        e.close()
        torch.cuda.empty_cache()


def bfv_points(it, rp, lines, rows):
    for lb, n, L, kb, t, batch in BFV_POINTS:
        nm = L + kb
        e, el = Engine(lb, n, nm), Engine(lb, n, L)
        ins = [el.fill_uniform(el.empty(batch), 5, k) for k in range(4)]
        ext = [torch.zeros((batch, nm, n), dtype=e.torch_dtype, device=ins[0].device) for _ in range(4)]
        ten = torch.empty((3, batch, nm, n), dtype=e.torch_dtype, device=ins[0].device)
        res = [torch.empty((3, batch, L, n), dtype=e.torch_dtype, device=ins[0].device) for _ in range(2)]

        def one_call():
            e.bfv_tensor_ntt(ins[0], ins[1], ins[2], ins[3], L, t, outs=(res[0][0], res[0][1], res[0][2]))

        def four_steps():
            for x, E in zip(ins, ext):
                E[:, :L] = x
                e.baseconv_ntt(E, (0, L), (0, nm), centered=True)
            e.tensor_ntt(ext[0], ext[1], ext[2], ext[3], outs=(ten[0], ten[1], ten[2]))
            for c in range(3):
                e.scale_round(ten[c], L, t, ntt=True, out=res[1][c])
        (one, one_lo, one_hi), (four, four_lo, four_hi) = timed_alternated([one_call, four_steps], it, rp)
        same = bool(torch.equal(res[0], res[1]))
        rec = {"shape": "u%d/%d" % (lb, n), "what": "bfv_tensor_ntt", "L": L, "kb": kb, "t": t, "batch": batch, "one_call_ms": round(one, 4),
               "one_call_ms_range": [round(one_lo, 4), round(one_hi, 4)], "four_steps_ms": round(four, 4),
               "four_steps_ms_range": [round(four_lo, 4), round(four_hi, 4)], "four_steps_over_one_call": round(four / one, 3),
               "four_steps_over_one_call_range": [round(four_lo / one_hi, 3), round(four_hi / one_lo, 3)], "products_per_s": round(batch / one * 1e3),
               "same_words": same}
        lines.append(json.dumps(rec))
        rows.append("%-12s bfv_tensor_ntt L=%d kb=%d batch %4d  one call %8.3f ms (%.3f .. %.3f)  four steps %8.3f ms (%.3f .. %.3f)  four/one x%.3f (%.3f .. %.3f)"
                    "  %d products/s  same words: %s" % (rec["shape"], L, kb, batch, one, one_lo, one_hi, four, four_lo, four_hi, rec["four_steps_over_one_call"],
                                                         four_lo / one_hi, four_hi / one_lo, rec["products_per_s"], same))
        del ins, ext, ten, res
        e.close()
        el.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines, rows = [], []
    scale_round_points(args.iters, args.reps, lines, rows)
    bfv_points(args.iters, args.reps, lines, rows)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/scale_round_bench.py --iters %d --reps %d (MI355X): bytes = nm rows read + ks written; copy = hipMemcpyAsync D2D moving the "
                    "same bytes; every variant of a point alternated block by block in one run; (lo .. hi) = the blocks' extremes\n" % (args.iters, args.reps))
            f.write(text)


if __name__ == "__main__":
    main()
