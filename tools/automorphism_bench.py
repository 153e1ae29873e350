#!/usr/bin/env python3
"""Time the Galois automorphisms (nflhip_automorphism_dev / nflhip_automorphism_multi_dev) against a same-run
hipMemcpyAsync device-to-device copy of the same bytes (nflhip_memcpy_d2d).  Bytes are read plus written; the ratio
is automorphism rate / copy rate.  Also: the multi form with 8 outputs against 8 single calls.

usage: tools/automorphism_bench.py [--iters N] [--out FILE]   (one line of JSON per measurement, plus a table)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

# (limb bits, degree, moduli, batch): the headline shape, the longest row, and the rows around the plan boundaries
CONFIGS = [(64, 4096, 4, 16384), (64, 65536, 30, 64), (64, 8192, 4, 4096), (64, 16384, 4, 2048), (64, 32768, 4, 1024),
           (32, 4096, 3, 8192), (64, 1024, 2, 32768)]


def timed(fn, iters):
    """mean milliseconds per call, HIP events on the current stream, after two warm-up calls"""
    fn()
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines, rows = [], []
    for lb, n, nm, batch in CONFIGS:
        e = Engine(lb, n, nm)
        a = e.fill_uniform(e.empty(batch), 1, 0)
        out = torch.empty_like(a)
        nbytes = batch * e.bytes_per_poly
        st = e._stream()
        ms_copy = timed(lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, out.data_ptr(), a.data_ptr(), nbytes, st)), args.iters)
        copy_tbs = 2 * nbytes / ms_copy / 1e9
        for form in ("coeff", "ntt"):
            ntt = form == "ntt"
            ms = timed(lambda: e.automorphism(a, 5, ntt=ntt, out=out), args.iters)
            tbs = 2 * nbytes / ms / 1e9
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "batch": batch, "form": form, "ms": round(ms, 4),
                   "TB_per_s": round(tbs, 3), "copy_ms": round(ms_copy, 4), "copy_TB_per_s": round(copy_tbs, 3),
                   "ratio_to_copy": round(tbs / copy_tbs, 3)}
            lines.append(json.dumps(rec))
            rows.append("%-14s batch %6d  %-5s %9.3f ms  %6.2f TB/s   copy %9.3f ms %6.2f TB/s   ratio %.3f" % (
                rec["shape"], batch, form, ms, tbs, ms_copy, copy_tbs, tbs / copy_tbs))
        del out
        if (lb, n, nm) == (64, 4096, 4):
            # hoisted rotations: 8 outputs from one read of the input, against 8 single calls
            b = 2048
            x = a[:b]
            ks = [3, 5, 7, 9, 11, 13, 15, 2 * n - 1]
            outs = [torch.empty_like(x) for _ in ks]
            for form in ("coeff", "ntt"):
                ntt = form == "ntt"
                ms_multi = timed(lambda: e.automorphism_multi(x, ks, ntt=ntt, outs=outs), args.iters)

                def singles():
                    for k, o in zip(ks, outs):
                        e.automorphism(x, k, ntt=ntt, out=o)
                ms_single = timed(singles, args.iters)
                rec = {"shape": "u64/4096/4", "batch": b, "form": form, "outputs": len(ks), "multi_ms": round(ms_multi, 4),
                       "singles_ms": round(ms_single, 4), "speedup": round(ms_single / ms_multi, 3),
                       "ideal_speedup": round(2 * len(ks) / (len(ks) + 1), 3)}
                lines.append(json.dumps(rec))
                rows.append("u64/4096/4     batch %6d  %-5s multi(8) %8.3f ms  8 singles %8.3f ms  speedup %.3f (byte ratio %.3f)" % (
                    b, form, ms_multi, ms_single, ms_single / ms_multi, 2 * len(ks) / (len(ks) + 1)))
            del outs
        del a
        e.close()
        torch.cuda.empty_cache()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/automorphism_bench.py --iters %d (MI355X): bytes = read + write; copy = hipMemcpyAsync D2D of the same bytes\n"
                    % args.iters)
            f.write(text)


if __name__ == "__main__":
    main()
