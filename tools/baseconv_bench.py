#!/usr/bin/env python3
"""Time the RNS base conversion and the mod-down (nflhip_baseconv_dev, nflhip_moddown_dev) in one run.  Per point: the time, the
compulsory bytes over time -- the ks source rows read plus the destination rows written (in place, a destination row that is a
source row is a copy and does not count); for the mod-down nm rows read plus nm - k written -- and the ratio to a same-run
hipMemcpyAsync device-to-device copy moving the same byte count (read + write).  The mod-down by one modulus is alternated with
the same run's nflhip_rescale_dev in coefficient form.  For scale: the host route (crt_lift, Python integers, crt_project) at a
batch of a few polynomials.
Every figure: two warm-up calls, then --iters calls between two HIP events, repeated --reps times; the median is reported.

The NTT-form entries (nflhip_baseconv_ntt_dev, nflhip_moddown_ntt_dev; --form ntt): per point the one-launch kernel, the composed plan
and a device copy of the compulsory bytes -- rows S read plus rows D \ S written, or nm read plus nm - k written -- alternated block
by block in the same run.

usage: tools/baseconv_bench.py [--form coeff|ntt|both] [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per measurement)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, what, src, dst or k): batch sized to about 1 GiB of compulsory traffic
POINTS = [(64, 4096, 4, "mod_up", (0, 2), (0, 4)), (64, 4096, 4, "mod_up", (0, 1), (0, 4)), (64, 4096, 4, "mod_up centred", (0, 2), (0, 4)),
          (64, 4096, 4, "mod_down", None, 1), (64, 4096, 4, "mod_down", None, 2), (64, 4096, 4, "mod_down floor", None, 2),
          (32, 4096, 3, "mod_up", (0, 1), (0, 3)), (64, 4096, 32, "mod_up", (0, 16), (0, 32)), (64, 4096, 32, "mod_up", (0, 17), (0, 32))]

# NTT form: (limb bits, degree, moduli, what, src, dst or k, plans)
NTT_POINTS = [(lb, n, nm, what, src, dst, ("fused", "composed"))
              for lb, n, nm in ((64, 1024, 4), (64, 2048, 4))
              for what, src, dst in (("mod_up", (0, 1), (0, 4)), ("mod_up", (0, 2), (0, 4)), ("mod_down", None, 1), ("mod_down", None, 2))]
NTT_POINTS += [(32, 4096, 3, "mod_up", (0, 1), (0, 3), ("fused", "composed")), (32, 4096, 3, "mod_down", None, 1, ("fused", "composed")),
               (64, 4096, 4, "mod_up", (0, 1), (0, 4), ("fused", "composed"))]   # rows of 32 KiB: the default composes, the kernel is forced


def timed(fn, iters, reps):
    """median over `reps` of the mean milliseconds per call (HIP events on the current stream), after two warm-up calls"""
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return float(np.median(ms))


def timed_pair(fa, fb, iters, reps):
    """two variants alternated block by block in one run: (median a, median b)"""
    for f in (fa, fb, fa, fb):
        f()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for k, f in enumerate((fa, fb)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                f()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / iters)
    return float(np.median(ms[0])), float(np.median(ms[1]))


def timed_alternated(fns, iters, reps):
    """any number of variants alternated block by block in one run: their medians"""
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
    return [float(np.median(m)) for m in ms]


def ntt_points(it, rp, lines, rows):
    """the NTT-form entries: both plans and the copy in the same run; which plan the default call takes is read off its time"""
    for lb, n, nm, what, src, dst, plans in NTT_POINTS:
        e = Engine(lb, n, nm)
        row = n * (lb // 8)
        down = what.startswith("mod_down")
        if down:
            k = dst
            nrows = nm + nm - k
        else:
            written = [j for j in range(dst[0], dst[0] + dst[1]) if not src[0] <= j < src[0] + src[1]]
            nrows = src[1] + len(written)
        batch = max(GIB // (nrows * row), 1)
        moved = batch * nrows * row
        a = e.fill_uniform(e.empty(batch), 1, 0)
        half = moved // 2 // 16 * 16
        cs, cd = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        if down:
            out = e.mod_down_ntt(a, k)
            call = lambda plan: (lambda: e.mod_down_ntt(a, k, out=out, plan=plan))  # noqa: E731
        else:
            call = lambda plan: (lambda: e.baseconv_ntt(a, src, dst, plan=plan))    # noqa: E731  (in place: the source rows do not change)
        fns = [call(p) for p in plans] + [call(None), lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))]
        ms = timed_alternated(fns, it, rp)
        ms_copy, ms_default = ms[-1], ms[-2]
        ctbs = 2 * half / ms_copy / 1e9
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "form": "ntt", "what": what, "batch": batch, "rows_moved": nrows, "copy_ms": round(ms_copy, 4),
               "copy_TB_per_s": round(ctbs, 3), "default_ms": round(ms_default, 4)}
        rec.update({"k": dst} if down else {"src": list(src), "dst": list(dst)})
        for p, t in zip(plans, ms):
            rec[p + "_ms"] = round(t, 4)
            rec[p + "_TB_per_s"] = round(moved / t / 1e9, 3)
            rec[p + "_ratio_to_copy"] = round(ms_copy / t, 3)
        rec["composed_over_fused"] = round(rec["composed_ms"] / rec["fused_ms"], 3)
        lines.append(json.dumps(rec))
        label = "%s k=%d" % (what, dst) if down else "%s %d->%d" % (what, src[1], dst[1])
        rows.append("%-12s ntt %-14s batch %6d  fused %8.3f ms %5.2f TB/s (x%.3f of copy)  composed %8.3f ms %5.2f TB/s (x%.3f)  composed/fused x%.3f  "
                    "default %8.3f ms  copy %8.3f ms %5.2f TB/s  (%d rows)" % (
                        rec["shape"], label, batch, rec["fused_ms"], rec["fused_TB_per_s"], rec["fused_ratio_to_copy"], rec["composed_ms"],
                        rec["composed_TB_per_s"], rec["composed_ratio_to_copy"], rec["composed_over_fused"], ms_default, ms_copy, ctbs, nrows))
        del a, cs, cd, fns
        e.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-polys", type=int, default=2, help="polynomials of the host-route context figure")
    ap.add_argument("--form", choices=("coeff", "ntt", "both"), default="both")
    args = ap.parse_args()
    it, rp = args.iters, args.reps
    lines, rows = [], []
    for lb, n, nm, what, src, dst in (POINTS if args.form != "ntt" else []):
        e = Engine(lb, n, nm)
        row = n * (lb // 8)
        down = what.startswith("mod_down")
        if down:
            k = dst
            nrows, macs = nm + nm - k, k * (nm - k)
        else:
            written = [j for j in range(dst[0], dst[0] + dst[1]) if not src[0] <= j < src[0] + src[1]]
            nrows, macs = src[1] + len(written), src[1] * len(written)
        batch = max(GIB // (nrows * row), 1)
        moved = batch * nrows * row
        a = e.fill_uniform(e.empty(batch), 1, 0)
        half = moved // 2 // 16 * 16
        cs, cd = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        ms_copy = timed(lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st)), it, rp)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "what": what, "batch": batch, "rows_moved": nrows, "multiply_adds_per_position": macs}
        if down:
            out = e.mod_down(a, k, floor="floor" in what)
            ms = timed(lambda: e.mod_down(a, k, floor="floor" in what, out=out), it, rp)
            rec["k"] = k
            if k == 1:
                ms_md, ms_rs = timed_pair(lambda: e.mod_down(a, 1, out=out), lambda: e.rescale(a, out=out), it, rp)
                rec.update({"alternated_mod_down_ms": round(ms_md, 4), "alternated_rescale_ms": round(ms_rs, 4), "mod_down_over_rescale": round(ms_md / ms_rs, 3)})
            del out
        else:
            rec.update({"src": list(src), "dst": list(dst)})
            ms = timed(lambda: e.baseconv(a, src, dst, centered="centred" in what), it, rp)   # in place: the source rows do not change
        tbs, ctbs = moved / ms / 1e9, 2 * half / ms_copy / 1e9
        rec.update({"ms": round(ms, 4), "TB_per_s": round(tbs, 3), "copy_ms": round(ms_copy, 4), "copy_TB_per_s": round(ctbs, 3),
                    "ratio_to_copy": round(tbs / ctbs, 3), "polys_per_s": round(batch / ms * 1e3)})
        lines.append(json.dumps(rec))
        label = "%s k=%d" % (what, dst) if down else "%s %d->%d" % (what, src[1], dst[1])
        rows.append("%-12s %-22s batch %5d  %8.3f ms %6.2f TB/s   copy %8.3f ms %6.2f TB/s  ratio %.3f  (%d rows, %d multiply-adds per position)%s" % (
            rec["shape"], label, batch, ms, tbs, ms_copy, ctbs, tbs / ctbs, nrows, macs,
            "   alternated with rescale: %.3f / %.3f ms = x%.3f" % (rec["alternated_mod_down_ms"], rec["alternated_rescale_ms"], rec["mod_down_over_rescale"]) if "mod_down_over_rescale" in rec else ""))
        del a, cs, cd
        e.close()
        torch.cuda.empty_cache()
    if args.form != "coeff":
        ntt_points(it, rp, lines, rows)
    if args.form != "ntt":
        host_route(args.host_polys, lines, rows)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/baseconv_bench.py --form %s --iters %d --reps %d (MI355X): bytes = source rows read + destination rows written (in place: "
                    "without the rows that are copies); mod-down: nm rows read + nm - k written; copy = hipMemcpyAsync D2D moving the same bytes\n" % (args.form, it, rp))
            f.write(text)


def host_route(hp, lines, rows):
    # for scale, the route without this feature: lift to integers on the device, divide and round in Python, project
    lb, n, nm, k = 64, 4096, 4, 2
    e, s = Engine(lb, n, nm), Engine(lb, n, nm - k)
    x = e.fill_uniform(e.empty(hp), 1, 0)
    want = e.mod_down(x, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    limbs = e.crt_lift(x).cpu().numpy().view(np.uint64)
    Pk = 1
    for p in e.P[nm - k:]:
        Pk *= p
    out_limbs = np.zeros((hp, n, s.crt_limbs), dtype=np.uint64)
    for b in range(hp):
        for i in range(n):
            X = int.from_bytes(limbs[b, i].tobytes(), "little")
            Y = X // Pk + (2 * (X % Pk) >= Pk)
            out_limbs[b, i] = np.frombuffer(Y.to_bytes(8 * s.crt_limbs + 8, "little")[:8 * s.crt_limbs], dtype=np.uint64)
    got = s.crt_project(torch.from_numpy(out_limbs.view(np.int64)).to(x.device))
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    same = bool(torch.equal(got, want))
    rec = {"shape": "u64/4096/4", "what": "host route: crt_lift, Python integers, crt_project (mod_down k=2)", "host_polys": hp,
           "host_seconds": round(sec, 4), "host_polys_per_s": round(hp / sec, 2), "same_words_as_mod_down": same}
    lines.append(json.dumps(rec))
    rows.append("u64/4096/4   host route (crt_lift, Python integers, crt_project), mod_down k=2: %d polys in %.3f s = %.1f polys/s (same words: %s)" % (
        hp, sec, hp / sec, same))
    e.close()
    s.close()


if __name__ == "__main__":
    main()
