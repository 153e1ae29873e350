#!/usr/bin/env python3
"""Time the gadget decomposition (nflhip_decompose_dev) in one run:
  coefficient form -- compulsory bytes (nm rows read plus the output written) over time, next to a same-run hipMemcpyAsync
                      device-to-device copy moving the same byte count (read + write) and a same-run fill (hipMemsetAsync) of the
                      output's bytes: the pass is almost all stores;
  NTT form         -- the one-launch kernel (NFLHIP_DECOMP_FUSED) against the composed plan (NFLHIP_DECOMP_COMPOSED), alternated in
                      one run, what the dispatcher runs by default (the nearer of the two timings names it), and each against the
                      same run's nflhip_ntt_fwd_dev alone on batch * terms polynomials;
  pipeline         -- decompose (NTT form) plus the two dots of a key switch at u64/4096/4, w = 31, against the same work with the
                      digits formed on the host (Python integers, small batch, scaled to the batch).
Every figure: two warm-up calls, then --iters calls between two HIP events, repeated --reps times; the median is reported.

usage: tools/decompose_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per measurement)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

# (limb bits, degree, moduli, batch, w, signed, format)
COEFF = [(64, 4096, 4, 1024, 31, True, "words"), (64, 4096, 4, 512, 16, True, "words"), (64, 4096, 4, 1024, 31, False, "words"),
         (64, 4096, 4, 8192, 31, True, "i32"), (64, 4096, 4, 8192, 15, True, "i16"), (32, 4096, 3, 2048, 15, True, "words")]
# (limb bits, degree, moduli, batch, w)
NTT = [(64, 1024, 2, 4096, 31), (64, 2048, 2, 2048, 31), (64, 4096, 4, 512, 31), (32, 1024, 2, 8192, 15), (32, 4096, 3, 2048, 15)]
_ESZ = {"i8": 1, "i16": 2, "i32": 4}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-polys", type=int, default=2, help="polynomials of the host-decomposition context figure")
    args = ap.parse_args()
    it, rp = args.iters, args.reps
    lines, rows = [], []
    for lb, n, nm, batch, w, signed, fmt in COEFF:
        e = Engine(lb, n, nm)
        terms = e.decompose_terms(w)
        a = e.fill_uniform(e.empty(batch), 1, 0)
        out = e.decompose(a, w, signed=signed, fmt=fmt)
        in_bytes = batch * nm * n * (lb // 8)
        out_bytes = out.numel() * out.element_size()
        moved = in_bytes + out_bytes
        half = moved // 2 // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        ms_copy = timed(lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, dst.data_ptr(), src.data_ptr(), half, st)), it, rp)
        ms_fill = timed(lambda: e._chk(e.lib.nflhip_memset_dev(e.ctx, out.data_ptr(), 0, out_bytes, st)), it, rp)
        ms = timed(lambda: e.decompose(a, w, signed=signed, fmt=fmt, out=out), it, rp)
        tbs, ctbs, ftbs = moved / ms / 1e9, 2 * half / ms_copy / 1e9, out_bytes / ms_fill / 1e9
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "batch": batch, "w": w, "signed": signed, "format": fmt, "terms": terms, "form": "coeff",
               "ms": round(ms, 4), "TB_per_s": round(tbs, 3), "copy_ms": round(ms_copy, 4), "copy_TB_per_s": round(ctbs, 3),
               "ratio_to_copy": round(tbs / ctbs, 3), "fill_ms": round(ms_fill, 4), "fill_TB_per_s": round(ftbs, 3),
               "time_over_fill_of_the_output": round(ms / ms_fill, 3), "polys_per_s": round(batch / ms * 1e3)}
        lines.append(json.dumps(rec))
        rows.append("%-12s batch %5d w %2d %-8s %-5s  %8.3f ms %6.2f TB/s   copy %8.3f ms %6.2f TB/s ratio %.3f   fill of the output %8.3f ms %6.2f TB/s (time x%.2f)" % (
            rec["shape"], batch, w, "signed" if signed else "unsigned", fmt, ms, tbs, ms_copy, ctbs, tbs / ctbs, ms_fill, ftbs, ms / ms_fill))
        if fmt == "words" and signed:
            g = e.gadget_mul(a, w, out=out)
            ms_g = timed(lambda: e.gadget_mul(a, w, out=g), it, rp)
            rec = {"shape": rec["shape"], "batch": batch, "w": w, "form": "gadget_mul", "ms": round(ms_g, 4), "TB_per_s": round(moved / ms_g / 1e9, 3),
                   "ratio_to_copy": round(moved / ms_g / 1e9 / ctbs, 3)}
            lines.append(json.dumps(rec))
            rows.append("%-12s batch %5d w %2d gadget_mul      %8.3f ms %6.2f TB/s   ratio to the copy %.3f" % (rec["shape"], batch, w, ms_g, moved / ms_g / 1e9, rec["ratio_to_copy"]))
        del a, out, src, dst
        e.close()
        torch.cuda.empty_cache()
    for lb, n, nm, batch, w in NTT:
        e = Engine(lb, n, nm)
        terms = e.decompose_terms(w)
        a = e.fill_uniform(e.empty(batch), 1, 0)
        out = e.decompose(a, w, signed=True)
        work = out.clone()
        ms_fwd = timed(lambda: e.ntt_(work), it, rp)
        del work
        ms_fused, ms_comp = timed_pair(lambda: e.decompose(a, w, signed=True, ntt=True, plan="fused", out=out),
                                       lambda: e.decompose(a, w, signed=True, ntt=True, plan="composed", out=out), it, rp)
        ms_default = timed(lambda: e.decompose(a, w, signed=True, ntt=True, out=out), it, rp)
        choice = "fused" if abs(ms_default - ms_fused) < abs(ms_default - ms_comp) else "composed"
        moved = (batch * nm * n + out.numel()) * (lb // 8)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "batch": batch, "w": w, "terms": terms, "form": "ntt", "fused_ms": round(ms_fused, 4),
               "composed_ms": round(ms_comp, 4), "composed_over_fused": round(ms_comp / ms_fused, 3), "default_ms": round(ms_default, 4),
               "dispatcher_runs": choice, "ntt_fwd_alone_ms": round(ms_fwd, 4), "fused_over_ntt_fwd": round(ms_fused / ms_fwd, 3),
               "composed_over_ntt_fwd": round(ms_comp / ms_fwd, 3), "default_TB_per_s": round(moved / ms_default / 1e9, 3),
               "polys_per_s": round(batch / ms_default * 1e3)}
        lines.append(json.dumps(rec))
        rows.append("%-12s batch %5d w %2d ntt   fused %8.3f ms  composed %8.3f ms (x%.2f)  default %8.3f ms = %s;  ntt_fwd alone on %d polys %8.3f ms (fused x%.2f, composed x%.2f)" % (
            rec["shape"], batch, w, ms_fused, ms_comp, ms_comp / ms_fused, ms_default, choice, batch * terms, ms_fwd, ms_fused / ms_fwd, ms_comp / ms_fwd))
        del a, out
        e.close()
        torch.cuda.empty_cache()
    # the pipeline a caller runs: decompose (NTT form) + the two dots of a key switch, u64/4096/4, w = 31, batch 1024
    lb, n, nm, batch, w = 64, 4096, 4, 1024, 31
    e = Engine(lb, n, nm)
    terms = e.decompose_terms(w)
    x = e.fill_uniform(e.empty(batch), 1, 0)
    K = e.fill_uniform(e.empty(2 * terms), 2, 0)                       # a key laid out [term][component], NTT-form values
    D = e.decompose(x, w, signed=True, ntt=True)
    c0, c1 = e.empty(batch), e.empty(batch)

    def pipeline():
        e.decompose(x, w, signed=True, ntt=True, out=D)
        e.dot_strided(D, (terms, 1), K.data_ptr(), (0, 2), batch, terms, out=c0)
        e.dot_strided(D, (terms, 1), K.data_ptr() + e.bytes_per_poly, (0, 2), batch, terms, out=c1)

    ms_pipe = timed(pipeline, it, rp)
    ms_dec = timed(lambda: e.decompose(x, w, signed=True, ntt=True, out=D), it, rp)
    hp = args.host_polys
    t0 = time.perf_counter()
    h = e.to_host(x[:hp])
    B, l = 1 << w, terms // nm
    digits = np.empty((hp, terms, nm, n), dtype=np.uint64)
    for m, p in enumerate(e.P):
        r = h[:, m, :].astype(object)
        r = np.where(r <= (p - 1) // 2, r, r - p)
        for t in range(l):
            d = ((r + B // 2) % B) - B // 2 if t < l - 1 else r
            r = (r - d) // B
            for m2, p2 in enumerate(e.P):
                digits[:, m * l + t, m2, :] = np.where(d < 0, d + p2, d).astype(np.uint64)
    Dh = e.ntt_(e.to_device(digits.reshape(hp * terms, nm, n)))
    e.dot_strided(Dh, (terms, 1), K.data_ptr(), (0, 2), hp, terms, out=c0[:hp])
    e.dot_strided(Dh, (terms, 1), K.data_ptr() + e.bytes_per_poly, (0, 2), hp, terms, out=c1[:hp])
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    same = bool(torch.equal(Dh, D[:hp * terms]))
    rec = {"shape": "u64/4096/4", "batch": batch, "w": w, "terms": terms, "pipeline": "decompose (NTT form) + two dots", "ms": round(ms_pipe, 4),
           "decompose_ms": round(ms_dec, 4), "polys_per_s": round(batch / ms_pipe * 1e3),
           "host_route": "download, digits in Python integers, upload, ntt_fwd, two dots", "host_polys": hp, "host_seconds": round(sec, 4),
           "host_polys_per_s": round(hp / sec, 2), "host_seconds_scaled_to_the_batch": round(sec / hp * batch, 2),
           "speedup_over_host_route": round(sec / hp * batch / (ms_pipe / 1e3)), "host_digits_equal": same}
    lines.append(json.dumps(rec))
    rows.append("u64/4096/4   batch %5d w %2d decompose (NTT) + 2 dots %8.3f ms (decompose %8.3f ms);  host digits: %d polys in %.3f s = %.1f s at this batch (x%d; same digits: %s)" % (
        batch, w, ms_pipe, ms_dec, hp, sec, sec / hp * batch, rec["speedup_over_host_route"], same))
    e.close()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/decompose_bench.py --iters %d --reps %d (MI355X): coefficient form bytes = nm rows read + the output written; "
                    "copy = hipMemcpyAsync D2D moving the same bytes; fill = hipMemsetAsync of the output's bytes\n" % (it, rp))
            f.write(text)


if __name__ == "__main__":
    main()
