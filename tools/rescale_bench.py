#!/usr/bin/env python3
"""Time the RNS rescale (nflhip_rescale_dev) in one run:
  coefficient form -- bytes moved, (2 nm - 1) n words per polynomial, over time, next to a same-run hipMemcpyAsync
                      device-to-device copy that moves the same byte count (read + write);
  NTT form         -- the one-launch kernel (NFLHIP_RESCALE_FUSED) against the composed plan (NFLHIP_RESCALE_COMPOSED), what the
                      dispatcher runs by default (the nearer of the two timings names it), and the default against the sum of
                      one inverse and nm - 1 forward row transforms at the rates this run measures for ntt_ / intt_;
  context          -- lift, divide on the host, project: the only route without the entry (small batch).
Every figure: two warm-up calls, then --iters calls between two HIP events, repeated --reps times; the median is reported.

usage: tools/rescale_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per measurement)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

COEFF = [(64, 4096, 4, 16384), (64, 65536, 30, 32), (32, 4096, 3, 16384)]
NTT = [(64, 4096, 4, 16384), (64, 1024, 2, 32768), (32, 1024, 2, 32768)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    it, rp = args.iters, args.reps
    lines, rows = [], []
    for lb, n, nm, batch in COEFF:
        e = Engine(lb, n, nm)
        a = e.fill_uniform(e.empty(batch), 1, 0)
        out = torch.empty((batch, nm - 1, n), dtype=a.dtype, device=a.device)
        moved = (2 * nm - 1) * n * (lb // 8) * batch
        half = moved // 2 // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
        st = e._stream()
        ms_copy = timed(lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, dst.data_ptr(), src.data_ptr(), half, st)), it, rp)
        ms = timed(lambda: e.rescale(a, out=out), it, rp)
        tbs, ctbs = moved / ms / 1e9, 2 * half / ms_copy / 1e9
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "batch": batch, "form": "coeff", "ms": round(ms, 4), "TB_per_s": round(tbs, 3),
               "copy_ms": round(ms_copy, 4), "copy_TB_per_s": round(ctbs, 3), "ratio_to_copy": round(tbs / ctbs, 3),
               "polys_per_s": round(batch / ms * 1e3)}
        lines.append(json.dumps(rec))
        rows.append("%-14s batch %6d  coeff %9.3f ms  %6.2f TB/s   copy %9.3f ms %6.2f TB/s   ratio %.3f" % (
            rec["shape"], batch, ms, tbs, ms_copy, ctbs, tbs / ctbs))
        del a, out, src, dst
        e.close()
        torch.cuda.empty_cache()
    for lb, n, nm, batch in NTT:
        e = Engine(lb, n, nm)
        a = e.ntt_(e.fill_uniform(e.empty(batch), 1, 0))
        out = torch.empty((batch, nm - 1, n), dtype=a.dtype, device=a.device)
        work = a.clone()
        ms_fwd = timed(lambda: e.ntt_(work), it, rp) / (batch * nm)     # per row
        ms_inv = timed(lambda: e.intt_(work), it, rp) / (batch * nm)
        bound = batch * (ms_inv + (nm - 1) * ms_fwd)
        ms_fused = timed(lambda: e.rescale(a, ntt=True, out=out, fused=True), it, rp)
        ms_comp = timed(lambda: e.rescale(a, ntt=True, out=out, composed=True), it, rp)
        ms_default = timed(lambda: e.rescale(a, ntt=True, out=out), it, rp)
        choice = "fused" if abs(ms_default - ms_fused) < abs(ms_default - ms_comp) else "composed"
        moved = (2 * nm - 1) * n * (lb // 8) * batch
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "batch": batch, "form": "ntt", "fused_ms": round(ms_fused, 4),
               "composed_ms": round(ms_comp, 4), "composed_over_fused": round(ms_comp / ms_fused, 3), "default_ms": round(ms_default, 4),
               "dispatcher_runs": choice,
               "transform_sum_ms": round(bound, 4), "default_over_transform_sum": round(ms_default / bound, 3),
               "default_TB_per_s": round(moved / ms_default / 1e9, 3), "polys_per_s": round(batch / ms_default * 1e3)}
        lines.append(json.dumps(rec))
        rows.append("%-14s batch %6d  ntt   fused %8.3f ms  composed %8.3f ms (x%.2f)  default %8.3f ms = %s;  1 inv + %d fwd rows %8.3f ms (default = x%.2f)" % (
            rec["shape"], batch, ms_fused, ms_comp, ms_comp / ms_fused, ms_default, choice, nm - 1, bound, ms_default / bound))
        del a, out, work
        e.close()
        torch.cuda.empty_cache()
    # context: lift -> divide on the host (Python integers) -> project, u64/4096/4, 4 polynomials
    e, s = Engine(64, 4096, 4), Engine(64, 4096, 3)
    batch = 4
    a = e.fill_uniform(e.empty(batch), 1, 0)
    q = e.P[-1]
    h, Qp = (q - 1) // 2, e.P[0] * e.P[1] * e.P[2]
    t0 = time.perf_counter()
    limbs = e.crt_lift(a).cpu().numpy().view(np.uint64)
    L = s.crt_limbs
    res = np.zeros((batch, 4096, L), dtype=np.uint64)
    for b in range(batch):
        for j in range(4096):
            y = ((int.from_bytes(limbs[b, j].tobytes(), "little") + h) // q) % Qp
            res[b, j] = np.frombuffer(y.to_bytes(8 * L, "little"), dtype=np.uint64)
    via = s.crt_project(torch.from_numpy(res.view(np.int64)).to(a.device))
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    same = bool(torch.equal(via, e.rescale(a)))
    rec = {"shape": "u64/4096/4", "batch": batch, "route": "lift, host divide (Python integers), project", "seconds": round(sec, 4),
           "polys_per_s": round(batch / sec, 1), "equals_rescale": same}
    lines.append(json.dumps(rec))
    rows.append("u64/4096/4     batch %6d  lift -> host divide -> project %8.3f s  (%.1f polys/s; equals rescale: %s)" % (batch, sec, batch / sec, same))
    e.close()
    s.close()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/rescale_bench.py --iters %d --reps %d (MI355X): coefficient form bytes = (2 nm - 1) n words per polynomial; "
                    "copy = hipMemcpyAsync D2D moving the same bytes\n" % (it, rp))
            f.write(text)


if __name__ == "__main__":
    main()
