#!/usr/bin/env python3
"""Time hoisted rotations (nflhip_rotate_hoisted_ntt_dev) in one run.  Per point and count the sequence plan (one key switch, one
addition and two automorphisms per rotation through the existing entries: what a caller had before this entry), the hoisted plan,
the default call and a hipMemcpyAsync device-to-device copy of the compulsory bytes are alternated block by block: --reps blocks
of --iters calls between two HIP events each, after two warm-up calls of every variant.  Reported per variant: the median of the
block means and the spread (max - min) / median of its blocks in this run.  Compulsory bytes: c0 and c1 read, 2 count L-row
polynomials written per input polynomial, every key read once.  The batch is sized to --gib of them at count 8.
est = the row-transform count of the sequence over the hoisted plan's: count (dnum nm + 2 nm) / (dnum nm + count 2 nm).

--dot times nflhip_dot_multi_dev (two groups per pass, and one with NFLHIP_DOT_UNTILED) against `outputs` calls of nflhip_dot_dev on
the same operands, at u64/4096/4 with 3 terms and a batch of 1024; compulsory bytes: a once, every b once, every output once.

usage: tools/rotate_bench.py [--dot] [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, k_special, alpha)
POINTS = [(64, 1024, 4, 1, 1), (64, 2048, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 4, 2, 2), (32, 4096, 3, 1, 1)]
COUNTS = (1, 4, 8, 16)
DOT_OUTPUTS = (2, 8, 16, 32)


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


def stats(names, ms, rec):
    for name, m in zip(names, ms):
        rec[name + "_ms"] = round(float(np.median(m)), 4)
        rec[name + "_spread"] = round(float((max(m) - min(m)) / np.median(m)), 4)


def cell(rec, name):
    return "%8.3f ms (+-%4.1f%%)" % (rec[name + "_ms"], 100 * rec[name + "_spread"])


def copier(e, nbytes):
    half = nbytes // 2 // 16 * 16
    cs, cd = (torch.empty(half, dtype=torch.uint8, device="cuda:%d" % e.device) for _ in range(2))
    st = e._stream()
    return lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))


def rotations(args):
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum * nm * row
        batch = max(int(args.gib * GIB - 8 * kbytes) // ((2 + 16) * L * row), 1)
        kept = Engine(lb, n, L)                                   # the ciphertext's ring: canonical words under the first L moduli
        c0, c1 = kept.fill_uniform(kept.empty(batch), 1, 0), kept.fill_uniform(kept.empty(batch), 2, 0)
        kept.close()
        keys = [e.fill_uniform(e.empty(2 * dnum), 3 + m, 0) for m in range(max(COUNTS))]
        for count in COUNTS:
            ks = [pow(5, m + 1, 2 * n) for m in range(count)]
            moved = batch * (2 + 2 * count) * L * row + count * kbytes
            outs = e.rotate_hoisted_ntt(c0, c1, keys[:count], ks, K, alpha, plan="sequence")
            got = e.rotate_hoisted_ntt(c0, c1, keys[:count], ks, K, alpha, plan="hoisted")
            assert all(torch.equal(g[c], o[c]) for g, o in zip(got, outs) for c in (0, 1)), (lb, n, nm, K, alpha, count)
            del got
            call = lambda plan: (lambda: e.rotate_hoisted_ntt(c0, c1, keys[:count], ks, K, alpha, outs=outs, plan=plan))      # noqa: E731
            names = ["sequence", "hoisted", "default", "copy"]
            ms = timed_alternated([call("sequence"), call("hoisted"), call(None), copier(e, moved)], args.iters, args.reps)
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "dnum": dnum, "count": count, "batch": batch,
                   "compulsory_bytes": moved}
            stats(names, ms, rec)
            for name in ("hoisted", "default"):
                rec["sequence_over_" + name] = round(rec["sequence_ms"] / rec[name + "_ms"], 3)
            rec["transform_estimate"] = round(count * (dnum * nm + 2 * nm) / (dnum * nm + count * 2 * nm), 3)
            rec["default_slower_than_sequence_beyond_spread"] = bool(
                rec["default_ms"] - rec["sequence_ms"] > max(rec["default_spread"] * rec["default_ms"], rec["sequence_spread"] * rec["sequence_ms"]))
            rec["default_ratio_to_copy"] = round(rec["copy_ms"] / rec["default_ms"], 3)
            lines.append(json.dumps(rec))
            rows.append("%-11s K=%d alpha=%d dnum=%d batch %5d count %2d  sequence %s  hoisted %s x%.3f (est x%.3f)  default %s x%.3f  copy %s" % (
                rec["shape"], K, alpha, dnum, batch, count, cell(rec, "sequence"), cell(rec, "hoisted"), rec["sequence_over_hoisted"],
                rec["transform_estimate"], cell(rec, "default"), rec["sequence_over_default"], cell(rec, "copy")))
            del outs
            torch.cuda.empty_cache()
        del c0, c1, keys
        e.close()
        torch.cuda.empty_cache()
    head = ("# tools/rotate_bench.py --iters %d --reps %d (MI355X): x = sequence / plan (above 1: the plan is faster than one key switch, one addition "
            "and two automorphisms per rotation); est = the row-transform counts' ratio; +- = (max - min) / median of the plan's blocks in this "
            "run; copy = hipMemcpyAsync D2D of the compulsory bytes (c0, c1 read, 2 count L-row polynomials written, the keys once)\n" % (args.iters, args.reps))
    return head, rows, lines


def dots(args):
    lines, rows = [], []
    lb, n, nm, terms, batch = 64, 4096, 4, 3, 1024
    e = Engine(lb, n, nm)
    pb = nm * n * (lb // 8)
    a = e.fill_uniform(e.empty(batch * terms), 1, 0)                     # [batch][terms], the layout of the inverse-transform route
    for outputs in DOT_OUTPUTS:
        keys = [e.fill_uniform(e.empty(2 * terms), 3 + m, 0) for m in range((outputs + 1) // 2)]
        bs = [keys[o // 2][o % 2:] for o in range(outputs)]              # a component of a key [term][component]: term stride 2
        outs = [e.empty(batch) for _ in range(outputs)]
        ref = [e.dot_strided(a, (terms, 1), bs[o], (0, 2), batch, terms) for o in range(outputs)]
        for untiled in (False, True):
            got = e.dot_multi(a, (terms, 1), bs, 2, batch, terms, untiled=untiled)
            assert all(torch.equal(g, r) for g, r in zip(got, ref)), (outputs, untiled)
            del got
        del ref

        def loop():
            for o in range(outputs):
                e.dot_strided(a, (terms, 1), bs[o], (0, 2), batch, terms, out=outs[o])
        moved = (batch * terms + outputs * terms + outputs * batch) * pb   # a once, b_o's terms once, the outputs
        names = ["dot_loop", "dot_multi", "dot_multi_untiled", "copy"]
        ms = timed_alternated([loop, lambda: e.dot_multi(a, (terms, 1), bs, 2, batch, terms, outs=outs),
                               lambda: e.dot_multi(a, (terms, 1), bs, 2, batch, terms, outs=outs, untiled=True), copier(e, moved)], args.iters, args.reps)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "terms": terms, "outputs": outputs, "batch": batch, "compulsory_bytes": moved}
        stats(names, ms, rec)
        for name in names[1:3]:
            rec["loop_over_" + name] = round(rec["dot_loop_ms"] / rec[name + "_ms"], 3)
        for name in names[:3]:
            rec[name + "_ratio_to_copy"] = round(rec["copy_ms"] / rec[name + "_ms"], 3)
        lines.append(json.dumps(rec))
        rows.append("%-11s terms %d batch %d outputs %2d  loop of dot %s (%.2f of copy)  dot_multi G=2 %s x%.3f (%.2f of copy)  G=1 %s x%.3f  copy %s" % (
            rec["shape"], terms, batch, outputs, cell(rec, "dot_loop"), rec["dot_loop_ratio_to_copy"], cell(rec, "dot_multi"), rec["loop_over_dot_multi"],
            rec["dot_multi_ratio_to_copy"], cell(rec, "dot_multi_untiled"), rec["loop_over_dot_multi_untiled"], cell(rec, "copy")))
        del keys, bs, outs
        torch.cuda.empty_cache()
    e.close()
    head = ("# tools/rotate_bench.py --dot --iters %d --reps %d (MI355X): x = the loop of nflhip_dot_dev / nflhip_dot_multi_dev; G = groups per pass; "
            "+- = (max - min) / median of the variant's blocks in this run; copy = hipMemcpyAsync D2D of the compulsory bytes (a once, every "
            "b and every output once)\n" % (args.iters, args.reps))
    return head, rows, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dot", action="store_true", help="time nflhip_dot_multi_dev against a loop of nflhip_dot_dev instead")
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per call at count 8 the batch is sized to")
    args = ap.parse_args()
    head, rows, lines = dots(args) if args.dot else rotations(args)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.exists(args.out) and args.dot else "w") as f:
            f.write(head)
            f.write(text)


if __name__ == "__main__":
    main()
