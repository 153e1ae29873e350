#!/usr/bin/env python3
"""Time slot linear transforms (nflhip_lintrans_ntt_dev) in one run.  Per point and count the sequence plan (the definition through
the existing entries), the hoisted plan, the default call, the PREVIOUS way -- nflhip_rotate_hoisted_ntt_dev (its default plan)
followed by two nflhip_dot_dev over the rotations: a different rounding, the same function -- and a hipMemcpyAsync device-to-device
copy of the compulsory bytes are alternated block by block: --reps blocks of --iters calls between two HIP events each, after two
warm-up calls of every variant.  Reported per variant: the median of the block means and the spread (max - min) / median of its
blocks in this run.  Compulsory bytes: c0 and c1 read, out0 and out1 written, every key and every diagonal read once.  The batch is
that of tools/rotate_bench.py (1 GiB of a hoisted rotation's compulsory traffic at count 8).  Every term is keyed.
est = the row-transform count of the previous way over the hoisted plan's: (dnum nm + count 2 nm) / (dnum nm + 2 nm).

--mac times nflhip_automorphism_mac_dev (one staging buffer, and two with NFLHIP_MAC_DOUBLE_BUFFER) against `terms` calls of
nflhip_automorphism_dev + nflhip_dot_dev (one term, the addend in place) on the same operands, at u64/4096/4 with a batch of 256;
compulsory bytes: every input once, every weight once, the output once.

usage: tools/lintrans_bench.py [--mac] [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402
from tools.rotate_bench import GIB, POINTS, cell, copier, stats, timed_alternated  # noqa: E402

COUNTS = (1, 2, 4, 8, 16)   # (1 and 2 for the default's rule: with one keyed term it is the sequence)
MAC_TERMS = (2, 4, 8, 16)


def transforms(args):
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum * nm * row
        batch = max(int(args.gib * GIB - 8 * kbytes) // ((2 + 16) * L * row), 1)
        kept = Engine(lb, n, L)                                   # the ciphertext's ring: canonical words under the first L moduli
        c0, c1 = kept.fill_uniform(kept.empty(batch), 1, 0), kept.fill_uniform(kept.empty(batch), 2, 0)
        keys = [e.fill_uniform(e.empty(2 * dnum), 3 + m, 0) for m in range(max(COUNTS))]
        ws = e.fill_uniform(e.empty(max(COUNTS)), 99, 0)          # the diagonals over all nm moduli ...
        wk = ws[:, :L].contiguous()                               # ... and their kept rows, dense, for the previous way's dots
        for count in COUNTS:
            ks = [pow(5, m + 1, 2 * n) for m in range(count)]
            moved = batch * 4 * L * row + count * (kbytes + nm * row)
            out = e.linear_transform_ntt(c0, c1, keys[:count], list(ws[:count]), ks, K, alpha, plan="sequence")
            got = e.linear_transform_ntt(c0, c1, keys[:count], list(ws[:count]), ks, K, alpha, plan="hoisted")
            assert torch.equal(got[0], out[0]) and torch.equal(got[1], out[1]), (lb, n, nm, K, alpha, count)
            del got
            rot = torch.empty((count, 2, batch, L, n), dtype=e.torch_dtype, device=c1.device)
            routs = [(rot[m, 0], rot[m, 1]) for m in range(count)]
            pout = torch.empty((2, batch, L, n), dtype=e.torch_dtype, device=c1.device)

            def previous():
                e.rotate_hoisted_ntt(c0, c1, keys[:count], ks, K, alpha, outs=routs)
                for c in (0, 1):
                    kept.dot_strided(rot[0, c], (1, 2 * batch), wk, (0, 1), batch, count, out=pout[c])
            call = lambda plan: (lambda: e.linear_transform_ntt(c0, c1, keys[:count], list(ws[:count]), ks, K, alpha, out=out, plan=plan))      # noqa: E731
            names = ["sequence", "hoisted", "default", "previous", "copy"]
            ms = timed_alternated([call("sequence"), call("hoisted"), call(None), previous, copier(e, moved)], args.iters, args.reps)
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "dnum": dnum, "count": count, "batch": batch,
                   "compulsory_bytes": moved}
            stats(names, ms, rec)
            for name in ("sequence", "hoisted", "default"):
                rec["previous_over_" + name] = round(rec["previous_ms"] / rec[name + "_ms"], 3)
            rec["transform_estimate"] = round((dnum * nm + count * 2 * nm) / (dnum * nm + 2 * nm), 3)
            rec["default_slower_than_previous_beyond_spread"] = bool(
                rec["default_ms"] - rec["previous_ms"] > max(rec["default_spread"] * rec["default_ms"], rec["previous_spread"] * rec["previous_ms"]))
            rec["default_ratio_to_copy"] = round(rec["copy_ms"] / rec["default_ms"], 3)
            lines.append(json.dumps(rec))
            rows.append("%-11s K=%d alpha=%d dnum=%d batch %5d count %2d  previous %s  sequence %s x%.3f  hoisted %s x%.3f (est x%.3f)  default %s x%.3f  copy %s" % (
                rec["shape"], K, alpha, dnum, batch, count, cell(rec, "previous"), cell(rec, "sequence"), rec["previous_over_sequence"],
                cell(rec, "hoisted"), rec["previous_over_hoisted"], rec["transform_estimate"], cell(rec, "default"), rec["previous_over_default"],
                cell(rec, "copy")))
            del out, rot, routs, pout
            torch.cuda.empty_cache()
        del c0, c1, keys, ws, wk
        kept.close()
        e.close()
        torch.cuda.empty_cache()
    head = ("# tools/lintrans_bench.py --iters %d --reps %d (MI355X): x = previous / plan (above 1: the plan is faster than the hoisted rotations "
            "followed by two sums of products); est = the row-transform counts' ratio; +- = (max - min) / median of the plan's blocks in this "
            "run; copy = hipMemcpyAsync D2D of the compulsory bytes (c0, c1 read, out0, out1 written, the keys and the diagonals once)\n" % (args.iters, args.reps))
    return head, rows, lines


def macs(args):
    lines, rows = [], []
    lb, n, nm, batch = 64, 4096, 4, 256
    e = Engine(lb, n, nm)
    pb = nm * n * (lb // 8)
    for terms in MAC_TERMS:
        ins = [e.fill_uniform(e.empty(batch), 1 + t, 0) for t in range(terms)]
        ws = e.fill_uniform(e.empty(terms), 77, 0)
        ks = [pow(5, t + 1, 2 * n) for t in range(terms)]
        out, tmp = e.empty(batch), e.empty(batch)

        def loop():
            for t in range(terms):
                e.automorphism(ins[t], ks[t], ntt=True, out=tmp)
                e.dot_strided(tmp, (1, 0), ws[t], (0, 0), batch, 1, addend=out if t else None, out=out)
        loop()
        ref = out.clone()
        for double in (False, True):
            assert torch.equal(e.automorphism_mac(ins, list(ws), ks, double_buffer=double), ref), (terms, double)
        moved = (terms * batch + terms + batch) * pb
        names = ["loop", "mac", "mac_double", "copy"]
        ms = timed_alternated([loop, lambda: e.automorphism_mac(ins, list(ws), ks, out=out),
                               lambda: e.automorphism_mac(ins, list(ws), ks, out=out, double_buffer=True), copier(e, moved)], args.iters, args.reps)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "terms": terms, "batch": batch, "compulsory_bytes": moved}
        stats(names, ms, rec)
        for name in names[1:3]:
            rec["loop_over_" + name] = round(rec["loop_ms"] / rec[name + "_ms"], 3)
        for name in names[:3]:
            rec[name + "_ratio_to_copy"] = round(rec["copy_ms"] / rec[name + "_ms"], 3)
        rec["double_over_single"] = round(rec["mac_double_ms"] / rec["mac_ms"], 3)
        lines.append(json.dumps(rec))
        rows.append("%-11s batch %d terms %2d  loop of automorphism + dot %s (%.2f of copy)  mac, one buffer %s x%.3f (%.2f of copy)  two buffers %s x%.3f (%.2f of copy)  copy %s" % (
            rec["shape"], batch, terms, cell(rec, "loop"), rec["loop_ratio_to_copy"], cell(rec, "mac"), rec["loop_over_mac"], rec["mac_ratio_to_copy"],
            cell(rec, "mac_double"), rec["loop_over_mac_double"], rec["mac_double_ratio_to_copy"], cell(rec, "copy")))
        del ins, ws, out, tmp, ref
        torch.cuda.empty_cache()
    e.close()
    head = ("# tools/lintrans_bench.py --mac --iters %d --reps %d (MI355X): x = the loop of nflhip_automorphism_dev + nflhip_dot_dev / "
            "nflhip_automorphism_mac_dev; +- = (max - min) / median of the variant's blocks in this run; copy = hipMemcpyAsync D2D of the "
            "compulsory bytes (every input, every weight and the output once)\n" % (args.iters, args.reps))
    return head, rows, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mac", action="store_true", help="time nflhip_automorphism_mac_dev against a loop of nflhip_automorphism_dev + nflhip_dot_dev instead")
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per hoisted rotation call at count 8 the batch is sized to")
    args = ap.parse_args()
    head, rows, lines = macs(args) if args.mac else transforms(args)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.exists(args.out) and args.mac else "w") as f:
            f.write(head)
            f.write(text)


if __name__ == "__main__":
    main()
