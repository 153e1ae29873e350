#!/usr/bin/env python3
"""Time BSGS slot linear transforms (nflhip_bsgs_ntt_dev) in one run.  Per point, level and (n1, n2) the hoisted plan, the sequence plan,
TODAY'S WAY -- one nflhip_lintrans_level_ntt_dev per giant step, one nflhip_rotate_hoisted_level_ntt_dev with count 1 per keyed giant
step, the additions: other roundings, the same function -- and a hipMemcpyAsync device-to-device copy of the compulsory bytes are
alternated block by block as tools/lintrans_bench.py does: --reps blocks of --iters calls between two HIP events each, after two
warm-up calls of every variant.  Reported per variant: the median of the block means and the spread (max - min) / median of its
blocks.  A standard BSGS: baby 0 and giant 0 are the unrotated steps, every other step is keyed; the batch is that of
tools/lintrans_bench.py.  Compulsory bytes: c0 and c1 read, out0 and out1 written, every key and every diagonal read once.
est = the row-transform counts' ratio, written down before the run: a mod-up forms dnum nm rows, a mod-down of one polynomial nm;
today's way pays (n2 + kg)(dnum nm + 2 nm), the hoisted plan dnum nm + kg (nm + dnum nm) + 2 nm, kg = n2 - 1 the keyed giants.

--mac times nflhip_automorphism_mac_multi_dev against `outputs` calls of nflhip_automorphism_mac_dev on the same inputs at u64/4096/4
with a batch of 256, terms 4 / 8 / 16 x outputs 2 / 4 / 8 / 16; compulsory bytes: every input once, every weight once, every output
once.

usage: tools/bsgs_bench.py [--mac] [--iters N] [--reps R] [--points I,J] [--out FILE]   (a table, then one line of JSON per point)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from nfllib_amd import OP_ADD, Engine  # noqa: E402
from tools.rotate_bench import GIB, POINTS, cell, copier, stats, timed_alternated  # noqa: E402

STEPS = ((4, 4), (8, 8), (16, 16), (16, 4))
MAC_TERMS, MAC_OUTPUTS = (4, 8, 16), (2, 4, 8, 16)


def transforms(args):
    lines, rows = [], []
    points = [POINTS[int(i)] for i in args.points.split(",")] if args.points else POINTS
    for lb, n, nm, K, alpha in points:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum_top = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum_top * nm * row
        keys = [e.fill_uniform(e.empty(2 * dnum_top), 3 + m, 0) for m in range(30)]
        ws = e.fill_uniform(e.empty(256), 99, 0)
        for lv in sorted({L, max(L - 1, 1)}, reverse=True):
            dnum = e.keyswitch_digits(K, alpha, lv)
            # the batch of tools/lintrans_bench.py (DESIGN.md 5.18's table), the same at every level: c0, c1 and 8 rotations' two outputs
            # each, [batch][L][n], next to 8 keys make --gib GiB
            batch = max(int(args.gib * GIB - 8 * kbytes) // ((2 + 16) * L * row), 1)
            kept = Engine(lb, n, lv)                              # the ciphertext's ring at the level
            c0, c1 = kept.fill_uniform(kept.empty(batch), 1, 0), kept.fill_uniform(kept.empty(batch), 2, 0)
            for n1, n2 in STEPS:
                bks, gks = [pow(5, i, 2 * n) for i in range(n1)], [pow(5, n1 * j, 2 * n) for j in range(n2)]
                bkeys = [None] + keys[:n1 - 1]
                gkeys = [None] + keys[15:15 + n2 - 1]
                weights = [[ws[j * n1 + i] for i in range(n1)] for j in range(n2)]
                kg, nml = n2 - 1, lv + K
                moved = batch * 4 * lv * row + (n1 + n2 - 2) * 2 * dnum * nml * row + n1 * n2 * nml * row
                out = e.bsgs_linear_transform_ntt(c0, c1, bkeys, bks, gkeys, gks, weights, K, alpha, plan="sequence", level=lv)
                got = e.bsgs_linear_transform_ntt(c0, c1, bkeys, bks, gkeys, gks, weights, K, alpha, plan="hoisted", level=lv)
                assert torch.equal(got[0], out[0]) and torch.equal(got[1], out[1]), (lb, n, nm, K, alpha, lv, n1, n2)
                del got
                t, r, acc = (torch.empty((2, batch, lv, n), dtype=e.torch_dtype, device=c1.device) for _ in range(3))

                def previous():
                    for j in range(n2):
                        e.linear_transform_ntt(c0, c1, bkeys, weights[j], bks, K, alpha, out=(t[0], t[1]), level=lv)
                        src = t
                        if gkeys[j] is not None:
                            e.rotate_hoisted_ntt(t[0], t[1], [gkeys[j]], [gks[j]], K, alpha, outs=[(r[0], r[1])], level=lv)
                            src = r
                        if j:
                            kept.pointwise(OP_ADD, acc.view(2 * batch, lv, n), src.view(2 * batch, lv, n), out=acc.view(2 * batch, lv, n))
                        else:
                            acc.copy_(src)
                call = lambda plan: (lambda: e.bsgs_linear_transform_ntt(c0, c1, bkeys, bks, gkeys, gks, weights, K, alpha, out=out, plan=plan, level=lv))  # noqa: E731
                names = ["hoisted", "sequence", "previous", "copy"]
                ms = timed_alternated([call("hoisted"), call("sequence"), previous, copier(e, moved)], args.iters, args.reps)
                rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "level": lv, "dnum": dnum, "n1": n1, "n2": n2, "batch": batch,
                       "compulsory_bytes": moved}
                stats(names, ms, rec)
                rec["previous_over_hoisted"] = round(rec["previous_ms"] / rec["hoisted_ms"], 3)
                rec["sequence_over_hoisted"] = round(rec["sequence_ms"] / rec["hoisted_ms"], 3)
                rec["transform_estimate"] = round((n2 + kg) * (dnum * nml + 2 * nml) / (dnum * nml + kg * (nml + dnum * nml) + 2 * nml), 3)
                rec["hoisted_ratio_to_copy"] = round(rec["copy_ms"] / rec["hoisted_ms"], 3)
                lines.append(json.dumps(rec))
                rows.append("%-11s K=%d alpha=%d level %d dnum=%d batch %5d (n1, n2) (%2d, %2d)  previous %s  hoisted %s x%.3f (est x%.3f)  sequence %s (x%.3f of hoisted)  copy %s" % (
                    rec["shape"], K, alpha, lv, dnum, batch, n1, n2, cell(rec, "previous"), cell(rec, "hoisted"), rec["previous_over_hoisted"],
                    rec["transform_estimate"], cell(rec, "sequence"), rec["sequence_over_hoisted"], cell(rec, "copy")))
                sys.stderr.write(rows[-1] + "\n")
                del out, t, r, acc
                torch.cuda.empty_cache()
            del c0, c1
            kept.close()
        del keys, ws
        e.close()
        torch.cuda.empty_cache()
    head = ("# tools/bsgs_bench.py --iters %d --reps %d (%s): x = today's way / hoisted (above 1: the BSGS entry is faster than a linear "
            "transform per giant step, a keyed rotation of each and the additions); est = the row-transform counts' ratio; +- = (max - min) / "
            "median of the variant's blocks in this run; copy = hipMemcpyAsync D2D of the compulsory bytes\n" % (args.iters, args.reps, torch.cuda.get_device_name(0)))
    return head, rows, lines


def macs(args):
    lines, rows = [], []
    lb, n, nm, batch = 64, 4096, 4, 256
    e = Engine(lb, n, nm)
    pb = nm * n * (lb // 8)
    ws = e.fill_uniform(e.empty(max(MAC_TERMS) * max(MAC_OUTPUTS)), 77, 0)
    for terms in MAC_TERMS:
        ins = [e.fill_uniform(e.empty(batch), 1 + t, 0) for t in range(terms)]
        ks = [pow(5, t + 1, 2 * n) for t in range(terms)]
        for outputs in MAC_OUTPUTS:
            weights = [[ws[o * terms + t] for t in range(terms)] for o in range(outputs)]
            outs, refs = [e.empty(batch) for _ in range(outputs)], [e.empty(batch) for _ in range(outputs)]

            def loop():
                for o in range(outputs):
                    e.automorphism_mac(ins, weights[o], ks, out=refs[o])
            loop()
            e.automorphism_mac_multi(ins, weights, ks, outs=outs)
            assert all(torch.equal(a, b) for a, b in zip(outs, refs)), (terms, outputs)
            moved = (terms * batch + terms * outputs + outputs * batch) * pb
            names = ["loop", "multi", "copy"]
            ms = timed_alternated([loop, lambda: e.automorphism_mac_multi(ins, weights, ks, outs=outs), copier(e, moved)], args.iters, args.reps)
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "terms": terms, "outputs": outputs, "batch": batch, "compulsory_bytes": moved}
            stats(names, ms, rec)
            rec["loop_over_multi"] = round(rec["loop_ms"] / rec["multi_ms"], 3)
            for name in names[:2]:
                rec[name + "_ratio_to_copy"] = round(rec["copy_ms"] / rec[name + "_ms"], 3)
            rec["multi_wins_beyond_spread"] = bool(
                rec["loop_ms"] - rec["multi_ms"] > max(rec["loop_spread"] * rec["loop_ms"], rec["multi_spread"] * rec["multi_ms"]))
            lines.append(json.dumps(rec))
            rows.append("%-11s batch %d terms %2d outputs %2d  loop of automorphism_mac %s (%.2f of copy)  several outputs %s x%.3f (%.2f of copy)  copy %s" % (
                rec["shape"], batch, terms, outputs, cell(rec, "loop"), rec["loop_ratio_to_copy"], cell(rec, "multi"), rec["loop_over_multi"],
                rec["multi_ratio_to_copy"], cell(rec, "copy")))
            sys.stderr.write(rows[-1] + "\n")
            del outs, refs
            torch.cuda.empty_cache()
        del ins
    e.close()
    head = ("# tools/bsgs_bench.py --mac --iters %d --reps %d (%s): x = `outputs` calls of nflhip_automorphism_mac_dev / one call of "
            "nflhip_automorphism_mac_multi_dev (the library's NFLHIP_MAC_MULTI_JB outputs per launch); +- = (max - min) / median of the variant's blocks in this run; copy = "
            "hipMemcpyAsync D2D of the compulsory bytes (every input, every weight and every output once)\n" % (args.iters, args.reps, torch.cuda.get_device_name(0)))
    return head, rows, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mac", action="store_true", help="time nflhip_automorphism_mac_multi_dev against a loop of nflhip_automorphism_mac_dev instead")
    ap.add_argument("--points", default=None, help="indices into tools/rotate_bench.py POINTS, comma-separated (default: all)")
    ap.add_argument("--gib", type=float, default=1.0, help="sizes the batch as tools/lintrans_bench.py sizes it: GiB of compulsory traffic of a hoisted rotation call at count 8")
    args = ap.parse_args()
    head, rows, lines = macs(args) if args.mac else transforms(args)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.exists(args.out) else "w") as f:
            f.write(head)
            f.write(text)


if __name__ == "__main__":
    main()
