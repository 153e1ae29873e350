#!/usr/bin/env python3
"""Time key switching and multiplication BELOW the top level (nflhip_keyswitch_level_ntt_dev, nflhip_mulrelin_level_ntt_dev) in one
run.  Per point and level l, for each of the two entries (default plan, fast mode, rounding, no rescale), four calls are alternated
block by block -- --reps blocks of --iters calls between two HIP events each, after two warm-up calls of every variant:
  (a)   the level call on the parent context with the ONE top-level key;
  (b)   the existing entry on the explicit context over the live rows (Engine.level_engine) with a pre-gathered key: entries this
        change does not touch, so the speed of the code before it;
  (b2)  (b) once more on a SECOND explicit context over the same moduli with its own copy of the gathered key: the same code and the
        same data as (b) in other allocations, so b2 / b is what two contexts differ by at this very cell with no change at all;
  top   the existing entry at the top level on the same batch, so that the scaling with l is on the page.
(a), (b) and (b2) are asserted equal, word for word, before anything is timed.  Reported per variant: the median of the block means and
the spread (max - min) / median of its blocks in this run; a / b above 1 means the level call is slower than (b), and `within` says
whether that is inside the larger block spread of the two.  The batch is sized to about 1 GiB of the key switch's compulsory traffic
at the level (l rows read, 2 l written, the live key once).  Also per point: the bytes of key memory a per-level copy of ONE key would
need, sum_l dnum_l 2 (l + K) n words, against the one key.

usage: tools/level_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point and level)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, k_special, alpha), every level of each
POINTS = [(64, 1024, 4, 1, 1), (64, 2048, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 6, 2, 2)]


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


def uniform(lb, n, rows, batch, seeds):
    """canonical words under the first `rows` moduli: one [batch, rows, n] tensor per seed"""
    ring = Engine(lb, n, rows)
    out = [ring.fill_uniform(ring.empty(batch), s, 0) for s in seeds]
    ring.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per key switch the batch is sized to")
    args = ap.parse_args()
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        key = e.fill_uniform(e.empty(2 * dnum), 2, 0).view(dnum, 2, nm, n)
        one_key = 2 * dnum * nm * row
        per_level = sum(2 * e.keyswitch_digits(K, alpha, level=lv) * (lv + K) * row for lv in range(1, L + 1))
        rows.append("%-11s K=%d alpha=%d: one key %d bytes; a compacted copy per level %d bytes (x%.2f)" % (
            "u%d/%d/%d" % (lb, n, nm), K, alpha, one_key, per_level, per_level / one_key))
        for level in range(1, L + 1):
            dl = e.keyswitch_digits(K, alpha, level=level)
            kbytes = 2 * dl * (level + K) * row
            batch = max(int(args.gib * GIB - kbytes) // (3 * level * row), 1)
            c, c2 = e.level_engine(level, K), e.level_engine(level, K)
            gkey = key[:dl][:, :, e.level_rows(level, K)].contiguous()
            gkey2 = gkey.clone()
            a = uniform(lb, n, level, batch, (1, 2, 3, 4))
            t = uniform(lb, n, L, batch, (1, 2, 3, 4))
            al = min(alpha, level)
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "level": level, "dnum_level": dl, "batch": batch,
                   "one_key_bytes": one_key, "per_level_copies_bytes": per_level}
            for name in ("keyswitch", "mulrelin"):
                if name == "keyswitch":
                    fa = lambda out=None: e.key_switch_ntt(a[1], key, K, alpha, out=out, level=level)          # noqa: E731
                    fb = lambda out=None: c.key_switch_ntt(a[1], gkey, K, al, out=out)                           # noqa: E731
                    f2 = lambda out=None: c2.key_switch_ntt(a[1], gkey2, K, al, out=out)                         # noqa: E731
                    ft = lambda out=None: e.key_switch_ntt(t[1], key, K, alpha, out=out)                          # noqa: E731
                else:
                    fa = lambda out=None: e.mul_relin_ntt(a[0], a[1], a[2], a[3], key, K, alpha, out=out, level=level)   # noqa: E731
                    fb = lambda out=None: c.mul_relin_ntt(a[0], a[1], a[2], a[3], gkey, K, al, out=out)                    # noqa: E731
                    f2 = lambda out=None: c2.mul_relin_ntt(a[0], a[1], a[2], a[3], gkey2, K, al, out=out)                  # noqa: E731
                    ft = lambda out=None: e.mul_relin_ntt(t[0], t[1], t[2], t[3], key, K, alpha, out=out)                   # noqa: E731
                oa, ob, o2, ot = fa(), fb(), f2(), ft()
                assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1]), (lb, n, nm, K, alpha, level, name)
                assert torch.equal(o2[0], ob[0]) and torch.equal(o2[1], ob[1]), (lb, n, nm, K, alpha, level, name)
                ms = timed_alternated([lambda: fa(oa), lambda: fb(ob), lambda: f2(o2), lambda: ft(ot)], args.iters, args.reps)
                med = [float(np.median(m)) for m in ms]
                spread = [float((max(m) - min(m)) / np.median(m)) for m in ms]
                for v, m_, s_ in zip(("a", "b", "b2", "top"), med, spread):
                    rec["%s_%s_ms" % (name, v)], rec["%s_%s_spread" % (name, v)] = round(m_, 4), round(s_, 4)
                rec[name + "_a_over_b"] = round(med[0] / med[1], 4)
                rec[name + "_within_spread"] = bool(med[0] / med[1] - 1 <= max(spread[0], spread[1]))
                rec[name + "_b2_over_b"] = round(med[2] / med[1], 4)
                del oa, ob, o2, ot
            lines.append(json.dumps(rec))
            cell = lambda nm_, v: "%8.3f ms (+-%4.1f%%)" % (rec["%s_%s_ms" % (nm_, v)], 100 * rec["%s_%s_spread" % (nm_, v)])   # noqa: E731
            for name in ("keyswitch", "mulrelin"):
                rows.append("%-11s K=%d alpha=%d l=%d dnum_l=%d batch %6d  %-9s (a) %s  (b) %s  a/b x%.3f %-14s (b2) %s b2/b x%.3f  top %s" % (
                    rec["shape"], K, alpha, level, dl, batch, name, cell(name, "a"), cell(name, "b"), rec[name + "_a_over_b"],
                    "within spread" if rec[name + "_within_spread"] else "OUTSIDE SPREAD", cell(name, "b2"), rec[name + "_b2_over_b"],
                    cell(name, "top")))
            del a, t, gkey, gkey2
            c.close()
            c2.close()
            torch.cuda.empty_cache()
        del key
        e.close()
        torch.cuda.empty_cache()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/level_bench.py --iters %d --reps %d (MI355X): (a) the level call on the parent context with the one top-level key; (b) the "
                    "existing entry on the explicit level context with a pre-gathered key; (b2) the same as (b) on a second such context with its own copy of the key; "
                    "top = the existing entry at the top level, same batch; "
                    "+- = (max - min) / median of the variant's blocks in this run; a/b above 1: (a) is slower\n" % (args.iters, args.reps))
            f.write(text)


if __name__ == "__main__":
    main()
