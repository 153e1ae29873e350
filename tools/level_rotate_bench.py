#!/usr/bin/env python3
"""Time hoisted rotations and slot linear transforms BELOW the top level (nflhip_rotate_hoisted_level_ntt_dev,
nflhip_lintrans_level_ntt_dev) in one run.  Per point, level l and count (rotations / terms), for each of the two entries (default
plan, fast mode, rounding), the calls are alternated block by block -- --reps blocks of --iters calls between two HIP events each,
after two warm-up calls of every variant:
  (a)   the level call on the parent context with the ONE top-level Galois key per rotation and the ONE top-level diagonal per term;
  (b)   the existing entry on the explicit context over the live rows (Engine.level_engine) with pre-gathered keys and diagonals:
        entries and kernel instances this change does not touch, so the speed of the code before it;
  (b2)  (b) once more on a SECOND explicit context over the same moduli with its own copies of the gathered keys and diagonals: the
        same code and the same data as (b) in other allocations, so b2 / b is what two contexts differ by at this very cell;
  top   the existing entry at the top level on the same batch, so that the scaling with l is on the page;
  comp  (rotations only) what a user had before: per rotation the level key switch of c1, the addition of c0 and automorphism on the
        l-row engine of both components -- no shared mod-up, one dot and one mod-down per rotation.
(a), (b) and (b2) are asserted equal, word for word, before anything is timed; comp is asserted equal to (a) as well.  Reported per
variant: the median of the block means and the spread (max - min) / median of its blocks in this run; a / b above 1 means the level
call is slower than (b), and `within` says whether a / b - 1 is inside the largest of the two block spreads and |b2 / b - 1|.  The batch
is sized to about 1 GiB of compulsory traffic per call at the level (c0 and c1 read, 2 count [rotations] or 2 [transform] results
written, the live rows and digits of every key and diagonal once).  Also per point: the bytes of Galois-key memory a compacted copy
per level of ONE key would need, sum_l dnum_l 2 (l + K) n words, against the one key.

usage: tools/level_rotate_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point, level and count)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine, _lib  # noqa: E402
from level_bench import timed_alternated, uniform  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, k_special, alpha), every level of each
POINTS = [(64, 1024, 4, 1, 1), (64, 2048, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 6, 2, 2)]
COUNTS = (4, 16)


def same(x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


def flat(outs):
    return [t for pair in outs for t in pair]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per call the batch is sized to")
    ap.add_argument("--points", type=int, default=len(POINTS), help="only the first N points")
    args = ap.parse_args()
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS[:args.points]:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        keys = [e.fill_uniform(e.empty(2 * dnum), 10 + m, 0).view(dnum, 2, nm, n) for m in range(max(COUNTS))]
        ws = [e.fill_uniform(e.empty(1), 40 + m, 0).view(nm, n) for m in range(max(COUNTS))]
        one_key = 2 * dnum * nm * row
        per_level = sum(2 * e.keyswitch_digits(K, alpha, level=lv) * (lv + K) * row for lv in range(1, L + 1))
        rows.append("%-11s K=%d alpha=%d: one Galois key %d bytes; a compacted copy per level %d bytes (x%.2f); one diagonal %d bytes, per level %d (x%.2f)" % (
            "u%d/%d/%d" % (lb, n, nm), K, alpha, one_key, per_level, per_level / one_key, nm * row, sum((lv + K) * row for lv in range(1, L + 1)),
            sum(lv + K for lv in range(1, L + 1)) / nm))
        for level in range(1, L + 1):
            dl = e.keyswitch_digits(K, alpha, level=level)
            al = min(alpha, level)
            live = e.level_rows(level, K)
            c, c2, ring = e.level_engine(level, K), e.level_engine(level, K), Engine(lb, n, level)
            gk = [k[:dl][:, :, live].contiguous() for k in keys]
            gw = [w[live].contiguous() for w in ws]
            gk2, gw2 = [k.clone() for k in gk], [w.clone() for w in gw]
            for count in COUNTS:
                ks = [(2 * i + 3) % (2 * n) for i in range(count)]
                rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "level": level, "dnum_level": dl, "count": count,
                       "one_key_bytes": one_key, "per_level_copies_bytes": per_level}
                for name in ("rotate", "lintrans"):
                    nout = 2 * count if name == "rotate" else 2
                    kbytes = count * (2 * dl * (level + K) * row + (0 if name == "rotate" else (level + K) * row))
                    batch = max(int(args.gib * GIB - kbytes) // ((2 + nout) * level * row), 1)
                    a0, a1 = uniform(lb, n, level, batch, (1, 2))
                    t0, t1 = uniform(lb, n, L, batch, (1, 2))
                    rec[name + "_batch"] = batch
                    if name == "rotate":
                        fa = lambda outs=None: e.rotate_hoisted_ntt(a0, a1, keys[:count], ks, K, alpha, outs=outs, level=level)       # noqa: E731
                        fb = lambda outs=None: c.rotate_hoisted_ntt(a0, a1, gk[:count], ks, K, al, outs=outs)                           # noqa: E731
                        f2 = lambda outs=None: c2.rotate_hoisted_ntt(a0, a1, gk2[:count], ks, K, al, outs=outs)                         # noqa: E731
                        ft = lambda outs=None: e.rotate_hoisted_ntt(t0, t1, keys[:count], ks, K, alpha, outs=outs)                      # noqa: E731
                        sw = torch.empty((2,) + tuple(a1.shape), dtype=a1.dtype, device=a1.device)

                        def fc(outs=None):
                            outs = outs or [(torch.empty_like(a1), torch.empty_like(a1)) for _ in ks]
                            for m, k in enumerate(ks):
                                e.key_switch_ntt(a1, keys[m], K, alpha, out=(sw[0], sw[1]), level=level)
                                ring.pointwise(_lib.OP_ADD, sw[0], a0, out=sw[0])
                                ring.automorphism(sw[0], k, ntt=True, out=outs[m][0])
                                ring.automorphism(sw[1], k, ntt=True, out=outs[m][1])
                            return outs
                        variants, fns = ("a", "b", "b2", "top", "comp"), (fa, fb, f2, ft, fc)
                        outs = [f() for f in fns]
                        assert same(flat(outs[0]), flat(outs[1])) and same(flat(outs[2]), flat(outs[1])), (lb, n, nm, K, alpha, level, count, name)
                        assert same(flat(outs[4]), flat(outs[0])), (lb, n, nm, K, alpha, level, count, "composition")
                    else:
                        fa = lambda out=None: e.linear_transform_ntt(a0, a1, keys[:count], ws[:count], ks, K, alpha, out=out, level=level)   # noqa: E731
                        fb = lambda out=None: c.linear_transform_ntt(a0, a1, gk[:count], gw[:count], ks, K, al, out=out)                       # noqa: E731
                        f2 = lambda out=None: c2.linear_transform_ntt(a0, a1, gk2[:count], gw2[:count], ks, K, al, out=out)                    # noqa: E731
                        ft = lambda out=None: e.linear_transform_ntt(t0, t1, keys[:count], ws[:count], ks, K, alpha, out=out)                  # noqa: E731
                        variants, fns = ("a", "b", "b2", "top"), (fa, fb, f2, ft)
                        outs = [f() for f in fns]
                        assert same(outs[0], outs[1]) and same(outs[2], outs[1]), (lb, n, nm, K, alpha, level, count, name)
                    ms = timed_alternated([(lambda f=f, o=o: f(o)) for f, o in zip(fns, outs)], args.iters, args.reps)
                    med = [float(np.median(m)) for m in ms]
                    spread = [float((max(m) - min(m)) / np.median(m)) for m in ms]
                    for v, m_, s_ in zip(variants, med, spread):
                        rec["%s_%s_ms" % (name, v)], rec["%s_%s_spread" % (name, v)] = round(m_, 4), round(s_, 4)
                    rec[name + "_a_over_b"] = round(med[0] / med[1], 4)
                    rec[name + "_b2_over_b"] = round(med[2] / med[1], 4)
                    rec[name + "_within_band"] = bool(med[0] / med[1] - 1 <= max(spread[0], spread[1], abs(med[2] / med[1] - 1)))
                    if name == "rotate":
                        rec["rotate_comp_over_a"] = round(med[4] / med[0], 4)
                    del outs, a0, a1, t0, t1
                    torch.cuda.empty_cache()
                lines.append(json.dumps(rec))
                cell = lambda nm_, v: "%8.3f ms (+-%4.1f%%)" % (rec["%s_%s_ms" % (nm_, v)], 100 * rec["%s_%s_spread" % (nm_, v)])   # noqa: E731
                for name in ("rotate", "lintrans"):
                    rows.append("%-11s K=%d alpha=%d l=%d dnum_l=%d count %2d batch %5d  %-8s (a) %s  (b) %s  a/b x%.3f %-12s (b2) %s b2/b x%.3f  top %s%s" % (
                        rec["shape"], K, alpha, level, dl, count, rec[name + "_batch"], name, cell(name, "a"), cell(name, "b"), rec[name + "_a_over_b"],
                        "within band" if rec[name + "_within_band"] else "OUTSIDE BAND", cell(name, "b2"), rec[name + "_b2_over_b"], cell(name, "top"),
                        "  comp %s comp/a x%.2f" % (cell(name, "comp"), rec["rotate_comp_over_a"]) if name == "rotate" else ""))
                    print(rows[-1], file=sys.stderr, flush=True)   # (progress: the table itself goes to stdout at the end)
            del gk, gw, gk2, gw2
            c.close(), c2.close(), ring.close()
            torch.cuda.empty_cache()
        del keys, ws
        e.close()
        torch.cuda.empty_cache()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/level_rotate_bench.py --iters %d --reps %d (MI355X): (a) the level call on the parent context with the one top-level key per "
                    "rotation and the one top-level diagonal per term; (b) the existing entry on the explicit level context with pre-gathered keys and "
                    "diagonals; (b2) the same as (b) on a second such context with its own copies; top = the existing entry at the top level, same "
                    "batch; comp = per rotation the level key switch + addition + two automorphisms; +- = (max - min) / median of the variant's blocks "
                    "in this run; a/b above 1: (a) is slower; band = the largest of the two block spreads and |b2/b - 1|\n" % (args.iters, args.reps))
            f.write(text)


if __name__ == "__main__":
    main()
