#!/usr/bin/env python3
"""Time the ciphertext multiplication with relinearisation (nflhip_mulrelin_ntt_dev) in one run.  Per point and per case -- general or
square, without or with the rescale -- the plans (sequence, merged, fused where it fits), the default call, PREV and a hipMemcpyAsync
device-to-device copy of the compulsory bytes are alternated block by block: --reps blocks of --iters calls between two HIP events
each, after two warm-up calls of every variant.  PREV is what a caller had before this entry, through entries that did not change:
the tensor product by nflhip_pointwise_dev and a two-term nflhip_dot_dev (the square: three products and a doubling), the key switch
of the third component at its default plan, two element-wise additions and, with the rescale, two nflhip_rescale_dev calls.
Reported per variant: the median of the block means and the spread (max - min) / median of its blocks in this run.  Compulsory bytes:
4 L rows read (2 L for the square), 2 L (or 2 (L - 1)) rows written, the key read once.

usage: tools/mulrelin_bench.py [--iters N] [--reps R] [--out FILE]   (a table, then one line of JSON per point and case)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine, NflHipError  # noqa: E402
from nfllib_amd._lib import ERR_UNSUPPORTED, OP_ADD, OP_MUL  # noqa: E402

GIB = 1 << 30
# (limb bits, degree, moduli, k_special, alpha): the points of tools/keyswitch_bench.py; batch sized to about --gib of compulsory traffic
POINTS = [(64, 1024, 4, 1, 1), (64, 1024, 4, 1, 3), (64, 2048, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 4, 2, 2), (32, 4096, 3, 1, 1)]
PLANS = ("sequence", "merged", "fused")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per call the batch is sized to")
    args = ap.parse_args()
    lines, rows = [], []
    for lb, n, nm, K, alpha in POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        dnum = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum * nm * row
        batch = max(int(args.gib * GIB - kbytes) // (6 * L * row), 1)
        kept = Engine(lb, n, L)                                   # the ciphertexts' ring: canonical words under the first L moduli
        A = kept.fill_uniform(kept.empty(2 * batch), 1, 0).view(2, batch, L, n)          # (a0, a1)
        Bx = kept.fill_uniform(kept.empty(2 * batch), 2, 0).view(2, batch, L, n)         # (b1, b0): the cross term as one two-term dot
        a0, a1, b1, b0 = A[0], A[1], Bx[0], Bx[1]
        key = e.fill_uniform(e.empty(2 * dnum), 3, 0)
        d = kept.empty(3 * batch).view(3, batch, L, n)
        ks = kept.empty(2 * batch).view(2, batch, L, n)
        st = e._stream()
        for square in (False, True):
            for rescale in (False, True):
                R = L - 1 if rescale else L
                moved = batch * ((2 if square else 4) * L + 2 * R) * row + kbytes
                out = torch.empty((2, batch, R, n), dtype=e.torch_dtype, device=a0.device)
                sums = kept.empty(2 * batch).view(2, batch, L, n) if rescale else out
                bb = (None, None) if square else (b0, b1)
                ref = e.mul_relin_ntt(a0, a1, bb[0], bb[1], key, K, alpha, rescale=rescale, plan="sequence")
                plans = []
                for p in PLANS:
                    try:
                        got = e.mul_relin_ntt(a0, a1, bb[0], bb[1], key, K, alpha, rescale=rescale, plan=p)
                    except NflHipError as err:
                        if err.code != ERR_UNSUPPORTED:
                            raise
                        continue
                    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (lb, n, nm, K, alpha, square, rescale, p)
                    plans.append(p)

                def prev():
                    if square:
                        kept.pointwise(OP_MUL, a0, a0, out=d[0])
                        kept.pointwise(OP_MUL, a0, a1, out=d[1])
                        kept.pointwise(OP_ADD, d[1], d[1], out=d[1])
                        kept.pointwise(OP_MUL, a1, a1, out=d[2])
                    else:
                        kept.pointwise(OP_MUL, a0, b0, out=d[0])
                        kept.dot_strided(A, (1, batch), Bx, (1, batch), batch, 2, out=d[1])
                        kept.pointwise(OP_MUL, a1, b1, out=d[2])
                    e.key_switch_ntt(d[2], key, K, alpha, out=(ks[0], ks[1]))
                    kept.pointwise(OP_ADD, d[0], ks[0], out=sums[0])
                    kept.pointwise(OP_ADD, d[1], ks[1], out=sums[1])
                    if rescale:
                        kept.rescale(sums[0], ntt=True, out=out[0])
                        kept.rescale(sums[1], ntt=True, out=out[1])

                prev()
                if not rescale:                                   # identity 1: the words of the one call
                    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), (lb, n, nm, K, alpha, square)
                half = moved // 2 // 16 * 16
                cs, cd = torch.empty(half, dtype=torch.uint8, device=a0.device), torch.empty(half, dtype=torch.uint8, device=a0.device)
                call = lambda plan: (lambda: e.mul_relin_ntt(a0, a1, bb[0], bb[1], key, K, alpha, rescale=rescale, out=(out[0], out[1]), plan=plan))  # noqa: E731
                fns = [call(p) for p in plans] + [call(None), prev, lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))]
                ms = timed_alternated(fns, args.iters, args.reps)
                med = [float(np.median(m)) for m in ms]
                spread = [float((max(m) - min(m)) / np.median(m)) for m in ms]
                rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "dnum": dnum, "batch": batch, "square": square,
                       "rescale": rescale, "compulsory_bytes": moved}
                for name, t, s in zip(plans + ["default", "prev", "copy"], med, spread):
                    rec[name + "_ms"], rec[name + "_spread"] = round(t, 4), round(s, 4)
                for name in plans + ["default"]:
                    rec["prev_over_" + name] = round(rec["prev_ms"] / rec[name + "_ms"], 3)
                rec["default_ratio_to_copy"] = round(rec["copy_ms"] / rec["default_ms"], 3)
                lines.append(json.dumps(rec))
                cell = lambda name: ("%7.3f ms +-%4.1f%% x%.3f" % (rec[name + "_ms"], 100 * rec[name + "_spread"], rec["prev_over_" + name])) \
                    if name + "_ms" in rec else "        -- (no fit)       "  # noqa: E731
                rows.append("%-11s K=%d alpha=%d dnum=%d batch %6d %-7s %-7s  prev %7.3f ms +-%4.1f%%  sequence %s  merged %s  fused %s  default %s  copy %7.3f ms" % (
                    rec["shape"], K, alpha, dnum, batch, "square" if square else "general", "rescale" if rescale else "", rec["prev_ms"],
                    100 * rec["prev_spread"], cell("sequence"), cell("merged"), cell("fused"), cell("default"), rec["copy_ms"]))
                del out, sums, ref, cs, cd, fns
        del A, Bx, a0, a1, b0, b1, key, d, ks
        kept.close()
        e.close()
        torch.cuda.empty_cache()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/mulrelin_bench.py --iters %d --reps %d (MI355X): x = prev / plan (above 1: the plan is faster than the hand composition "
                    "through the entries that existed before); +- = (max - min) / median of the variant's blocks in this run; copy = hipMemcpyAsync D2D "
                    "of the compulsory bytes (4 L rows read, 2 L for the square; 2 L or 2 (L - 1) written; the key once)\n" % (args.iters, args.reps))
            f.write(text)


if __name__ == "__main__":
    main()
