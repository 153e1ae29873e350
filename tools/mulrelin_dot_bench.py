#!/usr/bin/env python3
"""Time the sums of ciphertext products (nflhip_tensor_dot_ntt_dev, nflhip_mulrelin_dot_ntt_dev) in one run, in the manner of
tools/mulrelin_bench.py: every variant of a point is alternated block by block, --reps blocks of --iters calls between two HIP events
each, after two warm-up calls of every variant; reported per variant are the median of the block means and the spread
(max - min) / median of its blocks.  Words are asserted equal before anything is timed, wherever the variants compute the same words.

The kernel alone (rows = all moduli, groups sized to about --gib of compulsory bytes: 4 terms + 3 rows per output row):
  kernel    one launch of k_tensor_dot_ntt
  dot4      the four nflhip_dot_dev calls that form the same words (the cross sum through the addend)
  per_term  nflhip_tensor_ntt_dev per term and nflhip_pointwise_dev additions
  copy      hipMemcpyAsync device-to-device of the compulsory bytes
The call (groups sized to about --gib of compulsory bytes: 4 terms L rows read, 2 L or 2 (L - 1) written, the key once):
  default   nflhip_mulrelin_dot_ntt_dev at its default plan
  sequence  the same, the sequence forced
  per_term  `terms` calls of mul_relin_ntt at its default plan summed by pointwise additions, then rescale twice where it applies: what
            a caller had before, one key switch per product (other words: `terms` key-switch errors and, with the rescale, two roundings)
  lazy      tensor_ntt per term, additions, key_switch_ntt, two additions (and rescale twice): the best a caller could compose before

usage: tools/mulrelin_dot_bench.py [--iters N] [--reps R] [--gib G] [--out FILE]   (tables, then one line of JSON per point)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402
from nfllib_amd._lib import OP_ADD  # noqa: E402

GIB = 1 << 30
TERMS = (2, 4, 8, 16)
KERNEL_POINTS = [(64, 4096, 4), (32, 4096, 3)]
CALL_POINTS = [(64, 1024, 4, 1, 1), (64, 4096, 4, 1, 1), (64, 4096, 4, 2, 2), (32, 4096, 3, 1, 1)]


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


def record(rec, names, ms):
    for name, m in zip(names, ms):
        rec[name + "_ms"] = round(float(np.median(m)), 4)
        rec[name + "_spread"] = round(float((max(m) - min(m)) / np.median(m)), 4)


def copy_fn(e, nbytes, device):
    half = nbytes // 2 // 16 * 16
    cs, cd = torch.empty(half, dtype=torch.uint8, device=device), torch.empty(half, dtype=torch.uint8, device=device)
    st = e._stream()
    return lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, cd.data_ptr(), cs.data_ptr(), half, st))


def kernel_alone(args, lines, rows):
    for lb, n, nm in KERNEL_POINTS:
        e = Engine(lb, n, nm)
        row = n * (lb // 8)
        for terms in TERMS:
            groups = max(int(args.gib * GIB) // ((4 * terms + 3) * nm * row), 1)
            moved = groups * (4 * terms + 3) * nm * row
            ops = [e.fill_uniform(e.empty(groups * terms), 10 + k, 0) for k in range(4)]
            a0, a1, b0, b1 = ops
            out = e.empty(3 * groups).view(3, groups, nm, n)
            alt, tmp = e.empty(3 * groups).view(3, groups, nm, n), e.empty(3 * groups).view(3, groups, nm, n)
            s = (1, groups)                                        # term-major blocks [terms][groups]: term j of every group is dense
            v = [x.view(terms, groups, nm, n) for x in ops]

            def kernel():
                e.tensor_dot_strided((a0, s), (a1, s), (b0, s), (b1, s), groups, terms, outs=(out[0], out[1], out[2]))

            def dot4():
                e.dot_strided(a0, s, b0, s, groups, terms, out=alt[0])
                e.dot_strided(a0, s, b1, s, groups, terms, out=alt[1])
                e.dot_strided(a1, s, b0, s, groups, terms, addend=alt[1], out=alt[1])
                e.dot_strided(a1, s, b1, s, groups, terms, out=alt[2])

            def per_term():
                for j in range(terms):
                    dst = alt if j == 0 else tmp
                    e.tensor_ntt(v[0][j], v[1][j], v[2][j], v[3][j], outs=(dst[0], dst[1], dst[2]))
                    if j:
                        for c in range(3):
                            e.pointwise(OP_ADD, alt[c], tmp[c], out=alt[c])

            kernel()
            dot4()
            assert torch.equal(out, alt), (lb, n, nm, terms, "dot4")
            per_term()
            assert torch.equal(out, alt), (lb, n, nm, terms, "per_term")
            names = ["kernel", "dot4", "per_term", "copy"]
            ms = timed_alternated([kernel, dot4, per_term, copy_fn(e, moved, a0.device)], args.iters, args.reps)
            rec = {"part": "kernel", "shape": "u%d/%d/%d" % (lb, n, nm), "terms": terms, "groups": groups, "compulsory_bytes": moved}
            record(rec, names, ms)
            rec["dot4_over_kernel"] = round(rec["dot4_ms"] / rec["kernel_ms"], 3)
            rec["per_term_over_kernel"] = round(rec["per_term_ms"] / rec["kernel_ms"], 3)
            rec["kernel_ratio_to_copy"] = round(rec["copy_ms"] / rec["kernel_ms"], 3)
            lines.append(json.dumps(rec))
            rows.append("kernel %-10s terms %2d groups %5d  kernel %7.3f ms +-%4.1f%%  dot4 %7.3f ms +-%4.1f%% x%.3f  per_term %8.3f ms +-%4.1f%% x%.3f  copy %7.3f ms (%.2f of the kernel)" % (
                rec["shape"], terms, groups, rec["kernel_ms"], 100 * rec["kernel_spread"], rec["dot4_ms"], 100 * rec["dot4_spread"], rec["dot4_over_kernel"],
                rec["per_term_ms"], 100 * rec["per_term_spread"], rec["per_term_over_kernel"], rec["copy_ms"], rec["kernel_ratio_to_copy"]))
            del ops, a0, a1, b0, b1, out, alt, tmp, v
            torch.cuda.empty_cache()
        e.close()


def the_call(args, lines, rows):
    for lb, n, nm, K, alpha in CALL_POINTS:
        e = Engine(lb, n, nm)
        L, row = nm - K, n * (lb // 8)
        kept = Engine(lb, n, L)
        dnum = e.keyswitch_digits(K, alpha)
        kbytes = 2 * dnum * nm * row
        key = e.fill_uniform(e.empty(2 * dnum), 3, 0)
        for terms in TERMS:
            for rescale in (False, True):
                R = L - 1 if rescale else L
                groups = max(int(args.gib * GIB - kbytes) // ((4 * terms * L + 2 * R) * row), 1)
                moved = groups * (4 * terms * L + 2 * R) * row + kbytes
                ops = [kept.fill_uniform(kept.empty(groups * terms), 20 + k, 0) for k in range(4)]
                a0, a1, b0, b1 = ops
                v = [x.view(terms, groups, L, n) for x in ops]          # term-major blocks [terms][groups]: term j of every group is dense
                s = (1, groups)
                out = torch.empty((2, groups, R, n), dtype=e.torch_dtype, device=a0.device)
                alt = torch.empty((2, groups, R, n), dtype=e.torch_dtype, device=a0.device)
                acc = kept.empty(2 * groups).view(2, groups, L, n)
                part = kept.empty(2 * groups).view(2, groups, L, n)
                d, dt = kept.empty(3 * groups).view(3, groups, L, n), kept.empty(3 * groups).view(3, groups, L, n)

                def call(plan, o):
                    return lambda: e.mul_relin_dot_strided((a0, s), (a1, s), (b0, s), (b1, s), groups, terms, key, K, alpha, rescale=rescale,
                                                           out=(o[0], o[1]), plan=plan)

                def finish(sums, o):
                    if rescale:
                        kept.rescale(sums[0], ntt=True, out=o[0])
                        kept.rescale(sums[1], ntt=True, out=o[1])

                def per_term():
                    sums = acc if rescale else alt
                    for j in range(terms):
                        dst = sums if j == 0 else part
                        e.mul_relin_ntt(v[0][j], v[1][j], v[2][j], v[3][j], key, K, alpha, out=(dst[0], dst[1]))
                        if j:
                            for c in range(2):
                                kept.pointwise(OP_ADD, sums[c], part[c], out=sums[c])
                    finish(sums, alt)

                def lazy():
                    sums = acc if rescale else alt
                    for j in range(terms):
                        dst = d if j == 0 else dt
                        e.tensor_ntt(v[0][j], v[1][j], v[2][j], v[3][j], rows=L, outs=(dst[0], dst[1], dst[2]))
                        if j:
                            for c in range(3):
                                kept.pointwise(OP_ADD, d[c], dt[c], out=d[c])
                    e.key_switch_ntt(d[2], key, K, alpha, out=(part[0], part[1]))
                    for c in range(2):
                        kept.pointwise(OP_ADD, d[c], part[c], out=sums[c])
                    finish(sums, alt)

                call(None, out)()
                call("sequence", alt)()
                assert torch.equal(out, alt), (lb, n, nm, K, alpha, terms, rescale, "sequence")
                if not rescale:                                   # identity 1: the words of the one call
                    lazy()
                    assert torch.equal(out, alt), (lb, n, nm, K, alpha, terms, "lazy")
                names = ["default", "sequence", "per_term", "lazy", "copy"]
                ms = timed_alternated([call(None, out), call("sequence", out), per_term, lazy, copy_fn(e, moved, a0.device)], args.iters, args.reps)
                rec = {"part": "call", "shape": "u%d/%d/%d" % (lb, n, nm), "k_special": K, "alpha": alpha, "dnum": dnum, "terms": terms, "groups": groups,
                       "rescale": rescale, "compulsory_bytes": moved}
                record(rec, names, ms)
                for name in ("sequence", "per_term", "lazy"):
                    rec[name + "_over_default"] = round(rec[name + "_ms"] / rec["default_ms"], 3)
                rec["default_ratio_to_copy"] = round(rec["copy_ms"] / rec["default_ms"], 3)
                lines.append(json.dumps(rec))
                rows.append("call %-10s K=%d alpha=%d terms %2d groups %5d %-7s  default %8.3f ms +-%4.1f%%  sequence %8.3f ms +-%4.1f%% x%.3f  per_term %8.3f ms +-%4.1f%% x%.3f  lazy %8.3f ms +-%4.1f%% x%.3f  copy %7.3f ms" % (
                    rec["shape"], K, alpha, terms, groups, "rescale" if rescale else "", rec["default_ms"], 100 * rec["default_spread"], rec["sequence_ms"],
                    100 * rec["sequence_spread"], rec["sequence_over_default"], rec["per_term_ms"], 100 * rec["per_term_spread"], rec["per_term_over_default"],
                    rec["lazy_ms"], 100 * rec["lazy_spread"], rec["lazy_over_default"], rec["copy_ms"]))
                del ops, a0, a1, b0, b1, v, out, alt, acc, part, d, dt
                torch.cuda.empty_cache()
        del key
        for x in (kept, e):
            x.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0, help="compulsory traffic per call the groups are sized to")
    ap.add_argument("--part", choices=("kernel", "call", "both"), default="both")
    args = ap.parse_args()
    lines, rows = [], []
    if args.part in ("kernel", "both"):
        kernel_alone(args, lines, rows)
    if args.part in ("call", "both"):
        the_call(args, lines, rows)
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/mulrelin_dot_bench.py --iters %d --reps %d --gib %g (MI355X): x = variant / kernel (part kernel) or variant / default (part "
                    "call), above 1: the new entry is faster; +- = (max - min) / median of the variant's blocks in this run; copy = hipMemcpyAsync "
                    "D2D of the compulsory bytes\n" % (args.iters, args.reps, args.gib))
            f.write(text)


if __name__ == "__main__":
    main()
