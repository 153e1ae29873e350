#!/usr/bin/env python3
"""Time the sums of products across polynomials (nflhip_dot_dev, nflhip_dot_ptrs_dev) in one run:
  dense    -- groups x terms at u64/4096/4 and u32/4096/3: bytes moved, (2 terms + 1) rows per output row, over time, next to
              a same-run hipMemcpyAsync device-to-device copy that moves the same byte count (read + write), and next to the
              only route without the entry, `terms` chained programs c = a * b, then c = c + a * b: nflhip_eval_dev on a
              term-major copy of the operands (its operands are dense batches), and nflhip_eval_strided_dev on the operands
              as the dot reads them;
  matvec   -- matrix times shared vector at u64/4096/4, terms 4 / 16 / 64: the tiled plan (four groups per load of the shared
              words) against NFLHIP_DOT_UNTILED (the default column is the dispatcher's choice, api.hip dot_tiled_on);
  pointers -- the pointer form on 16 terms against the strided form on the same data, one output polynomial per launch.
Operands exceed 256 MiB in the dense and matvec figures; the pointer figure works on 4 MiB, 32 polynomials, and compares launch
and addressing cost, not bandwidth.  Every figure: two warm-up calls, then --iters calls between two HIP events,
repeated --reps times; the median is reported.

usage: tools/dot_bench.py [--iters N] [--reps R] [--groups G] [--out FILE]   (a table, then one line of JSON per measurement)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfllib_amd import Engine  # noqa: E402

DENSE = [(64, 4096, 4, (2, 4, 16)), (32, 4096, 3, (16,))]
MATVEC = (64, 4096, 4, (4, 16, 64))
MUL, MAC = [0, 1, 0x12], [0, 1, 2, 0x12, 0x10]      # postfix programs: a * b, c + a * b


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    it, rp, groups = args.iters, args.reps, args.groups
    lines, rows = [], []
    for lb, n, nm, term_list in DENSE:
        e = Engine(lb, n, nm)
        tmax = max(term_list)
        a = e.fill_uniform(e.empty(groups * tmax), 1, 0)
        b = e.fill_uniform(e.empty(groups * tmax), 2, 1)
        out, c, c2 = e.empty(groups), e.empty(groups), e.empty(groups)
        at = a.view(groups, tmax, nm, n).transpose(0, 1).contiguous()    # [term][group]: term j is one dense batch
        bt = b.view(groups, tmax, nm, n).transpose(0, 1).contiguous()
        st = e._stream()
        for terms in term_list:   # (the operands keep their stride of tmax polynomials per group)
            moved = (2 * terms + 1) * n * nm * (lb // 8) * groups
            half = moved // 2 // 16 * 16
            src, dst = torch.empty(half, dtype=torch.uint8, device=a.device), torch.empty(half, dtype=torch.uint8, device=a.device)
            ms_copy = timed(lambda: e._chk(e.lib.nflhip_memcpy_d2d(e.ctx, dst.data_ptr(), src.data_ptr(), half, st)), it, rp)
            del src, dst
            ms = timed(lambda: e.dot_strided(a, (tmax, 1), b, (tmax, 1), groups, terms, out=out), it, rp)

            def chain():
                e.eval_strided(MUL, [a, b], [tmax, tmax], c, batch=groups)
                for j in range(1, terms):
                    e.eval_strided(MAC, [c, a[j:], b[j:]], [1, tmax, tmax], c, batch=groups)
            ms_chain = timed(chain, it, rp)

            def chain_eval():
                e.eval(MUL, [at[0], bt[0]], out=c2)
                for j in range(1, terms):
                    e.eval(MAC, [c2, at[j], bt[j]], out=c2)
            ms_eval = timed(chain_eval, it, rp)
            same = bool(torch.equal(out, c)) and bool(torch.equal(out, c2))
            tbs, ctbs = moved / ms / 1e9, 2 * half / ms_copy / 1e9
            rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "groups": groups, "terms": terms, "plan": "dense", "ms": round(ms, 4),
                   "TB_per_s": round(tbs, 3), "copy_ms": round(ms_copy, 4), "copy_TB_per_s": round(ctbs, 3),
                   "ratio_to_copy": round(tbs / ctbs, 3), "chain_eval_ms": round(ms_eval, 4), "chain_eval_over_dot": round(ms_eval / ms, 3),
                   "chain_strided_ms": round(ms_chain, 4), "chain_strided_over_dot": round(ms_chain / ms, 3),
                   "chains_give_the_same_words": same}
            lines.append(json.dumps(rec))
            rows.append("%-12s groups %5d terms %3d  dot %8.3f ms %6.2f TB/s   copy %8.3f ms %6.2f TB/s  ratio %.3f   chain eval %8.3f ms (x%.2f)  eval_strided %8.3f ms (x%.2f)  same words: %s" % (
                rec["shape"], groups, terms, ms, tbs, ms_copy, ctbs, tbs / ctbs, ms_eval, ms_eval / ms, ms_chain, ms_chain / ms, same))
        del a, b, at, bt, out, c, c2
        e.close()
        torch.cuda.empty_cache()
    lb, n, nm, term_list = MATVEC
    e = Engine(lb, n, nm)
    for terms in term_list:
        m = e.fill_uniform(e.empty(groups * terms), 3, 0)
        v = e.fill_uniform(e.empty(terms), 4, 1)
        o1, o2 = e.empty(groups), e.empty(groups)
        ms_u = timed(lambda: e.matvec(m, v, out=o2, untiled=True), it, rp)
        ms_d = timed(lambda: e.matvec(m, v, out=o1), it, rp)      # the dispatcher's choice (api.hip dot_tiled_on)
        same = bool(torch.equal(o1, o2))
        compulsory = ((terms + 1) * groups + terms) * n * nm * (lb // 8)
        rec = {"shape": "u%d/%d/%d" % (lb, n, nm), "groups": groups, "terms": terms, "plan": "matvec", "default_ms": round(ms_d, 4),
               "untiled_ms": round(ms_u, 4), "untiled_over_default": round(ms_u / ms_d, 3),
               "default_TB_per_s_of_compulsory_bytes": round(compulsory / ms_d / 1e9, 3), "same_words": same}
        lines.append(json.dumps(rec))
        rows.append("%-12s groups %5d terms %3d  matvec default %8.3f ms   untiled %8.3f ms (x%.3f)   %6.2f TB/s of compulsory bytes  same words: %s" % (
            rec["shape"], groups, terms, ms_d, ms_u, ms_u / ms_d, compulsory / ms_d / 1e9, same))
        del m, v, o1, o2
        torch.cuda.empty_cache()
    terms = 16
    a, b = e.fill_uniform(e.empty(terms), 5, 0), e.fill_uniform(e.empty(terms), 6, 1)
    pa, pb, o1, o2 = list(a.split(1)), list(b.split(1)), e.empty(1), e.empty(1)
    ms_s = timed(lambda: e.dot(a, b, terms, out=o1), 10 * it, rp)
    ms_p = timed(lambda: e.dot_list(pa, pb, out=o2), 10 * it, rp)
    rec = {"shape": "u64/4096/4", "groups": 1, "terms": terms, "plan": "pointers", "strided_ms": round(ms_s, 5), "pointers_ms": round(ms_p, 5),
           "pointers_over_strided": round(ms_p / ms_s, 3), "same_words": bool(torch.equal(o1, o2))}
    lines.append(json.dumps(rec))
    rows.append("u64/4096/4   groups     1 terms  16  strided %8.4f ms   pointer form %8.4f ms (x%.3f)  same words: %s" % (ms_s, ms_p, ms_p / ms_s, rec["same_words"]))
    e.close()
    text = "\n".join(rows + [""] + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/dot_bench.py --iters %d --reps %d --groups %d (MI355X): dense bytes = (2 terms + 1) rows per output row; "
                    "copy = hipMemcpyAsync D2D moving the same bytes\n" % (it, rp, groups))
            f.write(text)


if __name__ == "__main__":
    main()
