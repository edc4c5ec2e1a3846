"""Transposed-product benchmark on one GPU: for each matrix, the forward
product and the transposed product in every form the block can take (copy +
inner plan, in place, self-transpose), all in ONE process, interleaved
rounds, best and median of each (events around `reps` back-to-back launches).

    python tools/tbench.py --n 512 --rows 10000000 --out tbench.json

Prints one JSON line per matrix: mult / transpmult ms per form, t_plan_us,
t_kib, and bytes per stored entry against the CSR roofline (the forward
product's compulsory bytes: 12 B per entry + rowptr + x + y).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spmv_amd import hip, poisson  # noqa: E402

FORM_NAMES = {1: "copy", 2: "in_place", 3: "self"}


def time_rounds(ctx, fns, reps, rounds):
    """{name: (best ms, median ms)}; the variants interleave round by round"""
    e0, e1 = ctx.event_create(), ctx.event_create()
    res = {k: [] for k in fns}
    for fn in fns.values():  # warm-up (and the XW probe's first launches)
        for _ in range(4):
            fn()
    ctx.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            ctx.event_record(e0)
            for _ in range(reps):
                fn()
            ctx.event_record(e1)
            ctx.event_sync(e1)
            res[k].append(ctx.elapsed_ms(e0, e1) / reps)
    ctx.event_destroy(e0), ctx.event_destroy(e1)
    return {k: (min(v), float(np.median(v))) for k, v in res.items()}


def measure(ctx, name, blk, reps, rounds):
    n, m = blk.nrows, blk.ncols
    x = ctx.empty(max(n, m), np.float64)
    y = ctx.empty(max(n, m), np.float64)
    ctx.fill_gaussian(max(n, m), 0, max(n, m), x.ptr)
    blk.transpose()
    form = blk.get("t_form")
    fns = {"mult": lambda: blk.mult(1.0, x.ptr, 0.0, y.ptr),
           FORM_NAMES[form]: lambda: blk.multt(1.0, x.ptr, 0.0, y.ptr)}
    t = time_rounds(ctx, fns, reps, rounds)
    blk.set("t_in_place", 1)
    t.update(time_rounds(ctx, {"in_place": lambda: blk.multt(1.0, x.ptr, 0.0,
                                                              y.ptr)},
                         reps, rounds))
    blk.set("t_in_place", 0)
    roof = poisson.csr_bytes(n, m, blk.nnz)
    rec = dict(matrix=name, rows=n, cols=m, nnz=blk.nnz, t_form=form,
               t_plan_us=blk.get("t_plan_us"), t_kib=blk.get("t_kib"),
               plan_kib=blk.get("plan_kib"),
               inner={k: blk.get("t." + k) for k in ("lat", "lx", "xw", "sdia",
                                                     "sdia_const", "wdia",
                                                     "wdia_const", "sjds")},
               csr_roofline_bytes_per_entry=roof / blk.nnz)
    for k, (best, med) in t.items():
        rec[k + "_ms"] = best
        rec[k + "_ms_med"] = med
        # the CSR roofline's bytes over the launch's time
        rec[k + "_gbs_at_roofline_bytes"] = roof / best / 1e6
    for k in t:
        if k != "mult":
            rec[k + "_over_mult"] = t[k][0] / t["mult"][0]
    print(json.dumps(rec), flush=True)
    x.free(), y.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the unstructured / FEM-like matrices")
    ap.add_argument("--skew-ppm", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma list of matrices")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    ctx = hip.Context(0)
    recs = []

    def want(k):
        return only is None or k in only

    N = args.n ** 3
    for name, skew in (("poisson", 0), ("poisson_skew", args.skew_ppm)):
        if not want(name):
            continue
        ctx.set_option("poisson_skew_ppm", skew)
        blk = hip.poisson3d_block(ctx, args.n, 0, N, hip.PART_ALL)
        ctx.set_option("poisson_skew_ppm", 0)
        blk.bake()
        recs.append(measure(ctx, f"{name}_{args.n}^3", blk, args.reps, args.rounds))
        blk.free()
    for name in ("unstructured", "fem_like"):
        if not want(name):
            continue
        if name == "unstructured":
            rp, ci, va = poisson.unstructured_csr(args.rows, per_row=7,
                                                  far_permille=100)
        else:
            rp, ci, va = poisson.fem_like_csr(args.rows)
        blk = hip.CsrBlock(ctx, args.rows, args.rows, np.asarray(rp, np.int32),
                           np.asarray(ci, np.int32), va)
        del rp, ci, va
        blk.bake()
        recs.append(measure(ctx, f"{name}_{args.rows}", blk, args.reps, args.rounds))
        blk.free()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
