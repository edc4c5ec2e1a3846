"""amg_apply_block / pcg_block(amg) benchmark on one GPU: the block V-cycle and
the block solver against the single-vector calls on the same objects, per
matrix in ONE process.

    python tools/amgbbench.py                # all cases -> profiles/amgbbench.json
    python tools/amgbbench.py --only poisson64   # the launch-bound case alone

Cases: the 7-point Poisson matrix on 64^3 points (an application is
launch-bound below level 0), on 512^3 points in CSR order,
and the FEM-like matrix of 10 M rows.  For nrhs = 2, 4, 8 one JSON record:
  apply    one amg_apply_block against nrhs calls of amg_apply on the same
           AmgPreconditioner: ms per application (wall time of one application
           ended by one synchronisation; minimum and median of `--repeats`
           repeats after `--warmup` warm-ups) and launches per application
           (counted from the hierarchy: levels, degrees, which products take the
           per-column path);
  solves   pcg_block with the AMG object against nrhs solves of pcg_amg with the
           same object and against pcg_block with an SgsPreconditioner, all to
           rtol = 1e-10 on right-hand sides B = A X* with a seeded X*:
           iterations (the largest column's), ms per iteration, time to 1e-10.
The baseline of every ratio is the single-vector calls timed in the same
process.

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cgbbench import WIDTHS, make_matrix, timed  # noqa: E402

RTOL = 1e-10
CASES = {"poisson64": ("poisson_csr", dict(n=64)),
         "poisson512": ("poisson_csr", dict(n=512)),
         "fem_like": ("fem_like", dict(rows=10_000_000))}


def launches(M, nrhs):
    """launches of one application, from the shape of the cycle: per level 2s + 1
    products and 2s + 2 vector kernels (the coarsest: c - 1 and c), one copy
    out.  A product of a block is one launch, or -- where mult_block takes the
    plan's single-vector launch per column -- nrhs + 2; which levels do is not
    visible from here, so the block count is the lower bound."""
    s, c, nl = M.options["smooth_degree"], M.options["coarse_degree"], M.levels()
    per_level = (2 * s + 1) + (2 * s + 2)
    return (nl - 1) * per_level + (2 * c - 1) + 1


def run_case(case, args):
    from spmv_amd import _lib, host
    kind, size = CASES[case]
    for k, v in size.items():
        setattr(args, k, v)
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    A = make_matrix(kind, args, comm, exec_, host, _lib)
    rows, nnz = A.rows(), A.non_zeros()
    amg = host.AmgPreconditioner(exec_, A)
    sgs = host.SgsPreconditioner(exec_, A)
    ws1, wsb = host.AmgPcgWorkspace(exec_), host.PcgBlockWorkspace(exec_)
    for nrhs in [w for w in WIDTHS if not args.widths
                 or str(w) in args.widths.split(",")]:
        n = rows * nrhs
        d_b, d_x, d_s = exec_.alloc(n), exec_.alloc(n), exec_.alloc(n)
        _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, n, 0, n, d_x, None)
        A.mult_block(d_x, d_b, nrhs)  # (one rank: no ghosts to update)
        exec_.synchronize()
        B = exec_.copy_to_host(d_b, n).reshape(rows, nrhs)
        exec_.copy_from_host(d_s, np.ascontiguousarray(B.T))
        rec = dict(case=case, rows=rows, nnz=nnz, nrhs=nrhs, repeats=args.repeats,
                   warmup=args.warmup, levels=amg.levels(),
                   level_rows=[amg.rows(l) for l in range(amg.levels())],
                   launches_per_apply_single=launches(amg, 1),
                   launches_per_apply_block_min=launches(amg, nrhs))

        def apply_block():
            host.amg_apply_block(exec_, amg, d_b, d_x, nrhs)
            exec_.synchronize()

        def apply_single():
            for c in range(nrhs):
                host.amg_apply(exec_, amg, d_s + 8 * rows * c, d_x + 8 * rows * c)
            exec_.synchronize()

        for name, fn in (("apply_block", apply_block),
                         ("nrhs_applies", apply_single)):
            ms = timed(fn, args.repeats, args.warmup)
            rec[name + "_ms_min"] = min(ms)
            rec[name + "_ms_med"] = float(np.median(ms))
        rec["apply_ratio_vs_nrhs_applies"] = (rec["nrhs_applies_ms_min"]
                                              / rec["apply_block_ms_min"])
        state = {}

        def solve_block(**pre):
            def fn():
                its, _, _ = host.pcg_block(comm, exec_, A, d_b, d_x, nrhs,
                                           args.kmax, RTOL, workspace=wsb, **pre)
                state["k"] = int(its.max())
            return fn

        def solve_singles():
            ks = []
            for c in range(nrhs):
                k, _ = host.pcg_amg(comm, exec_, A, amg, d_s + 8 * rows * c,
                                    d_x + 8 * rows * c, args.kmax, RTOL, ws1)
                ks.append(k)
            state["k"] = max(ks)

        for name, fn in (("pcg_block_amg", solve_block(amg=amg)),
                         ("nrhs_pcg_amg", solve_singles),
                         ("pcg_block_sgs", solve_block(sgs=sgs))):
            ms = timed(fn, args.solve_repeats, 1)
            k = state["k"]
            rec[name] = dict(iterations=k, converged=k < args.kmax,
                             ms_to_rtol_min=min(ms),
                             ms_to_rtol_med=float(np.median(ms)),
                             ms_per_iteration=min(ms) / max(k, 1))
        rec["solve_ratio_vs_nrhs_pcg_amg"] = (
            rec["nrhs_pcg_amg"]["ms_to_rtol_min"]
            / rec["pcg_block_amg"]["ms_to_rtol_min"])
        print(json.dumps(rec), flush=True)
        for p in (d_b, d_x, d_s):
            exec_.free(p)
    for w in (ws1, wsb):
        w.close()
    amg.close(), sgs.close()
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmax", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--widths", default=None, help="comma list of nrhs")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "amgbbench.json"))
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:  # a child: one case in this process
        run_case(args.case, args)
        return 0
    cases = [c for c in CASES if not args.only or c in args.only.split(",")]
    recs = []
    p = None
    for case in cases:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", case, "--kmax",
               str(args.kmax), "--repeats", str(args.repeats), "--warmup",
               str(args.warmup), "--solve-repeats", str(args.solve_repeats)]
        if args.widths:
            cmd += ["--widths", args.widths]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"amgbbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
