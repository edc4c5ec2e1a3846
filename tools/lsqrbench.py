"""lsqr benchmark on one GPU, per matrix in ONE process.

    python tools/lsqrbench.py              # all cases -> profiles/lsqrbench.json

Matrix: 7-point diffusion plus first-order upwind convection on n^3 points,
built in numpy as CSR (general storage) from the Poisson pattern: diagonal 6 +
3 c, upper neighbours -1, lower neighbours -1 - c (`--c`, default 0.5): square
and nonsymmetric.

One JSON record per case:

  step      wall ms per iteration at rtol = ltol = 0 over `--iters` iterations
            on a reused workspace -- lsqr, gmres(restart 30) and bicgstab --
            with the products' share from one more solve with
            CgOptions::time_spmv, and the launches per iteration beside the
            products by the solvers' own launch lists (host/cg.h)
  solve     iterations, status and wall ms to rtol `--rtol` (kmax `--kmax`),
            b = A.1, all three without a preconditioner

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("convdiff",)
# launches of one iteration on one rank beside the products (host/cg.h)
LAUNCHES = dict(lsqr=4, gmres30=8, bicgstab=5)


def spread(ms):
    return dict(min=float(min(ms)), median=float(np.median(ms)),
                max=float(max(ms)), n=len(ms))


def timed(fn, repeats, warmup):
    """wall ms of every repeat of fn (which ends synchronised)"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def run_case(case, args):
    from spmv_amd import _lib, host, poisson
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    rp, ci, va = poisson.poisson3d_csr(args.n)
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    va = np.array(va, np.float64)
    rows = len(rp) - 1
    row = np.repeat(np.arange(rows), np.diff(rp))
    va[ci == row] += 3.0 * args.c
    va[ci < row] -= args.c
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, rows, rows, [], [],
                                  False, host.P2P_BLOCKING)
    rec = dict(case=case, n=args.n, rows=rows, nnz=A.non_zeros(), c=args.c,
               repeats=args.repeats, warmup=args.warmup)
    d_b, d_x, d_one = (exec_.alloc(rows) for _ in range(3))
    _lib.call("spmv_hip_fill_const_f64", exec_.context, rows, 1.0, d_one, None)
    A.col_map().update(d_one)
    A.mult(d_one, d_b)  # b = A.1
    exec_.synchronize()
    ws_l, ws_g = host.LsqrWorkspace(exec_), host.GmresWorkspace(exec_)
    ws_b = host.BicgstabWorkspace(exec_)
    for w in (ws_l, ws_g, ws_b):
        w.reserve_timing(max(args.iters, args.kmax))

    def solvers(kmax, rtol):
        """name -> fn(time_spmv, stats) -> (k, hist, status)"""
        def lsqr(t, st):
            k, hist_r, _, status = host.lsqr(comm, exec_, A, d_b, d_x, kmax, rtol,
                                             ws=ws_l, time_spmv=t, stats=st)
            return k, hist_r, status
        return {"lsqr": lsqr,
                "gmres30": lambda t, st: host.gmres(
                    comm, exec_, A, d_b, d_x, 30, kmax, rtol, ws=ws_g,
                    time_spmv=t, stats=st),
                "bicgstab": lambda t, st: host.bicgstab(
                    comm, exec_, A, d_b, d_x, None, kmax, rtol, ws=ws_b,
                    time_spmv=t, stats=st)}

    rec["step"] = {}
    for name, fn in solvers(args.iters, 0.0).items():
        ms = timed(lambda: fn(False, None), args.repeats, args.warmup)
        st = {}
        k, _, status = fn(True, st)
        if k != args.iters:  # (bicgstab may break down or converge exactly)
            rec["step"][name] = dict(iters=k, status=status)
            continue
        per = min(ms) / k
        spmv = st["spmv_ms_total"] / max(st["spmv_launches"], 1)
        spmvs = st["spmv_launches"] / k
        rec["step"][name] = dict(
            iters=k, ms_per_iteration=per,
            ms_per_iteration_med=float(np.median(ms)) / k,
            spmvs_per_iteration=spmvs, spmv_ms=spmv,
            nonspmv_ms_per_iteration=per - spmv * spmvs,
            launches_per_iteration=LAUNCHES[name])
    rec["solve"] = dict(rtol=args.rtol, kmax=args.kmax)
    for name, fn in solvers(args.kmax, args.rtol).items():
        got = {}
        ms = timed(lambda: got.update(r=fn(False, None)), args.repeats,
                   args.warmup)
        k, hist, status = got["r"]
        rec["solve"][name] = dict(iterations=k, status=status, ms=spread(ms),
                                  ms_per_iteration=min(ms) / max(k, 1),
                                  rel_residual=float(hist[-1] / hist[0]))
    print(json.dumps(rec), flush=True)
    for w in (ws_l, ws_g, ws_b):
        w.close()
    for p in (d_b, d_x, d_one):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="grid edge")
    ap.add_argument("--c", type=float, default=0.5, help="the convection")
    ap.add_argument("--iters", type=int, default=60,
                    help="iterations of the fixed-length solves")
    ap.add_argument("--kmax", type=int, default=3000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "lsqrbench.json"))
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
               os.path.abspath(__file__), "--case", case]
        for key in ("n", "c", "iters", "kmax", "rtol", "repeats", "warmup"):
            cmd += ["--" + key, str(getattr(args, key))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"lsqrbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
