"""idrs benchmark on one GPU against bicgstab and gmres(30), one matrix per
process.

    python tools/idrsbench.py              # -> profiles/idrsbench.json

Matrices on n^3 points, general storage, no preconditioner:
  convdiff  the convection-diffusion matrix of the solver tests (diagonal 7.6,
            varying off-diagonals), b = A u with u = uniform(-1, 1)
  cdpe      central differences at cell Peclet number `--pe` (diagonal 6,
            off-diagonals -(1 +- pe)), b_i = sin(0.37 i) + 0.5: IDR(1) and
            BiCGStab are expected to fail here, s >= 4 to converge

One JSON record per matrix, with one entry per solver (idrs at s = 1, 2, 4, 8,
bicgstab, gmres(30)):

  step      wall ms per step at rtol = 0 over `--iters` steps on a reused
            workspace (min and median of `--repeats`), products per step (2 for
            bicgstab), the product's share from one more solve with time_spmv,
            and for idrs the bytes per second of what is left beside the
            product against the 2 s + 11 vector passes of an inner step
  solve     to rtol `--rtol` within `--kmax`: steps, products, status, the last
            recurrence residual over the first, total ms

The driver starts one child process per matrix under `timeout` and stops at the
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

MATRICES = ("convdiff", "cdpe")
S_VALUES = (1, 2, 4, 8)


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


def to_csr(N, rows, cols, vals):
    rows, cols, vals = map(np.concatenate, (rows, cols, vals))
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
    return (rp.astype(np.int32), cols[order].astype(np.int32),
            vals[order].astype(np.float64))


def stencil(n, diag, lower, upper):
    """7-point matrix on n^3: lower(d, a, b) / upper(d, a, b) give the entries
    (b, a) and (a, b) of the neighbours a, b = a + n^d"""
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, diag)]
    for d in range(3):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [lower(d, a, b), upper(d, a, b)]
    return to_csr(N, rows, cols, vals)


def convdiff(n):
    c = (0.9, 0.5, 0.2)
    return stencil(
        n, 7.6,
        lambda d, a, b: -(1 + c[d]) * (1 + 0.3 * np.sin(b.astype(np.float64))),
        lambda d, a, b: -(1 + 0.3 * np.cos(a.astype(np.float64))))


def cdpe(n, pe):
    return stencil(n, 6.0, lambda d, a, b: np.full(len(a), -(1.0 + pe)),
                   lambda d, a, b: np.full(len(a), -(1.0 - pe)))


def run_case(name, args):
    from spmv_amd import host
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    rp, ci, va = convdiff(args.n) if name == "convdiff" else cdpe(args.n, args.pe)
    rows = len(rp) - 1
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, rows, rows, [], [],
                                  False, host.P2P_BLOCKING)
    d_b, d_u, d_x = exec_.alloc(rows), exec_.alloc(rows), exec_.alloc(rows)
    if name == "convdiff":
        exec_.copy_from_host(d_u, np.random.default_rng(rows).uniform(-1, 1, rows))
        A.col_map().update(d_u)
        A.mult(d_u, d_b)
    else:
        exec_.copy_from_host(d_b, np.sin(0.37 * np.arange(rows)) + 0.5)
    exec_.synchronize()
    rec = dict(matrix=name, n=args.n, rows=rows, nnz=A.non_zeros(),
               pe=args.pe if name == "cdpe" else None, repeats=args.repeats,
               warmup=args.warmup, solvers={})
    cap = max(args.iters, args.kmax)

    def solver(label):
        """-> (call(kmax, rtol, **kw) -> (k, hist, status), products per step,
        close)"""
        if label.startswith("idrs"):
            s = int(label[4:])
            ws = host.IdrsWorkspace(exec_)
            ws.reserve_timing(cap)
            return (lambda kmax, rtol, **kw: host.idrs(
                comm, exec_, A, d_b, d_x, s, kmax, rtol, ws=ws, **kw)), 1, ws
        if label == "bicgstab":
            ws = host.BicgstabWorkspace(exec_)
            ws.reserve_timing(cap)
            return (lambda kmax, rtol, **kw: host.bicgstab(
                comm, exec_, A, d_b, d_x, None, kmax, rtol, ws=ws, **kw)), 2, ws
        ws = host.GmresWorkspace(exec_)
        ws.reserve_timing(cap)
        return (lambda kmax, rtol, **kw: host.gmres(
            comm, exec_, A, d_b, d_x, 30, kmax, rtol, ws=ws, **kw)), 1, ws

    for label in ["idrs%d" % s for s in S_VALUES] + ["bicgstab", "gmres30"]:
        call, products, ws = solver(label)
        out = {}
        # ---- a fixed number of steps
        ms = timed(lambda: out.update(r=call(args.iters, 0.0)), args.repeats,
                   args.warmup)
        k = max(out["r"][0], 1)
        st = {}
        call(args.iters, 0.0, time_spmv=True, stats=st)
        spmv = st["spmv_ms_total"] / max(st["spmv_launches"], 1)
        per = min(ms) / k
        step = dict(steps=out["r"][0], status=out["r"][2], ms_per_step=per,
                    ms_per_step_med=float(np.median(ms)) / k,
                    products_per_step=products, spmv_ms=spmv,
                    nonspmv_ms_per_step=per - products * spmv)
        if label.startswith("idrs"):
            s = int(label[4:])
            nbytes = (2 * s + 11) * 8.0 * rows
            rest = per - spmv
            step.update(vector_bytes_per_inner_step=nbytes,
                        vector_bytes_per_second=nbytes / (rest * 1e-3)
                        if rest > 0 else None, launches_per_step=5)
        # ---- to rtol
        ms = timed(lambda: out.update(r=call(args.kmax, args.rtol)),
                   args.repeats, args.warmup)
        k, hist, status = out["r"]
        last = float(hist[-1] / hist[0]) if hist[0] else 0.0
        rec["solvers"][label] = dict(step=step, solve=dict(
            rtol=args.rtol, kmax=args.kmax, steps=int(k),
            products=int(k) * products, status=int(status),
            converged=bool(last < args.rtol),
            relative_residual=last if np.isfinite(last) else None,
            ms=spread(ms)))
        ws.close()
    print(json.dumps(rec), flush=True)
    for p in (d_b, d_u, d_x):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=96, help="grid edge")
    ap.add_argument("--pe", type=float, default=5.0, help="cell Peclet number")
    ap.add_argument("--iters", type=int, default=60,
                    help="steps of the fixed-length solves")
    ap.add_argument("--kmax", type=int, default=3000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma list of matrices")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "idrsbench.json"))
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:  # a child: one matrix in this process
        run_case(args.case, args)
        return 0
    names = [m for m in MATRICES
             if not args.only or m in args.only.split(",")]
    recs = []
    p = None
    for m in names:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", m]
        for key in ("n", "pe", "iters", "kmax", "rtol", "repeats", "warmup"):
            cmd += ["--" + key, str(getattr(args, key))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"idrsbench: {m} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
