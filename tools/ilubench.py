"""Ilu0Preconditioner benchmark on one GPU: the device factorisation next to
what it competes with, per case in ONE process.

    python tools/ilubench.py                # all cases -> profiles/ilubench.json

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on; general storage) and the FEM-like matrix of `--rows` rows
in general storage (tools/sgsbench.py's cases).

One JSON record per case with
  colors, plan_bytes (ILU(0): sweep plan + working copy + maps) next to
  sgs_plan_bytes, matrix_bytes
  setup_ms           the Ilu0Preconditioner constructor, wall; symbolic_ms (host:
                     read-back of the pattern, colouring, parts, slots, upload)
                     and numeric_ms (device: gather, C - 1 factor launches,
                     finish, scatter, the read of the pivot counts)
  refactor_ms        wall ms of one refactor(A) (it ends with the read of the
                     counts, so it is synchronised; minimum of `--repeats`)
  sgs_setup_ms       one SgsPreconditioner construction of the same matrix
  mult_ms, ilu0_apply_ms, sgs_apply_ms
                     wall ms of one Matrix::mult, one ilu0_apply and one
                     sgs_apply (`--apply-reps` calls, then one synchronise;
                     minimum of `--repeats`); the two applications run the same
                     kernel on the same bytes
  solvers            pcg_sgs with each preconditioner: ms_per_iter of a
                     fixed-length solve (rtol = 0, `--iters` iterations) and
                     iterations / ms_to_solution of a solve to `--rtol`
The model to hold refactor_ms against: the gather and the scatter stream every
factor entry twice (about 2 x 28 bytes per entry); the factor launches read, per
row i, the finished rows of before(i) -- on a 7-point stencil 6 rows of 6
entries for one useful subtraction each, one wavefront per row.

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("poisson_csr", "fem_like")


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
    from spmv_amd import _lib, host
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    if case == "poisson_csr":
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 1 << 62)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"csr_in_place", 1)
        A = host.Matrix.create_poisson3d(comm, exec_, args.n, False,
                                         host.P2P_BLOCKING)
    else:
        A = host.Matrix.create_fem_like(comm, exec_, args.rows, symmetric=False)
    rows, nnz = A.rows(), A.non_zeros()
    d_b, d_x = exec_.alloc(rows), exec_.alloc(rows)
    _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, rows, 0, rows, d_b,
              None)
    exec_.synchronize()
    t0 = time.perf_counter()
    M = host.Ilu0Preconditioner(exec_, A, values=args.values)
    setup_ms = (time.perf_counter() - t0) * 1e3
    symbolic_ms, numeric_ms = M.setup_ms()
    refactor_ms = min(timed(lambda: M.refactor(A), args.repeats, args.warmup))
    t0 = time.perf_counter()
    S = host.SgsPreconditioner(exec_, A, values=args.values)
    sgs_setup_ms = (time.perf_counter() - t0) * 1e3

    def many(fn):
        def run():
            for _ in range(args.apply_reps):
                fn()
            exec_.synchronize()
        return min(timed(run, args.repeats, args.warmup)) / args.apply_reps

    mult_ms = many(lambda: A.mult(d_b, d_x))
    ilu0_apply_ms = many(lambda: host.ilu0_apply(exec_, M, d_b, d_x))
    sgs_apply_ms = many(lambda: host.sgs_apply(exec_, S, d_b, d_x))

    ws = host.SgsWorkspace(exec_)
    out = {}
    it = args.iters
    for name, pre in (("pcg_sgs_sgs", S), ("pcg_sgs_ilu0", M)):
        def solve(kmax, rtol, pre=pre):
            return host.pcg_sgs(comm, exec_, A, pre, d_b, d_x, kmax, rtol, ws)
        ms = timed(lambda: solve(it, 0.0), args.repeats, args.warmup)
        k, _ = solve(it, 0.0)
        assert k == it, (name, k)
        state = {}

        def to_solution():
            state["k"], state["h"] = solve(args.kmax, args.rtol)
        ms_sol = timed(to_solution, 2, 1)
        h = state["h"]
        out[name] = dict(ms_per_iter=min(ms) / it, iterations=state["k"],
                         ms_to_solution=min(ms_sol),
                         final_rel_residual=float(h[-1] / h[0]),
                         converged=bool(h[-1] / h[0] < args.rtol))
    rec = dict(case=case, values=args.values, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               rtol=args.rtol, kmax=args.kmax, colors=M.num_colors(),
               negative_pivots=M.negative_pivots(), plan_bytes=M.plan_bytes(),
               sgs_plan_bytes=S.plan_bytes(), matrix_bytes=A.format_size(),
               setup_ms=setup_ms, symbolic_ms=symbolic_ms, numeric_ms=numeric_ms,
               refactor_ms=refactor_ms, sgs_setup_ms=sgs_setup_ms,
               mult_ms=mult_ms, ilu0_apply_ms=ilu0_apply_ms,
               sgs_apply_ms=sgs_apply_ms, solvers=out)
    print(json.dumps(rec), flush=True)
    ws.close()
    M.close(), S.close()
    for p in (d_b, d_x):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like matrix")
    ap.add_argument("--iters", type=int, default=20, help="iterations per solve")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--apply-reps", type=int, default=10,
                    help="calls per timed window of the applications / mult")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=5000,
                    help="iteration limit of the solves to rtol")
    ap.add_argument("--values", choices=("fp64", "fp32"), default="fp64",
                    help="width of the sweep plans' values")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "ilubench.json"))
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
               os.path.abspath(__file__), "--case", case, "--values", args.values,
               "--n", str(args.n),
               "--rows", str(args.rows), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--apply-reps", str(args.apply_reps), "--rtol", str(args.rtol),
               "--kmax", str(args.kmax)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"ilubench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
