"""pcg_sgs benchmark on one GPU: pcg() with the Jacobi preconditioner,
pcg_chebyshev() at degree 4 and pcg_sgs() on the same matrix, per case in ONE
process.

    python tools/sgsbench.py                # all cases -> profiles/sgsbench.json

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on; general storage) and the FEM-like matrix of `--rows` rows
in general storage.  The Chebyshev bounds are the advised ones: lmax = 1.1 *
lambda_max_estimate(20 steps from the right-hand side), lmin = lmax / 30.

One JSON record per case with, for every solver,
  ms_per_iter        wall ms per iteration of a fixed-length solve (rtol = 0,
                     `--iters` iterations; minimum of `--repeats` repeats after
                     `--warmup` untimed ones on a reused workspace)
  iterations, ms_to_solution, converged
                     of a solve to `--rtol` (limit `--kmax`)
and for the preconditioner itself
  colors, plan_bytes, setup_ms (the constructor: read-back, colouring and
  reordering on the host, upload), launches_per_apply = 2 * colors - 1,
  sgs_apply_ms next to mult_ms: wall ms of one sgs_apply and of one
  Matrix::mult of the same matrix (`--apply-reps` calls, then one synchronise;
  minimum of `--repeats`).
The model to hold sgs_apply_ms against: an application reads every entry of the
local block once (12 bytes per stored entry and its padding) plus perm, dinv, r
and z -- about the bytes of one SpMV -- in 2 * colors - 1 launches.

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
DEGREE = 4


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
        # the caller's CSR arrays as they are (tools/cgbbench.py)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 1 << 62)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"csr_in_place", 1)
        A = host.Matrix.create_poisson3d(comm, exec_, args.n, False,
                                         host.P2P_BLOCKING)
    else:
        A = host.Matrix.create_fem_like(comm, exec_, args.rows, symmetric=False)
    rows, nnz = A.rows(), A.non_zeros()
    forms = {key: A.plan_get(key) for key in ("lat", "lx", "xw", "sjds", "sdia",
                                              "wdia")}
    d_dinv = exec_.alloc(rows)
    A.diagonal(d_dinv)
    host.jacobi_inverse(exec_, d_dinv, d_dinv, rows)
    d_b, d_x = exec_.alloc(rows), exec_.alloc(rows)
    _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, rows, 0, rows, d_b,
              None)
    exec_.synchronize()
    t0 = time.perf_counter()
    M = host.SgsPreconditioner(exec_, A, values=args.values)
    setup_ms = (time.perf_counter() - t0) * 1e3
    estimate = host.lambda_max_estimate(comm, exec_, A, d_dinv, d_b, 20)
    lmax = 1.1 * estimate
    lmin = lmax / 30
    ws_pcg, ws_ch = host.PcgWorkspace(exec_), host.ChebyshevWorkspace(exec_)
    ws_sgs = host.SgsWorkspace(exec_)

    # the application next to one SpMV of the same matrix
    def apply_many():
        for _ in range(args.apply_reps):
            host.sgs_apply(exec_, M, d_b, d_x)
        exec_.synchronize()

    def mult_many():
        for _ in range(args.apply_reps):
            A.mult(d_b, d_x)
        exec_.synchronize()

    apply_ms = min(timed(apply_many, args.repeats, args.warmup)) / args.apply_reps
    fp64 = {}
    if args.values == "fp32":  # the fp64 object next to it, in this process
        M32, M = M, host.SgsPreconditioner(exec_, A)
        fp64 = dict(sgs_apply_ms_fp64=min(timed(apply_many, args.repeats,
                                                args.warmup)) / args.apply_reps,
                    plan_bytes_fp64=M.plan_bytes())
        M.close()
        M = M32
    mult_ms = min(timed(mult_many, args.repeats, args.warmup)) / args.apply_reps

    def pcg(kmax, rtol):
        return host.pcg(comm, exec_, A, d_b, d_x, d_dinv, kmax, rtol, ws_pcg)

    def cheb(kmax, rtol):
        return host.pcg_chebyshev(comm, exec_, A, d_b, d_x, d_dinv, DEGREE, lmin,
                                  lmax, kmax, rtol, ws_ch)

    def sgs(kmax, rtol):
        return host.pcg_sgs(comm, exec_, A, M, d_b, d_x, kmax, rtol, ws_sgs)

    out = {}
    it = args.iters
    for name, solve in (("pcg", pcg), (f"chebyshev{DEGREE}", cheb),
                        ("pcg_sgs", sgs)):
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
    colors = M.num_colors()
    rec = dict(case=case, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               rtol=args.rtol, kmax=args.kmax, lmin=lmin, lmax=lmax,
               colors=colors, launches_per_apply=2 * colors - 1,
               plan_bytes=M.plan_bytes(), matrix_bytes=A.format_size(),
               setup_ms=setup_ms, sgs_apply_ms=apply_ms, mult_ms=mult_ms,
               solvers=out, plan_forms=forms, values=args.values,
               value_bits=M.value_bits, **fp64)
    print(json.dumps(rec), flush=True)
    ws_pcg.close(), ws_ch.close(), ws_sgs.close()
    M.close()
    for p in (d_dinv, d_b, d_x):
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
                    help="calls per timed window of sgs_apply / mult")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=5000,
                    help="iteration limit of the solves to rtol")
    ap.add_argument("--values", choices=("fp64", "fp32"), default="fp64",
                    help="width of the sweep plan's values; fp32 also times "
                         "the fp64 object's sgs_apply in the same process")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "sgsbench.json"))
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
               os.path.abspath(__file__), "--case", case, "--n", str(args.n),
               "--rows", str(args.rows), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--apply-reps", str(args.apply_reps), "--rtol", str(args.rtol),
               "--kmax", str(args.kmax), "--values", args.values]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"sgsbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
