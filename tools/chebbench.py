"""pcg_chebyshev benchmark on one GPU: cg() with defer_x = False, pcg() with the
Jacobi preconditioner and pcg_chebyshev() at degrees 2, 4 and 8 on the same
matrix, per case in ONE process.

    python tools/chebbench.py                # all cases -> profiles/chebbench.json

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on; general storage) and the FEM-like matrix of `--rows` rows
in symmetric storage (lower part and diagonal: symmetric positive definite).
The Chebyshev bounds are the advised ones: lmax = 1.1 * lambda_max_estimate(20
steps from the right-hand side), lmin = lmax / 30.

One JSON record per case with, for every solver,
  ms_per_iter        wall ms per iteration of a fixed-length solve (rtol = 0,
                     `--iters` iterations; minimum of `--repeats` repeats after
                     `--warmup` untimed ones on a reused workspace)
  spmv_ms_per_iter   the SpMVs' share, from one more solve with
                     CgOptions::time_spmv (pcg_chebyshev: all `degree` of them)
  iterations, ms_to_solution, converged
                     of a solve to `--rtol` (limit `--kmax`)
and the pass model to hold them against: an iteration of pcg_chebyshev is
`degree` SpMVs + 7 (degree - 1) + 11 vector passes with a dinv, where pcg()
streams 1 SpMV + 10 and this cg() path 1 SpMV + 8.

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

CASES = ("poisson_csr", "fem_like_sym")
DEGREES = (2, 4, 8)


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
        A = host.Matrix.create_fem_like(comm, exec_, args.rows, symmetric=True)
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
    estimate = host.lambda_max_estimate(comm, exec_, A, d_dinv, d_b, 20)
    estimate_ms = (time.perf_counter() - t0) * 1e3
    lmax = 1.1 * estimate
    lmin = lmax / 30
    ws_cg, ws_pcg = host.CgWorkspace(exec_), host.PcgWorkspace(exec_)
    ws_ch = host.ChebyshevWorkspace(exec_)
    ws_cg.reserve_timing(args.iters), ws_pcg.reserve_timing(args.iters)
    ws_ch.reserve_timing(args.iters * max(DEGREES))

    def cg(kmax, rtol, time_spmv=False):
        k, h, ms, _ = host.cg_ex(comm, exec_, A, d_b, d_x, kmax, rtol, ws_cg,
                                 time_spmv=time_spmv, defer_x=False, history=True)
        return k, h, ms

    def pcg(kmax, rtol, time_spmv=False):
        st = {}
        k, h = host.pcg(comm, exec_, A, d_b, d_x, d_dinv, kmax, rtol, ws_pcg,
                        time_spmv=time_spmv, stats=st)
        return k, h, st["spmv_ms_total"]

    def cheb(degree):
        def solve(kmax, rtol, time_spmv=False):
            st = {}
            k, h = host.pcg_chebyshev(comm, exec_, A, d_b, d_x, d_dinv, degree,
                                      lmin, lmax, kmax, rtol, ws_ch,
                                      time_spmv=time_spmv, stats=st)
            return k, h, st["spmv_ms_total"]
        return solve

    solvers = [("cg", cg, 1, 8), ("pcg", pcg, 1, 10)]
    solvers += [(f"chebyshev{d}", cheb(d), d, 7 * (d - 1) + 11) for d in DEGREES]
    out = {}
    it = args.iters
    for name, solve, spmvs, passes in solvers:
        ms = timed(lambda: solve(it, 0.0), args.repeats, args.warmup)
        k, _, spmv_ms = solve(it, 0.0, True)
        assert k == it, (name, k)
        state = {}

        def to_solution():
            state["k"], state["h"], _ = solve(args.kmax, args.rtol)
        ms_sol = timed(to_solution, 2, 1)
        h = state["h"]
        out[name] = dict(spmvs_per_iter=spmvs, vector_passes_per_iter=passes,
                         ms_per_iter=min(ms) / it,
                         spmv_ms_per_iter=spmv_ms / it,
                         nonspmv_ms_per_iter=min(ms) / it - spmv_ms / it,
                         iterations=state["k"], ms_to_solution=min(ms_sol),
                         final_rel_residual=float(h[-1] / h[0]),
                         converged=bool(h[-1] / h[0] < args.rtol))
    rec = dict(case=case, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               rtol=args.rtol, kmax=args.kmax, lambda_max_estimate=estimate,
               lambda_max_estimate_ms=estimate_ms, lmin=lmin, lmax=lmax,
               solvers=out, plan_forms=forms)
    print(json.dumps(rec), flush=True)
    ws_cg.close(), ws_pcg.close(), ws_ch.close()
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
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=5000,
                    help="iteration limit of the solves to rtol")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "chebbench.json"))
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
               "--rtol", str(args.rtol), "--kmax", str(args.kmax)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"chebbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
