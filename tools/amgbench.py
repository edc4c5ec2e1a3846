"""AmgPreconditioner benchmark on one GPU: the V-cycle next to what it competes
with, per case in ONE process.

    python tools/amgbench.py                # all cases -> profiles/amgbench.json

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on; general storage) and the FEM-like matrix of `--rows` rows
in general storage (tools/ilubench.py's cases).

One JSON record per case with
  levels             rows and stored entries of every level, operator
                     complexity (entries of all levels / entries of level 0),
                     lmax per level; plan_bytes next to matrix_bytes
  setup_ms           the AmgPreconditioner constructor, wall; symbolic_ms (host:
                     read-back, aggregates, patterns, source lists, uploads) and
                     numeric_ms (device: Galerkin sums, the coarse blocks' plans,
                     diagonals and bounds, the read-backs between the levels)
  refresh_ms         wall ms of one refresh(A) (it ends with the read of the
                     counts, so it is synchronised; minimum of `--repeats`)
  mult_ms, amg_apply_ms, sgs_apply_ms
                     wall ms of one Matrix::mult, one amg_apply and one
                     sgs_apply (`--apply-reps` calls, then one synchronise;
                     minimum of `--repeats`)
  launches_per_apply kernels and copies of one application, counted from the
                     definition: per level that is not the coarsest 2 s + 1
                     products, 2 s Chebyshev launches, restrict and prolong; on
                     the coarsest 2 coarse_degree - 1; one copy out
  coarse_apply_ms    amg_apply of a hierarchy built on the matrix of level 1
                     alone: the share of an application spent below the finest
                     level, where the launches are small
  tail               with --tail-rows (a comma list, 0 = off): per value, on the
                     SAME object in the same process and with the same repeats,
                     tail_levels, launches_per_apply (the tail's launches taken
                     off, its one launch added), amg_apply_ms and
                     pcg_amg_ms_per_iter, each as {min, median, max} of the
                     repeats.  The yardstick is the line of 0 of the same run
  solvers            cg, pcg_sgs, pcg_amg at coarse_scale 1.0 and 1.6:
                     ms_per_iter of a fixed-length solve (rtol = 0, `--iters`
                     iterations) and iterations / ms_to_solution to `--rtol`

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.  It is a
measurement, not a test, and gates nothing.
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
    M = host.AmgPreconditioner(exec_, A)
    setup_ms = (time.perf_counter() - t0) * 1e3
    symbolic_ms, numeric_ms = M.setup_ms()
    refresh_ms = min(timed(lambda: M.refresh(A), args.repeats, args.warmup))
    M16 = host.AmgPreconditioner(exec_, A, coarse_scale=1.6)
    S = host.SgsPreconditioner(exec_, A)
    nl = M.levels()
    levels = [dict(rows=M.rows(l), entries=M.non_zeros(l), lmax=M.lmax(l))
              for l in range(nl)]
    s, c = M.options["smooth_degree"], M.options["coarse_degree"]
    launches = (nl - 1) * ((2 * s + 1) + 2 * s + 2) + (2 * c - 1) + 1

    def spread(ms):
        ms = sorted(ms)
        return dict(min=ms[0], median=ms[len(ms) // 2], max=ms[-1])

    def many_all(fn):
        """ms per call of every repeat"""
        def run():
            for _ in range(args.apply_reps):
                fn()
            exec_.synchronize()
        return [v / args.apply_reps
                for v in timed(run, args.repeats, args.warmup)]

    def many(fn):
        return min(many_all(fn))

    mult_ms = many(lambda: A.mult(d_b, d_x))
    amg_apply_ms = many(lambda: host.amg_apply(exec_, M, d_b, d_x))
    sgs_apply_ms = many(lambda: host.sgs_apply(exec_, S, d_b, d_x))
    coarse_apply_ms = None
    if nl > 1:  # the hierarchy below the finest level, on its own
        rp, ci, va = M.level_matrix(1)
        n1 = M.rows(1)
        A1 = host.Matrix.create_matrix(comm, exec_, rp, ci, va, n1, n1, [], [],
                                       False, host.P2P_BLOCKING)
        M1 = host.AmgPreconditioner(exec_, A1)
        coarse_apply_ms = many(lambda: host.amg_apply(exec_, M1, d_b, d_x))
        M1.close()
        A1.close()

    ws = host.AmgPcgWorkspace(exec_)
    cws = host.CgWorkspace(exec_)
    solvers = {
        "cg": lambda kmax, rtol: host.cg_ex(comm, exec_, A, d_b, d_x, kmax, rtol,
                                            cws, history=True)[:2],
        "pcg_sgs": lambda kmax, rtol: host.pcg_sgs(comm, exec_, A, S, d_b, d_x,
                                                   kmax, rtol, ws),
        "pcg_amg_1.0": lambda kmax, rtol: host.pcg_amg(comm, exec_, A, M, d_b,
                                                       d_x, kmax, rtol, ws),
        "pcg_amg_1.6": lambda kmax, rtol: host.pcg_amg(comm, exec_, A, M16, d_b,
                                                       d_x, kmax, rtol, ws),
    }
    out = {}
    it = args.iters
    for name, solve in solvers.items():
        ms = timed(lambda: solve(it, 0.0), args.repeats, args.warmup)
        state = {}

        def to_solution():
            state["k"], state["h"] = solve(args.kmax, args.rtol)
        ms_sol = timed(to_solution, 2, 1)
        h = state["h"]
        out[name] = dict(ms_per_iter=min(ms) / it, iterations=state["k"],
                         ms_to_solution=min(ms_sol),
                         final_rel_residual=float(h[-1] / h[0]),
                         converged=bool(h[-1] / h[0] < args.rtol))
    tail = []
    for tail_rows in args.tail_rows:
        M.set_tail_rows(tail_rows)
        tl = M.tail_levels()
        t = nl - tl
        saved = (nl - 1 - t) * (4 * s + 3) + (2 * c - 1) - 1 if tl else 0
        tail.append(dict(
            tail_rows=tail_rows, tail_levels=tl,
            launches_per_apply=launches - saved,
            amg_apply_ms=spread(
                many_all(lambda: host.amg_apply(exec_, M, d_b, d_x))),
            pcg_amg_ms_per_iter=spread(
                [v / it for v in timed(lambda: solvers["pcg_amg_1.0"](it, 0.0),
                                       args.repeats, args.warmup)])))
    M.set_tail_rows(0)
    rec = dict(case=case, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               rtol=args.rtol, kmax=args.kmax, levels=levels,
               operator_complexity=sum(v["entries"] for v in levels) / max(nnz, 1),
               plan_bytes=M.plan_bytes(), matrix_bytes=A.format_size(),
               setup_ms=setup_ms, symbolic_ms=symbolic_ms, numeric_ms=numeric_ms,
               refresh_ms=refresh_ms, launches_per_apply=launches,
               mult_ms=mult_ms, amg_apply_ms=amg_apply_ms,
               sgs_apply_ms=sgs_apply_ms, coarse_apply_ms=coarse_apply_ms,
               solvers=out, tail=tail)
    print(json.dumps(rec), flush=True)
    ws.close()
    cws.close()
    M.close(), M16.close(), S.close()
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
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--tail-rows", default="",
                    type=lambda v: [int(x) for x in v.split(",") if x != ""],
                    help="comma list of set_tail_rows settings to time, 0 = off")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "amgbench.json"))
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
               "--kmax", str(args.kmax), "--tail-rows",
               ",".join(str(v) for v in args.tail_rows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"amgbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
