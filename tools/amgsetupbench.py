"""AmgPreconditioner setup benchmark on one GPU: the host constructor next to
the device setup (AmgOptions{setup = device}) with hashed and with natural
order, per matrix in ONE process.

    python tools/amgsetupbench.py           # all cases -> profiles/amgsetup.json

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on; general storage; `--n`, default 256) and the FEM-like
matrix of `--rows` rows (general storage).

One JSON record per case and path (host, device_hashed, device_natural) with
  setup_ms           wall ms of the constructor, minimum of `--repeats` after
                     `--warmup`; of the fastest construction: symbolic_ms with
                     its device halves aggregate_ms and build_ms, numeric_ms
  host_setup_ms, setup_ratio
                     the host constructor of the same process and run, the
                     yardstick, and host over this path
  rounds             per level (pass 1, pass 3); level_rows, level_nnz,
                     operator_complexity (sum of the levels' entries over level
                     0's), plan_bytes, temp_bytes (the peak of the device
                     setup's temporaries)
  amg_apply_ms       wall ms of one amg_apply (`--apply-reps` calls, then one
                     synchronise; minimum of `--repeats`)
  iterations, ms_to_solution, converged
                     pcg_amg to `--rtol` with the object
A record is printed as soon as its path is done.  The natural order needs as
many rounds as the longest dependency chain and comes last: on a lattice in
row order it is the path that may run into the case's time limit, and the
records before it stand.

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
PATHS = (("host", dict()),
         ("device_hashed", dict(setup="device", order="hashed")),
         ("device_natural", dict(setup="device", order="natural")))


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
    ws = host.AmgPcgWorkspace(exec_)
    host_setup_ms = None
    paths = [p for p in PATHS if not args.paths or p[0] in args.paths.split(",")]
    for name, kw in paths:
        best = None
        for rep in range(args.warmup + args.repeats):
            exec_.synchronize()
            t0 = time.perf_counter()
            M = host.AmgPreconditioner(exec_, A, **kw)
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup and (best is None or ms < best[0]):
                if best is not None:
                    best[1].close()
                best = (ms, M)
            else:
                M.close()
        setup_ms, M = best
        if name == "host":
            host_setup_ms = setup_ms
        symbolic_ms, numeric_ms = M.setup_ms()
        detail = M.setup_detail()
        levels = M.levels()
        level_nnz = [M.non_zeros(l) for l in range(levels)]

        def apply_many():
            for _ in range(args.apply_reps):
                host.amg_apply(exec_, M, d_b, d_x)
            exec_.synchronize()
        apply_ms = []
        for rep in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            apply_many()
            if rep >= args.warmup:
                apply_ms.append((time.perf_counter() - t0) * 1e3 / args.apply_reps)
        sol = []
        for rep in range(2):
            exec_.synchronize()
            t0 = time.perf_counter()
            k, h = host.pcg_amg(comm, exec_, A, M, d_b, d_x, args.kmax, args.rtol,
                                ws)
            sol.append((time.perf_counter() - t0) * 1e3)
        rec = dict(case=case, path=name, rows=rows, nnz=nnz, repeats=args.repeats,
                   setup_ms=setup_ms, host_setup_ms=host_setup_ms,
                   setup_ratio=host_setup_ms / setup_ms if host_setup_ms else None,
                   symbolic_ms=symbolic_ms, aggregate_ms=detail["aggregate_ms"],
                   build_ms=detail["build_ms"], numeric_ms=numeric_ms,
                   temp_bytes=detail["temp_bytes"],
                   rounds=[M.rounds(l) for l in range(levels)],
                   level_rows=[M.rows(l) for l in range(levels)],
                   level_nnz=level_nnz,
                   operator_complexity=sum(level_nnz) / max(level_nnz[0], 1),
                   plan_bytes=M.plan_bytes(), matrix_bytes=A.format_size(),
                   amg_apply_ms=min(apply_ms), iterations=k,
                   ms_to_solution=min(sol), rtol=args.rtol,
                   final_rel_residual=float(h[-1] / h[0]),
                   converged=bool(h[-1] / h[0] < args.rtol))
        print(json.dumps(rec), flush=True)
        M.close()
    ws.close()
    for p in (d_b, d_x):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like matrix")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--apply-reps", type=int, default=10,
                    help="calls per timed window of amg_apply")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=2000,
                    help="iteration limit of the solves to rtol")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--paths", default=None, help="comma list of paths")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "amgsetup.json"))
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
               "--rows", str(args.rows), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup), "--apply-reps", str(args.apply_reps),
               "--rtol", str(args.rtol), "--kmax", str(args.kmax)]
        if args.paths:
            cmd += ["--paths", args.paths]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"amgsetupbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
