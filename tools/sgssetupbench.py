"""SgsPreconditioner setup benchmark on one GPU: the host constructor next to
the device setup (SgsOptions{setup = device}) with hashed and with natural
order, per matrix in ONE process.

    python tools/sgssetupbench.py           # all cases -> profiles/sgssetup.json

Cases: the FEM-like matrix of `--rows` rows in general and in symmetric storage
(fem_like, fem_like_sym) and the 7-point Poisson matrix on n^3 points in CSR
order (lattice analysis off, csr_in_place on; general storage; `--n`, default
256 -- at 512 the host baseline alone takes about 24 s per construction).

One JSON record per case and path (host, device_hashed, device_natural) with
  setup_ms           wall ms of the constructor, minimum of `--repeats` after
                     `--warmup`; color_ms / build_ms: its two halves on the
                     device path (of the fastest construction)
  rounds, colors, plan_bytes, temp_bytes (peak of the device setup's
                     temporaries, spmv_tmap_build's own included by formula)
  sgs_apply_ms       wall ms of one sgs_apply (`--apply-reps` calls, then one
                     synchronise; minimum of `--repeats`)
  iterations, ms_to_solution, converged
                     pcg_sgs to `--rtol` with the object
A record is printed as soon as its path is done.  The natural order needs as
many rounds as the longest ascending path of the pattern and comes last: on a
matrix with long dependency chains it is the path that may run into the case's
time limit, and the records before it stand.

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.

    python tools/sgssetupbench.py --ilu0    # -> profiles/ilu0setup.json

measures Ilu0Preconditioner the same way: the host constructor (symbolic work
on the host from the pattern read back) next to the device setup.  Its records
add symbolic_ms (colouring + build, the part the two paths differ in) and
numeric_ms (the factorisation, the same kernels on both paths) of the fastest
construction, host_symbolic_ms and symbolic_ratio (host over this path, same
process and run), and negative_pivots; sgs_apply_ms is ilu0_apply; a factor
with negative pivots is not handed to pcg_sgs (iterations null).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("fem_like", "fem_like_sym", "poisson_csr")
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
        A = host.Matrix.create_fem_like(comm, exec_, args.rows,
                                        symmetric=case == "fem_like_sym")
    rows, nnz = A.rows(), A.non_zeros()
    d_b, d_x = exec_.alloc(rows), exec_.alloc(rows)
    _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, rows, 0, rows, d_b,
              None)
    exec_.synchronize()
    ws = host.SgsWorkspace(exec_)
    make = host.Ilu0Preconditioner if args.ilu0 else host.SgsPreconditioner
    host_symbolic_ms = None
    paths = [p for p in PATHS if not args.paths or p[0] in args.paths.split(",")]
    for name, kw in paths:
        best = None
        for rep in range(args.warmup + args.repeats):
            exec_.synchronize()
            t0 = time.perf_counter()
            M = make(exec_, A, **kw)
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup and (best is None or ms < best[0]):
                if best is not None:
                    best[1].close()
                best = (ms, M)
            else:
                M.close()
        setup_ms, M = best
        detail = M.setup_detail()

        def apply_many():
            for _ in range(args.apply_reps):
                host.sgs_apply(exec_, M, d_b, d_x)
            exec_.synchronize()
        apply_ms = []
        for rep in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            apply_many()
            if rep >= args.warmup:
                apply_ms.append((time.perf_counter() - t0) * 1e3 / args.apply_reps)
        sol, k, h = [], None, None
        for rep in range(0 if args.ilu0 and M.negative_pivots() else 2):
            exec_.synchronize()
            t0 = time.perf_counter()
            k, h = host.pcg_sgs(comm, exec_, A, M, d_b, d_x, args.kmax, args.rtol,
                                ws)
            sol.append((time.perf_counter() - t0) * 1e3)
        extra = dict(object_setup_ms=M.setup_ms())
        if args.ilu0:
            symbolic_ms, numeric_ms = M.setup_ms()
            if name == "host":
                host_symbolic_ms = symbolic_ms
            extra = dict(symbolic_ms=symbolic_ms, numeric_ms=numeric_ms,
                         host_symbolic_ms=host_symbolic_ms,
                         symbolic_ratio=(host_symbolic_ms / symbolic_ms
                                         if host_symbolic_ms else None),
                         negative_pivots=M.negative_pivots())
        rec = dict(case=case, path=name, rows=rows, nnz=nnz, repeats=args.repeats,
                   setup_ms=setup_ms, **extra,
                   color_ms=detail["color_ms"], build_ms=detail["build_ms"],
                   temp_bytes=detail["temp_bytes"], rounds=M.rounds(),
                   colors=M.num_colors(), plan_bytes=M.plan_bytes(),
                   matrix_bytes=A.format_size(), sgs_apply_ms=min(apply_ms),
                   iterations=k, ms_to_solution=min(sol) if sol else None,
                   rtol=args.rtol,
                   final_rel_residual=float(h[-1] / h[0]) if sol else None,
                   converged=bool(h[-1] / h[0] < args.rtol) if sol else None)
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--apply-reps", type=int, default=10,
                    help="calls per timed window of sgs_apply")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=5000,
                    help="iteration limit of the solves to rtol")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--paths", default=None, help="comma list of paths")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per case")
    ap.add_argument("--ilu0", action="store_true",
                    help="measure Ilu0Preconditioner (-> profiles/ilu0setup.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ilu0setup.json" if args.ilu0
                                else "sgssetup.json")
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
        if args.ilu0:
            cmd += ["--ilu0"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"sgssetupbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
