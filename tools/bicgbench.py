"""bicgstab benchmark on one GPU: cg() with defer_x = False against
bicgstab() with the Jacobi dinv and without a dinv, on the same matrix, per
case in ONE process.

    python tools/bicgbench.py                # all cases -> profiles/bicgstab.json

Fixed-length cases (rtol = 0, `--iters` iterations, any right-hand side): the
7-point Poisson matrix on n^3 points in CSR order (lattice analysis off,
csr_in_place on) and the FEM-like matrix of `--rows` rows, general storage.
(Both are symmetric: a fixed number of iterations costs what it costs on any
matrix of the same pattern, and cg() needs one to run on.)
One JSON record per case: wall ms per iteration of the three solvers on a
reused workspace (minimum and median of `--repeats` repeats after `--warmup`
untimed ones, every solve ended by its own synchronisation) and -- from one
more solve of each with CgOptions::time_spmv -- the SpMVs' share, so that the
rest can be held against the pass model: an iteration of bicgstab is 2 SpMVs
plus 23 vector passes with a dinv and 18 without, where this cg() path is 1
SpMV plus 8, so the non-SpMV time should be near 23 / 8 and 18 / 8 of cg()'s.

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

CASES = ("poisson_csr", "fem_like")
PASSES = {"cg": 8, "bicgstab_jacobi": 23, "bicgstab": 18}


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
        A = host.Matrix.create_fem_like(comm, exec_, args.rows)
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
    it = args.iters
    ws_cg, ws_bi = host.CgWorkspace(exec_), host.BicgstabWorkspace(exec_)
    ws_cg.reserve_timing(it), ws_bi.reserve_timing(it)
    state = {}

    def cg(time_spmv=False):
        k, _, ms, n = host.cg_ex(comm, exec_, A, d_b, d_x, it, 0.0, ws_cg,
                                 time_spmv=time_spmv, defer_x=False)
        state["cg"] = (k, 0, ms, n)

    def bicg(dinv, name, time_spmv=False):
        st = {}
        k, _, status = host.bicgstab(comm, exec_, A, d_b, d_x, dinv, it, 0.0,
                                     ws_bi, time_spmv=time_spmv, stats=st)
        state[name] = (k, status, st["spmv_ms_total"], st["spmv_launches"])

    solvers = {"cg": cg,
               "bicgstab_jacobi": lambda t=False: bicg(d_dinv, "bicgstab_jacobi", t),
               "bicgstab": lambda t=False: bicg(None, "bicgstab", t)}
    rec = dict(case=case, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               plan_forms=forms, passes=PASSES)
    for name, fn in solvers.items():
        ms = timed(fn, args.repeats, args.warmup)
        fn(True)  # the SpMVs' share: one solve with the events in
        k, status, spmv_ms, launches = state[name]
        assert k == it and status == 0, (name, k, status)
        per_it = min(ms) / it
        rec[name] = dict(ms_per_iter=per_it,
                         ms_per_iter_med=float(np.median(ms)) / it,
                         spmv_ms_per_iter=spmv_ms / it,
                         spmv_per_iter=launches / it,
                         nonspmv_ms_per_iter=per_it - spmv_ms / it)
    base = rec["cg"]
    for name in ("bicgstab_jacobi", "bicgstab"):
        r = rec[name]
        r["ratio_vs_cg"] = r["ms_per_iter"] / base["ms_per_iter"]
        r["spmv_ratio_vs_cg"] = r["spmv_ms_per_iter"] / base["spmv_ms_per_iter"]
        r["nonspmv_ratio_vs_cg"] = (r["nonspmv_ms_per_iter"]
                                    / base["nonspmv_ms_per_iter"])
        r["nonspmv_ratio_expected"] = PASSES[name] / PASSES["cg"]
    print(json.dumps(rec), flush=True)
    ws_cg.close(), ws_bi.close()
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
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "bicgstab.json"))
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
               "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"bicgbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
