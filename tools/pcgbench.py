"""pcg benchmark on one GPU: cg() with defer_x = False against pcg() with the
Jacobi preconditioner on the same matrix, per case in ONE process.

    python tools/pcgbench.py                 # all cases -> profiles/pcgbench.json

Fixed-length cases (rtol = 0, `--iters` iterations, any right-hand side): the
7-point Poisson matrix on n^3 points in CSR order (lattice analysis off,
csr_in_place on) and the FEM-like matrix of `--rows` rows, general storage.
One JSON record per case: wall ms per iteration of either solver on a reused
workspace (minimum and median of `--repeats` repeats after `--warmup` untimed
ones, every solve ended by its own synchronisation), their ratio, and -- from
one more solve of each with CgOptions::time_spmv -- the SpMV's share, so that
the rest can be held against the pass count: pcg streams 10 vector passes per
iteration beside the SpMV where this cg() path streams 8, so
nonspmv_ratio_pcg_vs_cg should be near 10 / 8.

Scaled case: the FEM-like matrix of `--scaled-rows` rows (numpy twin,
spmv_amd.poisson.fem_like_csr) scaled to S A S, S = diag(10^u), u uniform in
[-1, 1], in symmetric storage (lower part and diagonal: symmetric positive
definite); iterations to `--rtol` and wall time to solution of cg() with its
default options and of pcg().

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

CASES = ("poisson_csr", "fem_like", "fem_like_scaled")


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


def jacobi_dinv(host, exec_, A, rows):
    d = exec_.alloc(rows)
    A.diagonal(d)
    host.jacobi_inverse(exec_, d, d, rows)
    return d


def run_fixed(case, args):
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
    d_dinv = jacobi_dinv(host, exec_, A, rows)
    d_b, d_x = exec_.alloc(rows), exec_.alloc(rows)
    _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, rows, 0, rows, d_b,
              None)
    exec_.synchronize()
    ws_cg, ws_pcg = host.CgWorkspace(exec_), host.PcgWorkspace(exec_)
    ws_cg.reserve_timing(args.iters), ws_pcg.reserve_timing(args.iters)
    state = {}

    def cg(time_spmv=False):
        k, _, ms, _ = host.cg_ex(comm, exec_, A, d_b, d_x, args.iters, 0.0, ws_cg,
                                 time_spmv=time_spmv, defer_x=False)
        state["cg"] = (k, ms)

    def pcg(time_spmv=False):
        st = {}
        k, _ = host.pcg(comm, exec_, A, d_b, d_x, d_dinv, args.iters, 0.0, ws_pcg,
                        time_spmv=time_spmv, stats=st)
        state["pcg"] = (k, st["spmv_ms_total"])

    ms_cg = timed(cg, args.repeats, args.warmup)
    ms_pcg = timed(pcg, args.repeats, args.warmup)
    # the SpMV's share: one solve each with the events in (their wall time is
    # not used)
    t0 = time.perf_counter()
    cg(True)
    wall_cg_t = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pcg(True)
    wall_pcg_t = (time.perf_counter() - t0) * 1e3
    assert state["cg"][0] == args.iters and state["pcg"][0] == args.iters
    it = args.iters
    cg_it, pcg_it = min(ms_cg) / it, min(ms_pcg) / it
    cg_spmv, pcg_spmv = state["cg"][1] / it, state["pcg"][1] / it
    rec = dict(case=case, rows=rows, nnz=nnz, iters=it, repeats=args.repeats,
               cg_ms_per_iter=cg_it, cg_ms_per_iter_med=float(np.median(ms_cg)) / it,
               pcg_ms_per_iter=pcg_it,
               pcg_ms_per_iter_med=float(np.median(ms_pcg)) / it,
               ratio_pcg_vs_cg=pcg_it / cg_it,
               cg_spmv_ms_per_iter=cg_spmv, pcg_spmv_ms_per_iter=pcg_spmv,
               cg_nonspmv_ms_per_iter=cg_it - cg_spmv,
               pcg_nonspmv_ms_per_iter=pcg_it - pcg_spmv,
               nonspmv_ratio_pcg_vs_cg=(pcg_it - pcg_spmv) / (cg_it - cg_spmv),
               nonspmv_ratio_expected=10 / 8,
               timed_solve_wall_ms=dict(cg=wall_cg_t, pcg=wall_pcg_t),
               plan_forms=forms)
    print(json.dumps(rec), flush=True)
    ws_cg.close(), ws_pcg.close()
    for p in (d_dinv, d_b, d_x):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def run_scaled(args):
    from spmv_amd import host, poisson
    rows = args.scaled_rows
    rp, ci, va = poisson.fem_like_csr(rows)
    s = 10.0 ** np.random.default_rng(rows).uniform(-1, 1, rows)
    va = va * (s[np.repeat(np.arange(rows), np.diff(rp))] * s[ci])
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    # symmetric storage keeps the lower part and the diagonal of the rows given
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, rows, rows, [], [],
                                  True, host.P2P_BLOCKING)
    del rp, ci, va
    d_dinv = jacobi_dinv(host, exec_, A, rows)
    d_b, d_x = exec_.alloc(rows), exec_.alloc(rows)
    exec_.copy_from_host(d_b, np.random.default_rng(1).uniform(-1, 1, rows))
    ws_cg, ws_pcg = host.CgWorkspace(exec_), host.PcgWorkspace(exec_)
    state = {}

    def cg():
        k, h, _, _ = host.cg_ex(comm, exec_, A, d_b, d_x, args.kmax, args.rtol,
                                ws_cg, history=True)
        state["cg"] = (k, h[-1] / h[0])

    def pcg():
        k, h = host.pcg(comm, exec_, A, d_b, d_x, d_dinv, args.kmax, args.rtol,
                        ws_pcg)
        state["pcg"] = (k, h[-1] / h[0])

    ms_cg = timed(cg, 2, 1)
    ms_pcg = timed(pcg, 2, 1)
    (k_cg, rel_cg), (k_pcg, rel_pcg) = state["cg"], state["pcg"]
    rec = dict(case="fem_like_scaled", rows=rows, nnz=A.non_zeros(),
               storage="symmetric", rtol=args.rtol, kmax=args.kmax,
               cg_iterations=k_cg, cg_converged=bool(rel_cg < args.rtol),
               cg_final_rel_residual=rel_cg, cg_ms_to_solution=min(ms_cg),
               pcg_iterations=k_pcg, pcg_converged=bool(rel_pcg < args.rtol),
               pcg_final_rel_residual=rel_pcg, pcg_ms_to_solution=min(ms_pcg),
               iterations_ratio_cg_vs_pcg=k_cg / max(k_pcg, 1),
               time_ratio_cg_vs_pcg=min(ms_cg) / min(ms_pcg))
    print(json.dumps(rec), flush=True)
    ws_cg.close(), ws_pcg.close()
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
    ap.add_argument("--scaled-rows", type=int, default=1_000_000,
                    help="rows of the scaled FEM-like matrix (built on the host)")
    ap.add_argument("--iters", type=int, default=20, help="iterations per solve")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--kmax", type=int, default=20000,
                    help="iteration limit of the scaled case")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcgbench.json"))
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:  # a child: one case in this process
        if args.case == "fem_like_scaled":
            run_scaled(args)
        else:
            run_fixed(args.case, args)
        return 0
    cases = [c for c in CASES if not args.only or c in args.only.split(",")]
    recs = []
    p = None
    for case in cases:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", case, "--n", str(args.n),
               "--rows", str(args.rows), "--scaled-rows", str(args.scaled_rows),
               "--iters", str(args.iters), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup), "--rtol", str(args.rtol),
               "--kmax", str(args.kmax)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"pcgbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
