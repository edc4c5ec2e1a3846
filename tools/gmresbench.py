"""gmres benchmark on one GPU, per matrix in ONE process.

    python tools/gmresbench.py               # all cases -> profiles/gmresbench.json

Matrices: the 7-point Poisson matrix on n^3 points in CSR order (lattice
analysis off, csr_in_place on; `--skew-ppm` makes it nonsymmetric, 0 keeps the
Poisson matrix) and a nonsymmetric variant of the FEM-like matrix of `--rows`
rows: the numpy twin's matrix with every column j scaled by 1 + 0.3 sin(j) (the
pattern and the positive diagonal stay).

One JSON record per case with three parts.

  kernels   at j + 1 = 8, 16 and 30 basis vectors of the matrix's row count:
            (a) one gmres_multi_dot + gmres_reduce, and one gmres_multi_axpy,
            against (b) j + 1 launches of spmv_hip_dot_partial_f64 +
            spmv_hip_reduce_partials_f64, and of spmv_hip_axpy_f64, on the same
            vectors.  HIP events round `--kreps` back-to-back repeats, minimum
            and median of `--repeats` such measurements after a warm-up, and
            the bytes each moves by the pass model: (a) dot (j + 1 +
            ceil((j + 1) / 8)) vectors, axpy j + 3; (b) dot 2 (j + 1), axpy
            3 (j + 1).  The expectation: (a) approaches (j + 2) / (2 (j + 1))
            of (b)'s bytes for the dots; where the time does not follow, the
            GB/s of both say on which side.
  step      wall ms per inner step of gmres(restart 30, rtol = 0, `--iters`
            steps, no preconditioner and Jacobi) on a reused workspace, and from
            one more solve with CgOptions::time_spmv the SpMV's share.
  solve     iterations and wall ms to rtol 1e-10 (kmax `--kmax`) of
            gmres(30) and bicgstab, both with the Jacobi dinv, b = A.1; one
            bicgstab iteration has two SpMVs, one gmres step one.

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("poisson_csr", "fem_like_nonsym")
BASIS = (8, 16, 30)
GROUP = 8
H = 0  # SPMV_HIP_GMRES_H


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


def make_matrix(case, args, comm, exec_):
    from spmv_amd import _lib, host, poisson
    if case == "poisson_csr":
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 1 << 62)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"csr_in_place", 1)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"poisson_skew_ppm",
                  args.skew_ppm)
        return host.Matrix.create_poisson3d(comm, exec_, args.n, False,
                                            host.P2P_BLOCKING)
    rp, ci, va = poisson.fem_like_csr(args.rows)
    ci = np.asarray(ci, np.int32)
    va = np.asarray(va, np.float64) * (1.0 + 0.3 * np.sin(ci.astype(np.float64)))
    N = len(rp) - 1
    return host.Matrix.create_matrix(comm, exec_, np.asarray(rp, np.int32), ci, va,
                                     N, N, [], [], False, host.P2P_BLOCKING)


def kernel_part(exec_, rows, args):
    """(a) the multi-vector kernels against (b) single-vector launches"""
    from spmv_amd import _lib
    ctx = exec_.context
    call = _lib.call
    stride = rows + (rows & 1)
    nmax = max(BASIS)
    d_V = exec_.alloc(stride * nmax)
    d_w, d_res = exec_.alloc(stride), exec_.alloc(nmax)
    L = C.c_int()
    call("spmv_hip_dot_partials_len", ctx, C.byref(L))
    d_part = exec_.alloc(L.value)
    call("spmv_hip_fill_gaussian_f64", ctx, stride * nmax, 0, stride * nmax, d_V,
         None)
    call("spmv_hip_fill_gaussian_f64", ctx, rows, 0, rows, d_w, None)
    ws = C.c_void_p()
    call("spmv_hip_gmres_ws_create", ctx, 1, C.byref(ws))
    call("spmv_hip_gmres_ws_reset", ws, 0.0, 1, 64, None)  # H = 0: w unchanged
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        call("spmv_hip_event_create", ctx, 1, C.byref(e))

    def measure(body):
        def once():
            call("spmv_hip_event_record", ctx, ev[0], None)
            for _ in range(args.kreps):
                body()
            call("spmv_hip_event_record", ctx, ev[1], None)
            call("spmv_hip_event_synchronize", ctx, ev[1])
            ms = C.c_float()
            call("spmv_hip_event_elapsed_ms", ctx, ev[0], ev[1], C.byref(ms))
            return ms.value / args.kreps
        for _ in range(args.warmup):
            once()
        return spread([once() for _ in range(args.repeats)])

    out = {}
    vec_bytes = 8.0 * rows
    for nv in BASIS:
        def multi_dot():
            call("spmv_hip_gmres_multi_dot_f64", ctx, ws, rows, d_V, stride, nv,
                 d_w, None)
            call("spmv_hip_gmres_reduce", ctx, ws, H, nv, None)

        def single_dots():
            for i in range(nv):
                call("spmv_hip_dot_partial_f64", ctx, rows, d_V + 8 * stride * i,
                     d_w, d_part, None)
                call("spmv_hip_reduce_partials_f64", ctx, d_part, d_res + 8 * i,
                     None)

        def multi_axpy():  # coefficients 0.0: w keeps its values
            call("spmv_hip_gmres_multi_axpy_f64", ctx, ws, 0, rows, d_V, stride,
                 nv, d_w, None)

        def single_axpys():
            for i in range(nv):
                call("spmv_hip_axpy_f64", ctx, rows, 0.0, d_V + 8 * stride * i,
                     d_w, None)

        groups = -(-nv // GROUP)
        rec = {}
        for name, body, passes in (("multi_dot", multi_dot, nv + groups),
                                   ("single_dots", single_dots, 2 * nv),
                                   ("multi_axpy", multi_axpy, nv + 2),
                                   ("single_axpys", single_axpys, 3 * nv)):
            ms = measure(body)
            rec[name] = dict(ms=ms, vector_passes=passes,
                             gbs_at_min=passes * vec_bytes / ms["min"] / 1e6)
        rec["dot_time_ratio"] = (rec["multi_dot"]["ms"]["min"]
                                 / rec["single_dots"]["ms"]["min"])
        rec["dot_bytes_ratio"] = (nv + groups) / (2.0 * nv)
        rec["axpy_time_ratio"] = (rec["multi_axpy"]["ms"]["min"]
                                  / rec["single_axpys"]["ms"]["min"])
        rec["axpy_bytes_ratio"] = (nv + 2) / (3.0 * nv)
        out[str(nv)] = rec
    exec_.synchronize()
    for e in ev:
        call("spmv_hip_event_destroy", ctx, e)
    call("spmv_hip_gmres_ws_destroy", ws)
    for p in (d_V, d_w, d_res, d_part):
        exec_.free(p)
    return out


def run_case(case, args):
    from spmv_amd import _lib, host
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    A = make_matrix(case, args, comm, exec_)
    rows, nnz = A.rows(), A.non_zeros()
    forms = {key: A.plan_get(key) for key in ("lat", "lx", "xw", "sjds", "sdia",
                                              "wdia")}
    rec = dict(case=case, rows=rows, nnz=nnz, plan_forms=forms,
               repeats=args.repeats, warmup=args.warmup, kreps=args.kreps)
    rec["kernels"] = kernel_part(exec_, rows, args)

    d_dinv = exec_.alloc(rows)
    A.diagonal(d_dinv)
    host.jacobi_inverse(exec_, d_dinv, d_dinv, rows)
    d_b, d_x, d_one = exec_.alloc(rows), exec_.alloc(rows), exec_.alloc(rows)
    _lib.call("spmv_hip_fill_const_f64", exec_.context, rows, 1.0, d_one, None)
    A.col_map().update(d_one)
    A.mult(d_one, d_b)  # b = A.1
    exec_.synchronize()
    ws_g, ws_b = host.GmresWorkspace(exec_), host.BicgstabWorkspace(exec_)
    it = args.iters
    ws_g.reserve_timing(max(it, args.kmax)), ws_b.reserve_timing(args.kmax)

    # -- ms per inner step at restart 30, rtol = 0
    rec["step"] = {}
    for name, dinv in (("gmres30", None), ("gmres30_jacobi", d_dinv)):
        state = {}

        def solve(time_spmv=False):
            st = {}
            k, _, status = host.gmres(comm, exec_, A, d_b, d_x, 30, it, 0.0,
                                      dinv_ptr=dinv, ws=ws_g, time_spmv=time_spmv,
                                      stats=st)
            state.update(k=k, status=status, **st)

        ms = timed(solve, args.repeats, args.warmup)
        solve(True)
        assert state["k"] == it and state["status"] == 0, state
        per = min(ms) / it
        rec["step"][name] = dict(
            iters=it, ms_per_step=per, ms_per_step_med=float(np.median(ms)) / it,
            spmv_ms_per_step=state["spmv_ms_total"] / it,
            nonspmv_ms_per_step=per - state["spmv_ms_total"] / it)

    # -- iterations and time to 1e-10 against bicgstab, both with Jacobi
    rec["solve"] = dict(rtol=args.rtol, kmax=args.kmax)
    out = {}

    def run_gmres():
        out["gmres30_jacobi"] = host.gmres(comm, exec_, A, d_b, d_x, 30,
                                           args.kmax, args.rtol, dinv_ptr=d_dinv,
                                           ws=ws_g)

    def run_bicg():
        out["bicgstab_jacobi"] = host.bicgstab(comm, exec_, A, d_b, d_x, d_dinv,
                                               args.kmax, args.rtol, ws_b)

    for name, fn in (("gmres30_jacobi", run_gmres), ("bicgstab_jacobi", run_bicg)):
        ms = timed(fn, args.repeats, args.warmup)
        k, hist, status = out[name]
        rec["solve"][name] = dict(iterations=k, status=status, ms=spread(ms),
                                  rel_residual=float(hist[-1] / hist[0]),
                                  spmvs=k * (2 if name.startswith("bicg") else 1))
    print(json.dumps(rec), flush=True)
    ws_g.close(), ws_b.close()
    for p in (d_dinv, d_b, d_x, d_one):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--skew-ppm", type=int, default=0,
                    help="poisson_skew_ppm of the Poisson generator")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like matrix")
    ap.add_argument("--iters", type=int, default=60,
                    help="inner steps of the fixed-length solves")
    ap.add_argument("--kmax", type=int, default=2000)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kreps", type=int, default=5,
                    help="back-to-back repeats inside one event pair")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "gmresbench.json"))
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
        for key in ("n", "skew_ppm", "rows", "iters", "kmax", "rtol", "repeats",
                    "warmup", "kreps"):
            cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"gmresbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
