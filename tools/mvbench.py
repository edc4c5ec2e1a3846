"""Multi-vector product benchmark on one GPU: Matrix::mult_block against k
launches of Matrix::mult, per matrix in ONE process.

    python tools/mvbench.py                  # all cases -> profiles/mvbench.json
    python tools/mvbench.py --baseline-only  # mult alone (runs on older trees)

Cases: the 7-point Poisson matrix on n^3 points in CSR order (lattice analysis
off, csr_in_place on: mult runs the XW / gather kernels on the caller's arrays),
the FEM-like matrix and the unstructured matrix with 10 % far columns.
Each case: k = 1 (the single-vector product through mult_block), 2, 4, 8 natively and
k = 4 forced to the per-column fallback.  One JSON record per (case, k, mode):
ms per launch (HIP events around every launch; minimum and median of
`--launches` launches after warm-up), the byte model -- the matrix once, 12 B
per entry + 4 B per row, plus 8 k bytes of x per column and of y per row -- as a
fraction of 8 TB/s, and ratio_vs_k_mults = k * (mult's minimum in the same
process) / (the block's minimum).

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("poisson_csr", "fem_like", "unstructured")
PEAK = 8e12  # bytes per second


def make_matrix(case, args, comm, exec_, host, _lib):
    if case == "poisson_csr":
        # the caller's CSR arrays as they are: no lattice / diagonal form, no LX
        # or sliced jagged copy -- mult runs the CSR-order XW / gather kernels
        # (the records carry plan_forms)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 1 << 62)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"csr_in_place", 1)
        return host.Matrix.create_poisson3d(comm, exec_, args.n, False,
                                            host.P2P_BLOCKING)
    if case == "fem_like":
        return host.Matrix.create_fem_like(comm, exec_, args.rows)
    return host.Matrix.create_unstructured(comm, exec_, args.rows, per_row=7,
                                           far_permille=100)


def time_launches(exec_, _lib, fn, launches, warmup):
    """ms of every launch (its own pair of events), after `warmup` launches"""
    ctx = exec_.context
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.call("spmv_hip_event_create", ctx, 1, C.byref(e0))
    _lib.call("spmv_hip_event_create", ctx, 1, C.byref(e1))
    for _ in range(warmup):
        fn()
    exec_.synchronize()
    ms = []
    for _ in range(launches):
        _lib.call("spmv_hip_event_record", ctx, e0, None)
        fn()
        _lib.call("spmv_hip_event_record", ctx, e1, None)
        _lib.call("spmv_hip_event_synchronize", ctx, e1)
        t = C.c_float()
        _lib.call("spmv_hip_event_elapsed_ms", ctx, e0, e1, C.byref(t))
        ms.append(t.value)
    _lib.call("spmv_hip_event_destroy", ctx, e0)
    _lib.call("spmv_hip_event_destroy", ctx, e1)
    return ms


def run_case(case, args):
    from spmv_amd import _lib, host
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    A = make_matrix(case, args, comm, exec_, host, _lib)
    rows, nnz = A.rows(), A.non_zeros()
    cols = A.col_map().local_size() + A.col_map().num_ghosts()
    kmax = 1 if args.baseline_only else 8
    rng = np.random.default_rng(1)
    d_x, d_y = exec_.alloc(cols * kmax), exec_.alloc(rows * kmax)
    for c0 in range(0, cols * kmax, 1 << 24):  # (piecewise: a small host buffer)
        m = min(1 << 24, cols * kmax - c0)
        exec_.copy_from_host(d_x + 8 * c0, rng.uniform(-1, 1, m))
    forms = {key: A.plan_get(key) for key in ("lat", "lx", "xw", "sjds", "sdia",
                                              "wdia")}
    base = time_launches(exec_, _lib, lambda: A.mult(d_x, d_y), args.launches,
                         args.warmup)
    recs = []

    def record(k, mode, ms, form):
        model = 12.0 * nnz + 4.0 * rows + 8.0 * k * (cols + rows)
        rec = dict(case=case, rows=rows, cols=cols, nnz=nnz, k=k, mode=mode,
                   mv_form=form, launches=len(ms), ms_min=min(ms),
                   ms_med=float(np.median(ms)), model_bytes=model,
                   model_bytes_per_row_per_vector=model / rows / k,
                   fraction_of_8tbs=model / (min(ms) * 1e-3) / PEAK,
                   mult_ms_min=min(base), mult_ms_med=float(np.median(base)),
                   ratio_vs_k_mults=k * min(base) / min(ms), plan_forms=forms)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    record(1, "mult", base, 0)
    if not args.baseline_only:
        for k, native in ((1, 1), (2, 1), (4, 1), (8, 1), (4, 0)):
            A.plan_set("mv_native", native)
            ms = time_launches(exec_, _lib, lambda: A.mult_block(d_x, d_y, k),
                               args.launches, args.warmup)
            mode = "single" if k == 1 else "native" if native else "fallback"
            record(k, mode, ms, A.plan_get("mv_form"))
        A.plan_set("mv_native", 1)
    exec_.synchronize()
    exec_.free(d_x), exec_.free(d_y)
    A.close()
    comm.close()
    exec_.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like / unstructured matrices")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--baseline-only", action="store_true",
                    help="time mult alone: uses nothing mult_block added")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvbench.json"))
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    if args.case:  # a child: one case in this process
        run_case(args.case, args)
        return 0
    cases = [c for c in CASES if not args.only or c in args.only.split(",")]
    recs = []
    for case in cases:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", case, "--n", str(args.n),
               "--rows", str(args.rows), "--launches", str(args.launches),
               "--warmup", str(args.warmup)]
        if args.baseline_only:
            cmd.append("--baseline-only")
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"mvbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    else:
        p = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None else 1


if __name__ == "__main__":
    sys.exit(main())
