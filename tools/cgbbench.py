"""cg_block benchmark on one GPU: a fixed number of iterations of cg_block on
nrhs right-hand sides against nrhs solves of cg() with its default options,
per matrix in ONE process.

    python tools/cgbbench.py                 # all cases -> profiles/cg_block.json

Cases (those of tools/mvbench.py): the 7-point Poisson matrix on n^3 points in
CSR order (lattice analysis off, csr_in_place on), the unstructured matrix with
10 % far columns, the FEM-like matrix.  For nrhs = 2, 4, 8 one JSON record:
wall time of `--iters` iterations (rtol = 0) of cg_block on a reused workspace,
and of nrhs x `--iters` iterations of cg() on a reused workspace; minimum and
median of `--repeats` repeats after `--warmup` untimed ones, every solve ended
by its own synchronisation; ratio_vs_nrhs_cgs = (the cg()s' minimum) / (the
block's minimum); the form mult_block took (plan key mv_form: 1 native, 2 per
column) and the plan's forms.

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

CASES = ("poisson_csr", "unstructured", "fem_like")
WIDTHS = (2, 4, 8)


def make_matrix(case, args, comm, exec_, host, _lib):
    if case == "poisson_csr":
        # the caller's CSR arrays as they are: no lattice / diagonal form, no LX
        # or sliced jagged copy (tools/mvbench.py)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 1 << 62)
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"csr_in_place", 1)
        return host.Matrix.create_poisson3d(comm, exec_, args.n, False,
                                            host.P2P_BLOCKING)
    if case == "fem_like":
        return host.Matrix.create_fem_like(comm, exec_, args.rows)
    return host.Matrix.create_unstructured(comm, exec_, args.rows, per_row=7,
                                           far_permille=100)


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
    A = make_matrix(case, args, comm, exec_, host, _lib)
    rows, nnz = A.rows(), A.non_zeros()
    forms = {key: A.plan_get(key) for key in ("lat", "lx", "xw", "sjds", "sdia",
                                              "wdia")}
    ws1, wsb = host.CgWorkspace(exec_), host.CgBlockWorkspace(exec_)
    for nrhs in [w for w in WIDTHS if not args.widths
                 or str(w) in args.widths.split(",")]:
        d_b, d_x = exec_.alloc(rows * nrhs), exec_.alloc(rows * nrhs)
        # any right-hand side does for a fixed number of iterations: the
        # benchmark's Gaussian, laid over the block
        _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, rows * nrhs, 0,
                  rows * nrhs, d_b, None)
        exec_.synchronize()
        state = {}

        def block():
            its, _, _ = host.cg_block(comm, exec_, A, d_b, d_x, nrhs, args.iters,
                                      0.0, wsb)
            state["its"] = its

        def singles():  # nrhs solves, one after the other, on slices of B
            for c in range(nrhs):
                k, _, _, _ = host.cg_ex(comm, exec_, A, d_b + 8 * rows * c,
                                        d_x + 8 * rows * c, args.iters, 0.0, ws1)
                state["k"] = k

        ms_b = timed(block, args.repeats, args.warmup)
        form = A.plan_get("mv_form")
        ms_s = timed(singles, args.repeats, args.warmup)
        assert np.all(state["its"] == args.iters) and state["k"] == args.iters
        rec = dict(case=case, rows=rows, nnz=nnz, nrhs=nrhs, iters=args.iters,
                   repeats=args.repeats, mv_form=form,
                   cg_block_ms_min=min(ms_b), cg_block_ms_med=float(np.median(ms_b)),
                   nrhs_cgs_ms_min=min(ms_s), nrhs_cgs_ms_med=float(np.median(ms_s)),
                   cg_block_us_per_iter_per_rhs=min(ms_b) * 1e3 / args.iters / nrhs,
                   cg_us_per_iter=min(ms_s) * 1e3 / args.iters / nrhs,
                   ratio_vs_nrhs_cgs=min(ms_s) / min(ms_b), plan_forms=forms)
        print(json.dumps(rec), flush=True)
        exec_.free(d_b), exec_.free(d_x)
    ws1.close(), wsb.close()
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like / unstructured matrices")
    ap.add_argument("--iters", type=int, default=20, help="iterations per solve")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--widths", default=None, help="comma list of nrhs")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_block.json"))
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
        if args.widths:
            cmd += ["--widths", args.widths]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"cgbbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
