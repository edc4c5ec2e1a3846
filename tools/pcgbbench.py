"""pcg_block benchmark on one GPU: the block sweeps and the block solver against
the single-vector calls on the same objects, per matrix in ONE process.

    python tools/pcgbbench.py                # all cases -> profiles/pcgbbench.json
    python tools/pcgbbench.py --n 48 --rows 100000   # a trial

Cases (those of tools/cgbbench.py): the 7-point Poisson matrix on n^3 points in
CSR order, the unstructured matrix with 10 % far columns, the FEM-like matrix.
For nrhs = 2, 4, 8 one JSON record:
  sweeps   one sgs_apply_block against nrhs calls of sgs_apply on the same
           SgsPreconditioner (wall ms of `--applies` applications ended by one
           synchronisation, minimum and median of `--repeats` repeats);
  solves   pcg_block with the SGS object, and with an Ilu0Preconditioner,
           against nrhs solves of pcg_sgs with the same object and against
           cg_block, all to rtol = 1e-10 on right-hand sides B = A X* with a
           seeded X*: iterations (the largest column's), ms per iteration and
           time to 1e-10, minimum of `--repeats` repeats.
The comparison is always against the single-vector calls in the same process.
A matrix for which no SgsPreconditioner can be built (the unstructured one: its
diagonal is not positive) gets a record with `not_applicable` and the reason.

The driver starts one child process per case under `timeout` and stops at the
first child that fails, so trouble in one case ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cgbbench import CASES, WIDTHS, make_matrix, timed  # noqa: E402

RTOL = 1e-10


def run_case(case, args):
    from spmv_amd import _lib, host
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    A = make_matrix(case, args, comm, exec_, host, _lib)
    rows, nnz = A.rows(), A.non_zeros()
    try:
        sgs = host.SgsPreconditioner(exec_, A, values=args.values)
    except host.SpmvHostError as err:
        # the unstructured matrix has no positive diagonal: no SGS / ILU(0)
        # object exists for it and CG does not apply; recorded as it is
        print(json.dumps(dict(case=case, rows=rows, nnz=nnz,
                              not_applicable=str(err))), flush=True)
        A.close()
        comm.close()
        exec_.close()
        return
    ilu = host.Ilu0Preconditioner(exec_, A, values=args.values)
    ws1, wsb = host.SgsWorkspace(exec_), host.PcgBlockWorkspace(exec_)
    wsc = host.CgBlockWorkspace(exec_)
    for nrhs in [w for w in WIDTHS if not args.widths
                 or str(w) in args.widths.split(",")]:
        n = rows * nrhs
        d_b, d_x, d_s = exec_.alloc(n), exec_.alloc(n), exec_.alloc(n)
        # B = A X*, X* Gaussian, as a block (for the sweeps: any R does) and
        # column-major in d_s for the single-vector calls
        _lib.call("spmv_hip_fill_gaussian_f64", exec_.context, n, 0, n, d_x, None)
        A.mult_block(d_x, d_b, nrhs)  # (one rank: no ghosts to update)
        exec_.synchronize()
        B = exec_.copy_to_host(d_b, n).reshape(rows, nrhs)
        exec_.copy_from_host(d_s, np.ascontiguousarray(B.T))
        rec = dict(case=case, values=args.values, rows=rows, nnz=nnz, nrhs=nrhs, repeats=args.repeats,
                   colors=sgs.num_colors(), applies=args.applies)

        def sweeps_block():
            for _ in range(args.applies):
                host.sgs_apply_block(exec_, sgs, d_b, d_x, nrhs)
            exec_.synchronize()

        def sweeps_single():
            for _ in range(args.applies):
                for c in range(nrhs):
                    host.sgs_apply(exec_, sgs, d_s + 8 * rows * c,
                                   d_x + 8 * rows * c)
            exec_.synchronize()

        for name, fn in (("apply_block", sweeps_block),
                         ("nrhs_applies", sweeps_single)):
            ms = timed(fn, args.repeats, args.warmup)
            rec[name + "_ms_min"] = min(ms) / args.applies
            rec[name + "_ms_med"] = float(np.median(ms)) / args.applies
        rec["apply_ratio_vs_nrhs_applies"] = (rec["nrhs_applies_ms_min"]
                                              / rec["apply_block_ms_min"])

        state = {}

        def solve_block(M):
            def fn():
                its, _, _ = host.pcg_block(comm, exec_, A, d_b, d_x, nrhs,
                                           args.kmax, RTOL, sgs=M, workspace=wsb)
                state["k"] = int(its.max())
            return fn

        def solve_singles(M):
            def fn():
                ks = []
                for c in range(nrhs):
                    k, _ = host.pcg_sgs(comm, exec_, A, M, d_s + 8 * rows * c,
                                        d_x + 8 * rows * c, args.kmax, RTOL, ws1)
                    ks.append(k)
                state["k"] = max(ks)
            return fn

        def solve_cg_block():
            its, _, _ = host.cg_block(comm, exec_, A, d_b, d_x, nrhs, args.kmax,
                                      RTOL, wsc)
            state["k"] = int(its.max())

        for name, fn in (("pcg_block_sgs", solve_block(sgs)),
                         ("nrhs_pcg_sgs", solve_singles(sgs)),
                         ("pcg_block_ilu0", solve_block(ilu)),
                         ("nrhs_pcg_ilu0", solve_singles(ilu)),
                         ("cg_block", solve_cg_block)):
            ms = timed(fn, args.repeats, args.warmup)
            k = state["k"]
            rec[name] = dict(iterations=k, converged=k < args.kmax,
                             ms_to_rtol_min=min(ms),
                             ms_to_rtol_med=float(np.median(ms)),
                             ms_per_iteration=min(ms) / max(k, 1))
        print(json.dumps(rec), flush=True)
        for p in (d_b, d_x, d_s):
            exec_.free(p)
    for w in (ws1, wsb, wsc):
        w.close()
    sgs.close(), ilu.close()
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="Poisson grid edge")
    ap.add_argument("--rows", type=int, default=10_000_000,
                    help="rows of the FEM-like / unstructured matrices")
    ap.add_argument("--kmax", type=int, default=2000)
    ap.add_argument("--applies", type=int, default=10,
                    help="applications of M per timed repeat")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--values", choices=("fp64", "fp32"), default="fp64",
                    help="width of the sweep plans' values")
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--widths", default=None, help="comma list of nrhs")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "pcgbbench.json"))
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
               os.path.abspath(__file__), "--case", case, "--values", args.values,
               "--n", str(args.n),
               "--rows", str(args.rows), "--kmax", str(args.kmax), "--applies",
               str(args.applies), "--repeats", str(args.repeats), "--warmup",
               str(args.warmup)]
        if args.widths:
            cmd += ["--widths", args.widths]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"pcgbbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
