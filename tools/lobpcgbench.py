"""lobpcg benchmark on one GPU, one preconditioner per process.

    python tools/lobpcgbench.py            # all cases -> profiles/lobpcgbench.json

Matrix: the 7-point Poisson matrix on n^3 points (general storage), nev
vectors (`--nev`, default 8), the initial block from a seeded generator.

One JSON record per case (none, jacobi, sgs, amg):

  solve    iterations, status and wall ms to `--rtol` (kmax `--kmax`), the true
           residual norms of the epilogue, the restarts
  step     wall ms per iteration of a solve of `--iters` iterations at a
           tolerance no column meets, with mult_block's share from one more
           solve with time_spmv
  kernels  (case none only) the Gram, Rayleigh-Ritz, update and residual kernels
           and the preconditioner applications, each launched `--launches` times
           on its own through the C ABI: ms per launch, and for the Gram (6
           blocks read) and update (6 read, 4 written) kernels the achieved
           bytes per second

    python tools/lobpcgbench.py --mass     # -> profiles/lobpcgbench_gen.json

`--mass`: the same cases once more in the same process with a mass-like B on A's
pattern (1.1 on the diagonal, 0.1 beside it), the pencil A x = lambda B x.  Each
record then also has

  solve_gen, step_gen   as solve and step, with B; step_gen adds mult_block(B)
           (B.mult_block launched `--launches` times on its own) beside
           mult_block(A) from time_spmv
  kernels  (case none only) the nine-block Gram kernel (9 blocks read) and the
           three-triple update (9 read, 6 written) with their bytes per second,
           beside the six-block kernels' figures from the same process, and
           split_gen_ms: one iteration with B as mult_block(A), mult_block(B),
           Gram (+ reducer), Rayleigh-Ritz, update and residual (+ norms)

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

CASES = ("none", "jacobi", "sgs", "amg")


def run_case(case, args):
    from spmv_amd import _lib, host, poisson
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    rp, ci, va = poisson.poisson3d_csr(args.n)
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    va = np.array(va, np.float64)
    rows, nev = len(rp) - 1, args.nev
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, rows, rows, [], [],
                                  False, host.P2P_BLOCKING)
    X0 = np.random.default_rng(1).uniform(-1.0, 1.0, (rows, nev))
    d_x = exec_.alloc(rows * nev)
    d_dinv = exec_.alloc(rows)
    exec_.copy_from_host(d_dinv, np.full(rows, 1.0 / 6.0))
    pre, M = {}, None
    if case == "jacobi":
        pre = dict(dinv=d_dinv)
    elif case == "sgs":
        M = host.SgsPreconditioner(exec_, A)
        pre = dict(sgs=M)
    elif case == "amg":
        M = host.AmgPreconditioner(exec_, A)
        pre = dict(amg=M)
    ws = host.LobpcgWorkspace(exec_)
    ws.reserve_timing(max(args.iters, args.kmax))
    rec = dict(case=case, n=args.n, rows=rows, nev=nev, nnz=A.non_zeros())

    B = None
    if args.mass:
        vb = np.where(ci == np.repeat(np.arange(rows), np.diff(rp)), 1.1, 0.1)
        B = host.Matrix.create_matrix(comm, exec_, rp, ci, vb, rows, rows, [], [],
                                      False, host.P2P_BLOCKING)

    def solve(kmax, rtol, **kw):
        exec_.copy_from_host(d_x, X0)
        exec_.synchronize()
        st = {}
        t0 = time.perf_counter()
        k, theta, hist, status = host.lobpcg(comm, exec_, A, d_x, nev, kmax, rtol,
                                             workspace=ws, stats=st, **pre, **kw)
        return (time.perf_counter() - t0) * 1e3, k, theta, status, st

    def per_launch(fn):
        fn()
        exec_.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            fn()
        exec_.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.launches

    for tag, kw in (("", {}),) + ((("_gen", dict(B=B)),) if B is not None else ()):
        solve(2, 1e-30, **kw)  # warm-up: plans, workspace
        ms, k, theta, status, st = solve(args.kmax, args.rtol, **kw)
        rec["solve" + tag] = dict(rtol=args.rtol, kmax=args.kmax, iterations=k,
                                  status=status, ms=ms, theta=theta.tolist(),
                                  true_resnorm=st["true_resnorm"].tolist(),
                                  restarts=st["restarts"])
        best = min(solve(args.iters, 1e-30, **kw)[0]
                   for _ in range(args.repeats))
        _, k2, _, _, st = solve(args.iters, 1e-30, time_spmv=True, **kw)
        rec["step" + tag] = dict(iters=k2, ms_per_iteration=best / max(k2, 1),
                                 mult_block_ms=st["spmv_ms_total"]
                                 / max(st["spmv_launches"], 1))
    if B is not None:
        d_in, d_out = exec_.alloc(rows * nev), exec_.alloc(rows * nev)
        exec_.copy_from_host(d_in, X0)
        rec["step_gen"]["mult_block_b_ms"] = per_launch(
            lambda: B.mult_block(d_in, d_out, nev))
        rec["step_gen"]["mult_block_a_alone_ms"] = per_launch(
            lambda: A.mult_block(d_in, d_out, nev))
        exec_.free(d_in)
        exec_.free(d_out)

    if case == "none":
        ctx = exec_.context
        h = C.c_void_p()
        _lib.call("spmv_hip_lobpcg_ws_create", ctx, 4, nev, C.byref(h))
        blocks = [exec_.alloc(rows * nev) for _ in range(10)]
        rng = np.random.default_rng(2)
        for b in blocks:  # independent blocks: the Rayleigh-Ritz step succeeds
            exec_.copy_from_host(b, rng.uniform(-1.0, 1.0, (rows, nev)))

        X, W, P, AX, AW, AP, R, BX, BW, BP = blocks
        _lib.call("spmv_hip_lobpcg_ws_reset", h, 1e-30, 0.0, 4, 0, None)
        nbytes = rows * nev * 8
        kern = {}
        kern["gram_ms"] = per_launch(lambda: _lib.call(
            "spmv_hip_lobpcg_gram_f64", ctx, h, rows, 3, X, W, P, AX, AW, AP, None))
        kern["gram_bytes_per_s"] = 6 * nbytes / (kern["gram_ms"] * 1e-3)

        kern["gram_reduce_ms"] = per_launch(lambda: _lib.call(
            "spmv_hip_lobpcg_gram_reduce", ctx, h, rows, 3, None))

        def rr():  # (the state is put back so that every launch does the work)
            _lib.call("spmv_hip_lobpcg_ws_set_state", h, (1 << nev) - 1, 1, 0, 0,
                      None)
            _lib.call("spmv_hip_lobpcg_rr", ctx, h, rows, 3, 0, 1, 0, None)
        kern["rr_ms"] = per_launch(rr)
        exec_.synchronize()
        state = np.zeros(8, np.int32)
        _lib.call("spmv_hip_lobpcg_ws_read_async", h,
                  state.ctypes.data_as(C.c_void_p), None, 0, None, None)
        exec_.synchronize()
        kern["rr_status"] = int(state[2])
        kern["update_ms"] = per_launch(lambda: _lib.call(
            "spmv_hip_lobpcg_update_f64", ctx, h, rows, 3, X, W, P, AX, AW, AP,
            None))
        kern["update_bytes_per_s"] = 10 * nbytes / (kern["update_ms"] * 1e-3)
        kern["residual_ms"] = per_launch(lambda: _lib.call(
            "spmv_hip_lobpcg_residual_f64", ctx, h, rows, X, AX, None, R, W, 0,
            None))
        if B is not None:
            kern["norms_ms"] = per_launch(lambda: _lib.call(
                "spmv_hip_lobpcg_norms", ctx, h, 0, 1, None))
            kern["gram_gen_ms"] = per_launch(lambda: _lib.call(
                "spmv_hip_lobpcg_gram_gen_f64", ctx, h, rows, 3, X, W, P, AX, AW,
                AP, BX, BW, BP, None))
            kern["gram_gen_bytes_per_s"] = 9 * nbytes / (kern["gram_gen_ms"] * 1e-3)
            _lib.call("spmv_hip_lobpcg_gram_f64", ctx, h, rows, 3, X, W, P, AX, AW,
                      AP, None)  # (finite coefficients again for the update)
            _lib.call("spmv_hip_lobpcg_gram_reduce", ctx, h, rows, 3, None)
            rr()
            kern["update_gen_ms"] = per_launch(lambda: _lib.call(
                "spmv_hip_lobpcg_update_gen_f64", ctx, h, rows, 3, X, W, P, AX, AW,
                AP, BX, BW, BP, None))
            kern["update_gen_bytes_per_s"] = (15 * nbytes
                                              / (kern["update_gen_ms"] * 1e-3))
            kern["residual_gen_ms"] = per_launch(lambda: _lib.call(
                "spmv_hip_lobpcg_residual_gen_f64", ctx, h, rows, AX, BX, None, R,
                W, 0, None))
            g = rec["step_gen"]
            kern["split_gen_ms"] = dict(
                mult_block_a=g["mult_block_a_alone_ms"],
                mult_block_b=g["mult_block_b_ms"],
                gram=kern["gram_gen_ms"] + kern["gram_reduce_ms"],
                rayleigh_ritz=kern["rr_ms"], update=kern["update_gen_ms"],
                residual=kern["residual_gen_ms"] + kern["norms_ms"])
            kern["split_ms"] = dict(
                mult_block_a=g["mult_block_a_alone_ms"],
                gram=kern["gram_ms"] + kern["gram_reduce_ms"],
                rayleigh_ritz=kern["rr_ms"], update=kern["update_ms"],
                residual=kern["residual_ms"] + kern["norms_ms"])
        sgs = host.SgsPreconditioner(exec_, A)
        kern["sgs_apply_block_ms"] = per_launch(
            lambda: host.sgs_apply_block(exec_, sgs, R, W, nev))
        sgs.close()
        amg = host.AmgPreconditioner(exec_, A)
        kern["amg_apply_block_ms"] = per_launch(
            lambda: host.amg_apply_block(exec_, amg, R, W, nev))
        amg.close()
        rec["kernels"] = kern
        _lib.call("spmv_hip_lobpcg_ws_destroy", h)
        for b in blocks:
            exec_.free(b)

    print(json.dumps(rec), flush=True)
    ws.close()
    if M is not None:
        M.close()
    exec_.free(d_x)
    exec_.free(d_dinv)
    if B is not None:
        B.close()
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="grid edge")
    ap.add_argument("--nev", type=int, default=8)
    ap.add_argument("--iters", type=int, default=40,
                    help="iterations of the fixed-length solves")
    ap.add_argument("--kmax", type=int, default=1000)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--only", default=None, help="comma list of cases")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--mass", action="store_true",
                    help="also the pencil with a mass-like B on A's pattern")
    ap.add_argument("--out", default=None,
                    help="default: profiles/lobpcgbench.json "
                         "(--mass: profiles/lobpcgbench_gen.json)")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lobpcgbench_gen.json"
                                if args.mass else "lobpcgbench.json")
    if args.case:  # a child: one case in this process
        run_case(args.case, args)
        return 0
    cases = [c for c in CASES if not args.only or c in args.only.split(",")]
    recs = []
    p = None
    for case in cases:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", case]
        for key in ("n", "nev", "iters", "kmax", "rtol", "repeats", "launches"):
            cmd += ["--" + key, str(getattr(args, key))]
        if args.mass:
            cmd.append("--mass")
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"lobpcgbench: case {case} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
