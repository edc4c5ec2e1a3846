"""cg_shifted benchmark on one GPU, per shift count in ONE process.

    python tools/cgsbench.py              # ns = 1, 2, 4, 8 -> profiles/cgsbench.json

Matrix: the 7-point Poisson matrix on n^3 points (general storage), b = A.1.
Shifts: the first ns of `--shifts` (default 0, 0.01, 0.1, 0.5, 1, 3, 10, 100).

One JSON record per ns:

  step      wall ms per iteration of cg_shifted at rtol = 0 over `--iters`
            iterations on a reused workspace (every shift active throughout),
            the product's share from one more solve with CgOptions::time_spmv,
            and the bytes per second of update_xp: what is left of an
            iteration beside the product and update_r's three passes, against
            the 4 ns + 3 passes of 8 rows bytes update_xp makes (an upper
            bound of its time, hence a lower bound of its rate)
  solve     cg_shifted to rtol `--rtol`: the count of every shift, total ms,
            and `active`: how many shifts were active in iteration j (from the
            counts: shift s is active in iterations 1..iterations[s])
  cg        (a) ns calls of cg() on explicitly shifted matrices A + sigma_s I
            (one Matrix per shift, built outside the timed region): iterations
            and ms of each, and their sum
  cg_block  (b) cg_block on ns copies of b with the UNSHIFTED matrix, as a
            stand-in for the cost of streaming the matrix for every column: a
            block solver of the shifted family would need ns matrices; ms per
            iteration alone

The driver starts one child process per ns under `timeout` and stops at the
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

WIDTHS = (1, 2, 4, 8)


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


def run_case(ns, args):
    from spmv_amd import _lib, host, poisson
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    rp, ci, va = poisson.poisson3d_csr(args.n)
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    va = np.array(va, np.float64)
    rows = len(rp) - 1
    row = np.repeat(np.arange(rows), np.diff(rp))
    shifts = [float(s) for s in args.shifts.split(",")][:ns]

    def matrix(sigma):
        v = va.copy()
        v[ci == row] += sigma
        return host.Matrix.create_matrix(comm, exec_, rp, ci, v, rows, rows, [],
                                         [], False, host.P2P_BLOCKING)

    A = matrix(0.0)
    rec = dict(ns=ns, n=args.n, rows=rows, nnz=A.non_zeros(), shifts=shifts,
               repeats=args.repeats, warmup=args.warmup)
    ldx = (rows + 1) // 2 * 2
    d_b, d_one = exec_.alloc(rows), exec_.alloc(rows)
    d_x = exec_.alloc(ns * ldx)
    _lib.call("spmv_hip_fill_const_f64", exec_.context, rows, 1.0, d_one, None)
    A.col_map().update(d_one)
    A.mult(d_one, d_b)  # b = A.1
    exec_.synchronize()
    ws = host.CgShiftedWorkspace(exec_)
    ws.reserve_timing(max(args.iters, args.kmax))

    def shifted(kmax, rtol, **kw):
        return host.cg_shifted(comm, exec_, A, d_b, d_x, ldx, shifts, kmax, rtol,
                               ws=ws, **kw)

    # ---- one iteration with every shift active
    ms = timed(lambda: shifted(args.iters, 0.0), args.repeats, args.warmup)
    st = {}
    k, its, _, status = shifted(args.iters, 0.0, time_spmv=True, stats=st)
    per = min(ms) / max(k, 1)
    spmv = st["spmv_ms_total"] / max(st["spmv_launches"], 1)
    rest = per - spmv
    xp_bytes = (4 * ns + 3) * 8.0 * rows
    all_bytes = (4 * ns + 6) * 8.0 * rows
    rec["step"] = dict(iters=k, status=status, ms_per_iteration=per,
                       ms_per_iteration_med=float(np.median(ms)) / max(k, 1),
                       spmv_ms=spmv, nonspmv_ms_per_iteration=rest,
                       vector_bytes_per_iteration=all_bytes,
                       vector_bytes_per_second=all_bytes / (rest * 1e-3)
                       if rest > 0 else None,
                       update_xp_bytes=xp_bytes,
                       launches_per_iteration=3)
    # ---- to rtol
    got = {}
    ms = timed(lambda: got.update(r=shifted(args.kmax, args.rtol)), args.repeats,
               args.warmup)
    k, its, hist, status = got["r"]
    its = [int(v) for v in its]
    rec["solve"] = dict(rtol=args.rtol, kmax=args.kmax, iterations=its,
                        status=status, ms=spread(ms),
                        ms_per_iteration=min(ms) / max(k, 1),
                        active=[sum(1 for v in its if v >= j)
                                for j in range(1, k + 1)])
    # ---- (a) ns solves of cg() on shifted matrices
    ws_cg = host.CgWorkspace(exec_)
    total, each = 0.0, []
    for sigma in shifts:
        As = matrix(sigma)
        res = {}
        ms = timed(lambda: res.update(r=host.cg_ex(
            comm, exec_, As, d_b, d_x, args.kmax, args.rtol, workspace=ws_cg)),
            args.repeats, args.warmup)
        each.append(dict(sigma=sigma, iterations=res["r"][0], ms=spread(ms)))
        total += min(ms)
        As.close()
    ws_cg.close()
    rec["cg"] = dict(each=each, ms_total=total)
    # ---- (b) cg_block, ns columns streamed through the matrix
    d_bb, d_xb = exec_.alloc(ns * rows), exec_.alloc(ns * rows)
    bb = np.repeat(exec_.copy_to_host(d_b, rows), ns)  # interleaved copies
    exec_.copy_from_host(d_bb, bb)
    ws_b = host.CgBlockWorkspace(exec_)
    ms = timed(lambda: host.cg_block(comm, exec_, A, d_bb, d_xb, ns, args.iters,
                                     0.0, workspace=ws_b),
               args.repeats, args.warmup)
    rec["cg_block"] = dict(iters=args.iters,
                           ms_per_iteration=min(ms) / max(args.iters, 1))
    ws_b.close()
    print(json.dumps(rec), flush=True)
    ws.close()
    for p in (d_b, d_x, d_one, d_bb, d_xb):
        exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="grid edge")
    ap.add_argument("--shifts", default="0,0.01,0.1,0.5,1,3,10,100")
    ap.add_argument("--iters", type=int, default=60,
                    help="iterations of the fixed-length solves")
    ap.add_argument("--kmax", type=int, default=3000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma list of shift counts")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "cgsbench.json"))
    ap.add_argument("--case", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:  # a child: one shift count in this process
        run_case(args.case, args)
        return 0
    widths = [w for w in WIDTHS
              if not args.only or str(w) in args.only.split(",")]
    recs = []
    p = None
    for w in widths:  # each GPU step under its own timeout, chained
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--case", str(w)]
        for key in ("n", "shifts", "iters", "kmax", "rtol", "repeats", "warmup"):
            cmd += ["--" + key, str(getattr(args, key))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        recs += [json.loads(line) for line in p.stdout.splitlines()
                 if line.startswith("{")]
        if p.returncode != 0:
            print(f"cgsbench: ns = {w} ended with status {p.returncode}; "
                  "nothing more is started", file=sys.stderr)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if p is None or p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
