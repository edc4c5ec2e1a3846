"""spmv::cg_shifted (multi-shift CG) on the device.

poisson11 (1331 rows) with b = A uniform(-1, 1) and the shift sets of
cgs_cases.py; KMAX = 200, RTOL = 1e-10.  The reference is cgs_cases.cgs_ref on
oracle.csr_spmv, run with two summation orders of the dot product (oracle.ddot,
minres_cases.dot_chunks64).  Matrix::mult_dot produces the partials of p.q
inside the SpMV kernel of whatever plan form the matrix took, in that kernel's
own order, which the restatement does not model: whole solves are therefore held
to the bars of test_gpu_minres.py, per shift, every figure printed before
anything is asserted:
  |k_s - k_ref_s| <= 1, equal status
  the history over min(k_s, k_ref_s, 50) entries within max(1e-9, 10 * dev_ref)
      of its first entry; a case whose dev_ref exceeds 1e-5 FAILS
  ||x_s - x_ref_s|| <= max(1e-8, 10 * xdev_ref) ||x_ref_s||
  ||b - (A + sigma_s I) x_s|| / ||b|| <= 10 * max(rtol, the same of x_ref_s),
      and <= 10 * rtol on symmetric storage and two ranks
by oracle.csr_spmv.  What the device owes bit for bit whatever the order of a
sum -- poll_every, time_spmv, duplicate shifts, the copy path of unaligned
columns, a reused workspace -- is held to bits.

X sits between guard words and is filled with a sentinel before every solve."""
import numpy as np
import pytest

import cgs_cases as cc
import minres_cases as mc
import oracle
from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24
SENTINEL = 777.0
KMAX, RTOL = cc.KMAX, cc.RTOL
GUARD = 2
N = 1331


@pytest.fixture(scope="module")
def exec_():
    e = host.HipExecutor(0)
    yield e
    e.synchronize()
    e.close()


@pytest.fixture(scope="module")
def comm():
    c = host.Comm.self_comm()
    yield c
    c.close()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, exec_):
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


class _Ref:
    def __init__(self, spmv, b, shifts, kmax=KMAX, rtol=RTOL, dots=None):
        d1, d2 = dots or (oracle.ddot, mc.dot_chunks64)
        self.X, self.k, self.its, self.hist, self.status = cc.cgs_ref(
            spmv, d1, b, shifts, kmax, rtol)
        self.second = cc.cgs_ref(spmv, d2, b, shifts, kmax, rtol)
        self.b, self.shifts, self.spmv = b, shifts, spmv

    def res(self, s, x):
        r = self.b - (self.spmv(x) + self.shifts[s] * x)
        return float(np.linalg.norm(r) / np.linalg.norm(self.b))


def _vs_ref(k, its, hist, X, status, ref, what, rtol=RTOL, strict_residual=False):
    """every figure is printed before anything is asserted"""
    rows = []
    for s in range(len(ref.shifts)):
        n = min(its[s], ref.its[s], ref.second[2][s], 50)
        h0 = ref.hist[s, 0]
        dev_ref = float(np.abs(ref.second[3][s, :n + 1]
                               - ref.hist[s, :n + 1]).max() / h0)
        dev = float(np.abs(hist[s, :n + 1] - ref.hist[s, :n + 1]).max() / h0)
        nx = np.linalg.norm(ref.X[s])
        xdev_ref = float(np.linalg.norm(ref.second[0][s] - ref.X[s]) / nx)
        err = float(np.linalg.norm(X[s] - ref.X[s]) / nx)
        res, res_ref = ref.res(s, X[s]), ref.res(s, ref.X[s])
        rows.append((s, n, dev_ref, dev, xdev_ref, err, res, res_ref))
        print(what, "sigma", ref.shifts[s], "k", its[s], "k_ref", ref.its[s],
              "k_ref (second order)", ref.second[2][s], "history deviation", dev,
              "dev_ref", dev_ref, "x error", err, "xdev_ref", xdev_ref,
              "true residual", res, "of the reference", res_ref)
    print(what, "status", status, "status_ref", ref.status, "k", k)
    assert status == ref.status and k == max(its), what
    for s, n, dev_ref, dev, xdev_ref, err, res, res_ref in rows:
        assert abs(its[s] - ref.its[s]) <= 1, (what, s)
        assert dev_ref <= 1e-5, (what, s, "the reference disagrees with itself")
        assert dev <= max(1e-9, 10 * dev_ref), (what, s, dev, dev_ref)
        assert err <= max(1e-8, 10 * xdev_ref), (what, s, err, xdev_ref)
        assert np.all(hist[s, its[s] + 1:] == -1.0), (what, s)
        if rtol > 0.0 and its[s] < hist.shape[1] - 1:
            assert hist[s, its[s]] / hist[s, 0] < rtol, (what, s)
            assert res <= 10 * max(rtol, res_ref), (what, s, res, res_ref)
            if strict_residual:
                assert res <= 10 * rtol, (what, s, res)


class _Problem:
    """poisson11 in both storages, its right-hand side and the references
    (computed once)"""

    def __init__(self, exec_, comm):
        self.exec_ = exec_
        self.csr = cc.poisson11()
        self.spmv = lambda q: oracle.csr_spmv(*self.csr, q)
        self.b = cc.poisson11_rhs(self.spmv)
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.d_b = exec_.alloc(N + 2)
        self.len_x = 8 * (N + 5) + 2 * GUARD + 2
        self.d_x = exec_.alloc(self.len_x)
        self.ws = host.CgShiftedWorkspace(exec_)
        self._ref = {}

    def ref(self, shifts, **kw):
        key = (tuple(shifts), tuple(sorted(kw.items())))
        if key not in self._ref:
            self._ref[key] = _Ref(self.spmv, self.b, tuple(shifts), **kw)
        return self._ref[key]

    def solve(self, comm, shifts, kmax=KMAX, rtol=RTOL, ldx=N + 1, x_off=GUARD,
              symmetric=False, ws=None, b=None, finite=True, A=None, **kw):
        """-> (k, its, hist, X, status)"""
        e, ns = self.exec_, len(shifts)
        e.copy_from_host(self.d_b, self.b if b is None else b)
        e.copy_from_host(self.d_x, np.full(self.len_x, SENTINEL))
        k, its, hist, status = host.cg_shifted(
            comm, e, A or self.A[symmetric], self.d_b, self.d_x + 8 * x_off, ldx,
            shifts, kmax, rtol, ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, self.len_x)
        keep = np.zeros(self.len_x, bool)
        X = np.empty((ns, N))
        for s in range(ns):
            X[s] = buf[x_off + s * ldx:x_off + s * ldx + N]
            keep[x_off + s * ldx:x_off + s * ldx + N] = True
        # the guards, the gaps between the columns, everything behind
        assert np.all(buf[~keep] == SENTINEL), "a word outside the columns moved"
        if finite:
            assert np.all(np.isfinite(X)) and not np.any(X == SENTINEL)
            assert np.all(np.isfinite(hist))
        return k, list(its), hist.copy(), X, status

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_b, self.d_x):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def P(exec_, comm):
    p = _Problem(exec_, comm)
    yield p
    p.close()


def _same(a, b, what):
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4], (what, a[:2], b[:2])
    assert np.array_equal(a[2], b[2], equal_nan=True), what
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), what


# ---- whole solves against the reference ---------------------------------------
@pytest.mark.parametrize("which", ["four", "eight"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
def test_against_the_reference(comm, P, nt, which, symmetric):
    shifts = cc.SHIFT_SETS[which]
    ref = P.ref(shifts)
    assert tuple(ref.its) == cc.COUNTS[which]
    k, its, hist, X, status = P.solve(comm, shifts, symmetric=symmetric)
    _vs_ref(k, its, hist, X, status, ref, (which, symmetric),
            strict_residual=symmetric)


def test_one_shift_of_zero_against_cg(comm, P, nt):
    e = P.exec_
    ref = P.ref(cc.SHIFTS1)
    k, its, hist, X, status = P.solve(comm, cc.SHIFTS1, ldx=N)
    _vs_ref(k, its, hist, X, status, ref, "one")
    d_x = e.alloc(N)
    try:
        e.copy_from_host(P.d_b, P.b)
        k_cg, h_cg = host.cg(comm, e, P.A[False], P.d_b, d_x, KMAX, RTOL)
        x_cg = e.copy_to_host(d_x, N)
    finally:
        e.free(d_x)
    n = min(k, k_cg, 50)
    dev = np.abs(hist[0, :n + 1] - h_cg[:n + 1]).max() / h_cg[0]
    err = np.linalg.norm(X[0] - x_cg) / np.linalg.norm(x_cg)
    dev_ref = np.abs(ref.second[3][0, :n + 1] - ref.hist[0, :n + 1]).max() \
        / ref.hist[0, 0]
    xdev_ref = np.linalg.norm(ref.second[0][0] - ref.X[0]) / np.linalg.norm(ref.X[0])
    print("k", k, "k_cg", k_cg, "history deviation", dev, "dev_ref", dev_ref,
          "x error", err, "xdev_ref", xdev_ref)
    assert abs(k - k_cg) <= 1
    assert dev <= max(1e-9, 10 * dev_ref) and err <= max(1e-8, 10 * xdev_ref)


def test_columns_of_a_wide_solve(comm, P, nt):
    """column s of the eight-shift solve is the one-shift solve with sigma_s;
    duplicate shifts give equal bits, a permutation permutes the columns"""
    wide = P.solve(comm, cc.SHIFTS8)
    for s in (0, 3, 4, 6):
        one = P.solve(comm, (cc.SHIFTS8[s],))
        ref = P.ref((cc.SHIFTS8[s],))
        err = np.linalg.norm(wide[3][s] - one[3][0]) / np.linalg.norm(one[3][0])
        xdev_ref = np.linalg.norm(ref.second[0][0] - ref.X[0]) \
            / np.linalg.norm(ref.X[0])
        print("sigma", cc.SHIFTS8[s], "k", wide[1][s], one[1][0], "x error", err,
              "xdev_ref", xdev_ref)
        assert wide[1][s] == one[1][0]
        assert err <= max(1e-8, 10 * xdev_ref)
    dup = P.solve(comm, (1.0, 0.1, 1.0, 1.0))
    for s in (2, 3):
        assert dup[1][s] == dup[1][0]
        assert np.array_equal(dup[2][s], dup[2][0])
        assert np.array_equal(dup[3][s].view(np.uint64), dup[3][0].view(np.uint64))
    perm = (2, 0, 3, 1)
    four = P.solve(comm, cc.SHIFTS4)
    got = P.solve(comm, [cc.SHIFTS4[i] for i in perm])
    for j, i in enumerate(perm):
        assert got[1][j] == four[1][i] and np.array_equal(got[2][j], four[2][i])
        assert np.array_equal(got[3][j].view(np.uint64),
                              four[3][i].view(np.uint64))


# ---- frame ------------------------------------------------------------------------
def test_x_is_frozen_after_convergence(comm, P, nt):
    """the host runs up to 16 iterations ahead of the device's `done`: what it
    enqueues after the stop changes nothing"""
    want = P.solve(comm, cc.SHIFTS8, poll_every=1)
    assert 0 < want[0] < KMAX
    _same(want, P.solve(comm, cc.SHIFTS8, poll_every=16), "poll 16")
    _same(want, P.solve(comm, cc.SHIFTS8), "default poll")


def test_time_spmv_counts_one_product_per_iteration(comm, P):
    stats = {}
    want = P.solve(comm, cc.SHIFTS4, kmax=9, rtol=0.0)
    got = P.solve(comm, cc.SHIFTS4, kmax=9, rtol=0.0, time_spmv=True, stats=stats)
    _same(want, got, "timed")
    assert got[0] == 9 and got[1] == [9] * 4
    assert stats["spmv_launches"] == 9 and stats["spmv_ms_total"] > 0.0


def test_fixed_number_of_steps(comm, P, nt):
    for kmax in (0, 1, 2, 7):
        k, its, hist, X, status = P.solve(comm, cc.SHIFTS4, kmax=kmax, rtol=0.0)
        ref = P.ref(cc.SHIFTS4, kmax=kmax, rtol=0.0)
        assert (k, its, status) == (kmax, [kmax] * 4, 0) and ref.k == kmax
        assert hist.shape == (4, kmax + 1)
        assert np.any(X != 0.0) == (kmax > 0)
        dev = np.abs(hist - ref.hist).max() / hist[0, 0]
        print("kmax", kmax, "history deviation", dev)
        assert dev <= 1e-9


def test_layouts_keep_the_bits(comm, P, nt):
    """ldx > rows: the gap words are untouched (solve() checks them); an odd
    ldx and an X 8 bytes off take the copy path with the same bits"""
    want = P.solve(comm, cc.SHIFTS4, ldx=N + 1)
    for ldx, x_off in ((N, GUARD), (N + 4, GUARD), (N + 1, GUARD + 1),
                       (N, GUARD + 1), (N + 5, GUARD)):
        _same(want, P.solve(comm, cc.SHIFTS4, ldx=ldx, x_off=x_off), (ldx, x_off))
    one = P.solve(comm, (1.0,), ldx=N)
    _same(one, P.solve(comm, (1.0,), ldx=N, x_off=GUARD + 1), "one, offset")


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
def test_the_exits_on_one_workspace(comm, P, nt, symmetric):
    """b = 0, an indefinite and a negative definite seed, zeta underflowing at
    rtol = 0, rrn == 0, a NaN in b -- on ONE workspace, then a clean solve with
    unchanged bits"""
    e = P.exec_
    ws = host.CgShiftedWorkspace(e)
    want = P.solve(comm, cc.SHIFTS4, symmetric=symmetric)
    d_b = d_x = None
    try:
        for name in cc.EXITS:
            csr, b, shifts, kmax, rtol, k_want, status_want = cc.exit_case(name)
            n = len(b)
            ref = cc.cgs_ref(lambda q: oracle.csr_spmv(*csr, q), oracle.ddot, b,
                             shifts, kmax, rtol)
            A = host.Matrix.create_matrix(comm, e, *csr, n, n, [], [], symmetric,
                                          host.P2P_NONBLOCKING)
            d_b, d_x = e.alloc(n), e.alloc(len(shifts) * n)
            e.copy_from_host(d_b, b)
            e.copy_from_host(d_x, np.full(len(shifts) * n, SENTINEL))
            k, its, hist, status = host.cg_shifted(comm, e, A, d_b, d_x, n, shifts,
                                                   kmax, rtol, ws=ws)
            X = e.copy_to_host(d_x, len(shifts) * n).reshape(len(shifts), n)
            print(name, "k", k, "iterations", list(its), "status", status, "ref",
                  ref[1], ref[2], ref[4])
            assert status == status_want == ref[4]
            assert abs(k - ref[1]) <= 1 and (k_want is None or k == k_want)
            assert not np.any(X == SENTINEL)
            if name != "nan":
                assert np.all(np.isfinite(X)) and np.all(np.isfinite(hist))
                err = np.abs(X - ref[0]).max()
                print(name, "max |x - x_ref|", err)
                assert err <= 1e-9 * max(1.0, np.abs(ref[0]).max())
            else:
                assert np.all(X == 0.0) and np.all(np.isnan(hist[:, 0]))
            if name in ("zero", "negative"):
                assert np.all(X == 0.0) and list(its) == [0] * len(shifts)
            A.close()
            e.free(d_b), e.free(d_x)
            d_b = d_x = None
        _same(want, P.solve(comm, cc.SHIFTS4, symmetric=symmetric, ws=ws),
              "after the exits")
    finally:
        if d_b:
            e.free(d_b), e.free(d_x)
        ws.close()


def test_a_workspace_grows(comm, P):
    ws = host.CgShiftedWorkspace(P.exec_)
    try:
        a = P.solve(comm, (1.0,), kmax=5, rtol=0.0)
        b = P.solve(comm, cc.SHIFTS8)
        for _ in range(2):
            _same(a, P.solve(comm, (1.0,), kmax=5, rtol=0.0, ws=ws), "small")
            _same(b, P.solve(comm, cc.SHIFTS8, ws=ws), "more shifts, more steps")
    finally:
        ws.close()


def test_error_strings(comm, P):
    e, A = P.exec_, P.A[False]
    x = P.d_x + 8 * GUARD
    for kw, name in ((dict(shifts=()), "ns"), (dict(shifts=(0.0,) * 9), "ns"),
                     (dict(kmax=-1), "kmax"), (dict(ldx=N - 1), "ldx"),
                     (dict(shifts=(0.0, -1.0)), "shifts"),
                     (dict(shifts=(float("nan"),)), "shifts"),
                     (dict(b=x + 8 * (N + 7)), "overlaps")):
        a = dict(shifts=(0.0, 1.0), kmax=5, ldx=N + 1, b=P.d_b)
        a.update(kw)
        with pytest.raises(host.SpmvHostError, match=name):
            host.cg_shifted(comm, e, A, a["b"], x, a["ldx"], a["shifts"],
                            a["kmax"], 1e-8)
    # the executor's stream is restored after a refused call
    k, its, hist, X, status = P.solve(comm, cc.SHIFTS4)
    assert 0 < k < KMAX and status == 0


# ---- several ranks -------------------------------------------------------------------
def test_slab_ranks_threaded_cg_shifted():
    """Two ranks as threads (tests/thread_world.py), poisson11 in slabs via
    oracle.localise_rows, both storages' general form with a blocking and an
    overlapping halo model, one workspace per rank: the reducers, the
    all-reduces of p.q and r.r, `reduced` in update_r / start / step and the
    ghost tail of p.  Against cgs_ref on oracle.dist_spmv with the rank-ordered
    dot product; every rank returns the same counts and status."""
    from thread_world import ThreadWorld
    world = 2
    csr = cc.poisson11()
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    plain = lambda q: oracle.csr_spmv(*csr, q)  # noqa: E731
    b = cc.poisson11_rhs(plain)

    def dist(dot):
        def dd(u, v):
            s = 0.0
            for r in range(world):
                s += dot(u[ranges[r]:ranges[r + 1]], v[ranges[r]:ranges[r + 1]])
            return s
        return dd

    refs = {}
    for cm in models:
        def spmv(q, cm=cm):
            return oracle.dist_spmv(world, *csr, q, False, cm)
        refs[cm] = {which: _Ref(spmv, b, cc.SHIFT_SETS[which],
                                dots=(dist(oracle.ddot), dist(mc.dot_chunks64)))
                    for which in ("four", "eight")}
        for ref in refs[cm].values():
            ref.spmv = plain  # the true residual by oracle.csr_spmv
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.CgShiftedWorkspace(exec_)
        ldx = M + 3
        d_b = exec_.alloc(M)
        d_x = exec_.alloc(8 * ldx + 2 * GUARD)
        for cm in models:
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            for which, ref in refs[cm].items():
                shifts = cc.SHIFT_SETS[which]
                ns = len(shifts)
                exec_.copy_from_host(d_b, b[r0:r1])
                exec_.copy_from_host(d_x, np.full(8 * ldx + 2 * GUARD, SENTINEL))
                k, its, hist, status = host.cg_shifted(
                    comm, exec_, A, d_b, d_x + 8 * GUARD, ldx, shifts, KMAX, RTOL,
                    ws=ws)
                buf = exec_.copy_to_host(d_x, 8 * ldx + 2 * GUARD)
                keep = np.zeros(len(buf), bool)
                local = np.empty((ns, M))
                for s in range(ns):
                    local[s] = buf[GUARD + s * ldx:GUARD + s * ldx + M]
                    keep[GUARD + s * ldx:GUARD + s * ldx + M] = True
                assert np.all(buf[~keep] == SENTINEL)
                ks = tw.gather(rank, np.array(list(its) + [k, status]))
                assert np.all(ks.reshape(world, -1) == list(its) + [k, status]), ks
                X = np.stack([tw.gather(rank, local[s]) for s in range(ns)])
                _vs_ref(k, list(its), hist, X, status, ref, (world, cm, which),
                        strict_residual=True)
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
