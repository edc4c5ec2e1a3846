"""spmv::lsqr (LSQR on Matrix::mult and Matrix::transpmult).

Shapes are lsqr_cases.py's: convdiff11 (c = 0.5, 2), tall (900 x 300), wide
(300 x 900), poisson11 for symmetric storage, skew64 for bicgstab's breakdown;
right-hand sides A.1 and uniform(-1, 1); KMAX = 600, RTOL = LTOL = 1e-10.  The
reference is lsqr_cases.lsqr_ref on oracle.csr_spmv of the matrix and of its
stable transpose, run with two summation orders of the dot product
(oracle.ddot, lsqr_cases.dot_chunks64); the bars, every figure printed before
anything is asserted:
  |k - k_ref| <= 1, equal status
  both histories over min(k, k_ref, 50) entries within max(1e-9, 10 * dev_ref)
      of their first entry; a case whose dev_ref exceeds 1e-5 FAILS
  ||x - x_ref|| <= max(1e-8, 10 * xdev_ref) ||x_ref||
  status 0: ||b - A x|| / ||b|| <= 10 * max(rtol, the same of x_ref)
  status 1: ||A^T (b - A x) - damp^2 x|| <= 10 * the same of x_ref
both by oracle.csr_spmv.

X sits between guard words and is filled with a sentinel before every solve."""
import numpy as np
import pytest

import lsqr_cases as lc
import oracle
from spmv_amd import _lib, host
from test_lsqr_host import exit_case, products

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24
SENTINEL = 777.0
KMAX, RTOL, LTOL = lc.KMAX, lc.RTOL, lc.LTOL
GUARD = 2


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


class _Ref:
    def __init__(self, spmv, spmvt, b, kmax=KMAX, rtol=RTOL, ltol=LTOL, damp=0.0,
                 dots=None):
        d1, d2 = dots or (oracle.ddot, lc.dot_chunks64)
        self.x, self.k, self.hist_r, self.hist_ar, self.status = lc.lsqr_ref(
            spmv, spmvt, d1, b, kmax, rtol, ltol, damp)
        self.second = lc.lsqr_ref(spmv, spmvt, d2, b, kmax, rtol, ltol, damp)
        self.b, self.damp, self.spmv, self.spmvt = b, damp, spmv, spmvt
        self.true_res = self.res(self.x)
        self.true_ares = self.ares(self.x)

    def res(self, x):
        return float(np.linalg.norm(self.b - self.spmv(x))
                     / np.linalg.norm(self.b))

    def ares(self, x):
        return float(np.linalg.norm(self.spmvt(self.b - self.spmv(x))
                                    - self.damp * self.damp * x))

    def xdev(self):
        return float(np.linalg.norm(self.second[0] - self.x)
                     / np.linalg.norm(self.x))

    def dev(self, n):
        n = min(n, self.second[1])
        if n == 0:
            return 0.0
        return max(float(np.abs(self.second[i][:n] - h[:n]).max() / h[0])
                   for i, h in ((2, self.hist_r), (3, self.hist_ar)))


def _vs_ref(k, hist_r, hist_ar, x, status, ref, what, kmax=KMAX, rtol=RTOL,
            history_only=False):
    """every figure is printed before anything is asserted"""
    n = min(k, ref.k, 50)
    dev_ref, xdev_ref = ref.dev(n), ref.xdev()
    dev = max(float(np.abs(h[:n] - r[:n]).max() / r[0]) for h, r in
              ((hist_r, ref.hist_r), (hist_ar, ref.hist_ar))) if n else 0.0
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res, ares = ref.res(x), ref.ares(x)
    print(what, "k", k, "k_ref", ref.k, "k_ref (second order)", ref.second[1],
          "status", status, "status_ref", ref.status, "history deviation", dev,
          "dev_ref", dev_ref, "x error", err, "xdev_ref", xdev_ref,
          "true residual", res, "of the reference", ref.true_res,
          "true A^T residual", ares, "of the reference", ref.true_ares)
    assert status == ref.status, (what, status, ref.status)
    assert len(hist_r) == len(hist_ar) == k + 1, what
    assert dev_ref <= 1e-5, (what, "the reference disagrees with itself", dev_ref)
    assert dev <= max(1e-9, 10 * dev_ref), (what, dev, dev_ref)
    if history_only:
        return
    assert abs(k - ref.k) <= 1, (what, k, ref.k)
    assert err <= max(1e-8, 10 * xdev_ref), (what, err, xdev_ref)
    if status == 0:
        if 0 < k < kmax:
            assert hist_r[k] / hist_r[0] < rtol, what
        assert res <= 10 * max(rtol, ref.true_res), (what, res, ref.true_res)
    if status == 1:
        assert ares <= 10 * ref.true_ares, (what, ares, ref.true_ares)


class _Problem:
    """One matrix (general storage; poisson11 also symmetric), right-hand sides
    and references (computed once)."""

    def __init__(self, exec_, comm, name):
        self.name, self.exec_ = name, exec_
        self.csr, self.ncols = lc.csr_by_name(name)
        self.nrows = len(self.csr[0]) - 1
        self.spmv, self.spmvt = products(name)
        self.rhs = {kind: lc.rhs(name, kind, self.spmv)
                    for kind in ("ones", "rand")}
        self.rhs["zero"] = np.zeros(self.nrows)
        self.A = {False: host.Matrix.create_matrix(
            comm, exec_, *self.csr, self.nrows, self.ncols, [], [], False,
            host.P2P_NONBLOCKING)}
        if name == "poisson11":
            self.A[True] = host.Matrix.create_matrix(
                comm, exec_, *self.csr, self.nrows, self.ncols, [], [], True,
                host.P2P_NONBLOCKING)
        self.d_b = exec_.alloc(self.nrows + 2)
        self.d_x = exec_.alloc(self.ncols + 2 * GUARD + 2)
        self.ws = host.LsqrWorkspace(exec_)
        self._ref = {}

    def ref(self, rhs, **kw):
        key = (rhs, tuple(sorted(kw.items())))
        if key not in self._ref:
            self._ref[key] = _Ref(self.spmv, self.spmvt, self.rhs[rhs], **kw)
        return self._ref[key]

    def solve(self, comm, rhs, kmax=KMAX, rtol=RTOL, ltol=LTOL, damp=0.0,
              ws=None, x_off=GUARD, b=None, b_off=0, symmetric=False,
              finite=True, **kw):
        """-> (k, hist_r, x, status, hist_ar)"""
        e, N = self.exec_, self.ncols
        bb = self.rhs[rhs] if b is None else b
        e.copy_from_host(self.d_b + 8 * b_off, bb)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD + 2, SENTINEL))
        k, hist_r, hist_ar, status = host.lsqr(
            comm, e, self.A[symmetric], self.d_b + 8 * b_off,
            self.d_x + 8 * x_off, kmax, rtol, ltol, damp, ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD + 2)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[x_off + N:] == SENTINEL), (self.name, "guard behind")
        if finite:
            assert np.all(np.isfinite(x)) and not np.any(x == SENTINEL), self.name
            assert np.all(np.isfinite(hist_r)), self.name
            assert np.all(np.isfinite(hist_ar)), self.name
        return k, hist_r.copy(), x, status, hist_ar.copy()

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_b, self.d_x):
            self.exec_.free(p)


SHAPES = ("convdiff11_0.5", "convdiff11_2", "tall", "wide", "poisson11", "skew64")


@pytest.fixture(scope="module")
def problems(exec_, comm):
    ps = {name: _Problem(exec_, comm, name) for name in SHAPES}
    yield ps
    for p in ps.values():
        p.close()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, exec_):
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]), what
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), what
    assert a[3] == b[3], (what, a[3], b[3])


# ---- whole solves against the reference ---------------------------------------
@pytest.mark.parametrize("case", sorted(lc.TABLE), ids=str)
def test_against_the_reference(comm, problems, nt, case):
    shape, rhs, damp = case
    P = problems[shape]
    ref = P.ref(rhs, damp=damp)
    k, hist_r, x, status, hist_ar = P.solve(comm, rhs, damp=damp)
    assert k < KMAX and status == lc.TABLE[case][1]
    _vs_ref(k, hist_r, hist_ar, x, status, ref, case)


def test_symmetric_storage_equals_general(comm, problems, nt):
    """poisson11 with b = uniform(-1, 1).  (b = A.1 is left out: on this
    symmetric grid the restatement's own two summation orders disagree by 5e-2
    in the history, so the case would fail the dev_ref bar whatever the device
    does.)"""
    P = problems["poisson11"]
    ref = P.ref("rand")
    g = P.solve(comm, "rand")
    s = P.solve(comm, "rand", symmetric=True)
    _vs_ref(g[0], g[1], g[4], g[2], g[3], ref, "general")
    _vs_ref(s[0], s[1], s[4], s[2], s[3], ref, "symmetric")
    n = min(g[0], s[0], 50)
    dev = max(np.abs(s[i][:n] - g[i][:n]).max() / g[i][0] for i in (1, 4))
    print("symmetric against general", dev, "dev_ref", ref.dev(n), "k", s[0], g[0])
    assert dev <= max(1e-9, 10 * ref.dev(n))
    assert abs(s[0] - g[0]) <= 1 and s[3] == g[3] == 0


def test_where_bicgstab_breaks_down(comm, problems):
    P = problems["skew64"]
    e, A, N = P.exec_, P.A[False], P.nrows
    b = P.rhs["ones"]  # A.1: b.(A b) is exactly 0, block by block
    d_x = e.alloc(N)
    try:
        e.copy_from_host(P.d_b, b)
        out = host.bicgstab(comm, e, A, P.d_b, d_x, None, 50, RTOL)
        print("bicgstab", out[0], out[-1])
        assert out[-1] in (1, 2), "bicgstab was expected to break down"
    finally:
        e.free(d_x)
    k, hist_r, x, status, hist_ar = P.solve(comm, "ones")
    res = np.linalg.norm(b - P.spmv(x)) / np.linalg.norm(b)
    print("lsqr k", k, "status", status, "residual", res)
    assert status == 0 and 0 < k < KMAX and res < RTOL
    assert hist_r[k] / hist_r[0] < RTOL
    _vs_ref(k, hist_r, hist_ar, x, status, P.ref("ones"), "skew64")


# ---- the exits on the device ----------------------------------------------------
def _dense_csr(A):
    import gmres_cases as gc
    m, n = A.shape
    r, c = np.nonzero(np.ones((m, n)))
    return gc.to_csr(m, [r], [c], [A[r, c]])


@pytest.mark.parametrize("name", ["identity", "orthogonal", "diag123", "ltol",
                                  "ltol_damped", "kmax", "rtol"])
def test_the_exits(exec_, comm, nt, name):
    A, b, damp, kmax, rtol, ltol, ref, _, status_want = exit_case(name)
    x_ref, k_ref, hr_ref, har_ref, status_ref = ref
    m, n = A.shape
    M = host.Matrix.create_matrix(comm, exec_, *_dense_csr(A), m, n, [], [],
                                  False, host.P2P_NONBLOCKING)
    d_b, d_x = exec_.alloc(m), exec_.alloc(n)
    try:
        exec_.copy_from_host(d_b, b)
        exec_.copy_from_host(d_x, np.full(n, SENTINEL))
        k, hist_r, hist_ar, status = host.lsqr(comm, exec_, M, d_b, d_x, kmax,
                                               rtol, ltol, damp)
        x = exec_.copy_to_host(d_x, n)
        print(name, "k", k, "status", status, "x", x, "hist_r", hist_r,
              "hist_ar", hist_ar)
        assert (k, status) == (k_ref, status_ref)
        assert status_want is None or status == status_want
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(hist_r))
        assert np.allclose(x, x_ref, rtol=0, atol=1e-13)
        assert np.allclose(hist_r, hr_ref, rtol=0, atol=1e-13 * hr_ref[0])
    finally:
        M.close()
        exec_.free(d_b), exec_.free(d_x)


def test_a_zero_right_hand_side(comm, problems, nt):
    for name in ("tall", "wide"):
        k, hist_r, x, status, hist_ar = problems[name].solve(comm, "zero")
        assert (k, status) == (0, 0)
        assert list(hist_r) == [0.0] and list(hist_ar) == [0.0]
        assert np.all(x == 0.0)


# ---- frame ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,rhs,damp", [("convdiff11_2", "ones", 0.0),
                                            ("tall", "rand", 0.5)])
def test_x_is_frozen_after_convergence(comm, problems, nt, shape, rhs, damp):
    """the host runs up to 16 iterations ahead of the device's `done`: what it
    enqueues after the stop changes nothing"""
    P = problems[shape]
    want = P.solve(comm, rhs, damp=damp, poll_every=1)
    assert 0 < want[0] < KMAX
    _same(want, P.solve(comm, rhs, damp=damp, poll_every=16), "poll 16")
    _same(want, P.solve(comm, rhs, damp=damp), "default poll")


def test_fixed_number_of_steps(comm, problems, nt):
    P = problems["convdiff11_0.5"]
    for kmax in (0, 1, 2, 7):
        k, hist_r, x, status, hist_ar = P.solve(comm, "ones", kmax=kmax, rtol=0.0,
                                                ltol=0.0)
        assert (k, status) == (kmax, 0) and hist_r.shape == (kmax + 1,)
        assert hist_ar.shape == (kmax + 1,)
        assert np.any(x != 0.0) == (kmax > 0)
        ref = P.ref("ones", kmax=kmax, rtol=0.0, ltol=0.0)
        assert ref.k == kmax
        dev = max(np.abs(hist_r - ref.hist_r).max() / hist_r[0],
                  np.abs(hist_ar - ref.hist_ar).max() / hist_ar[0])
        print("kmax", kmax, "history deviation", dev)
        assert dev <= 1e-9


def test_unaligned_vectors_keep_the_bits(comm, problems, nt):
    for name in ("tall", "wide"):
        P = problems[name]
        want = P.solve(comm, "rand", kmax=10)
        _same(want, P.solve(comm, "rand", kmax=10, x_off=GUARD + 1), "unaligned x")
        _same(want, P.solve(comm, "rand", kmax=10, b_off=1), "unaligned b")
        _same(want, P.solve(comm, "rand", kmax=10, x_off=GUARD + 1, b_off=1),
              "both unaligned")


def test_a_workspace_is_reused_and_grows(comm, problems):
    small, large = problems["wide"], problems["convdiff11_2"]
    ws = host.LsqrWorkspace(small.exec_)
    try:
        want_s = small.solve(comm, "rand", kmax=10)
        want_l = large.solve(comm, "rand")
        for _ in range(2):
            _same(want_s, small.solve(comm, "rand", kmax=10, ws=ws), "small")
            _same(want_l, large.solve(comm, "rand", ws=ws), "grown")
    finally:
        ws.close()


def test_time_spmv_counts_two_products_per_iteration(comm, problems):
    P = problems["tall"]
    stats = {}
    want = P.solve(comm, "rand", kmax=5, rtol=0.0, ltol=0.0)
    got = P.solve(comm, "rand", kmax=5, rtol=0.0, ltol=0.0, time_spmv=True,
                  stats=stats)
    _same(want, got, "timed")
    assert got[0] == 5
    assert stats["spmv_launches"] == 10 and stats["spmv_ms_total"] > 0.0


def test_error_strings(comm, problems):
    P = problems["tall"]
    e, A = P.exec_, P.A[False]
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.lsqr(comm, e, A, P.d_b, P.d_x, -1, 1e-8)
    with pytest.raises(host.SpmvHostError, match="ltol"):
        host.lsqr(comm, e, A, P.d_b, P.d_x, 5, 1e-8, ltol=-1.0)
    with pytest.raises(host.SpmvHostError, match="damp"):
        host.lsqr(comm, e, A, P.d_b, P.d_x, 5, 1e-8, damp=float("nan"))
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.lsqr(comm, e, A, P.d_b, P.d_b + 8 * 899, 5, 1e-8)
    # the executor's stream is restored after a refused call
    k, hist_r, x, status, hist_ar = P.solve(comm, "ones")
    assert 0 < k < KMAX and status == 0


def test_nan_runs_to_kmax_and_the_workspace_stays_usable(comm, problems, nt):
    P = problems["tall"]
    want = P.solve(comm, "rand")
    b = P.rhs["rand"].copy()
    b[17] = np.nan
    k, hist_r, x, status, hist_ar = P.solve(comm, "rand", b=b, kmax=12,
                                            finite=False)
    assert (k, status) == (12, 0) and np.all(np.isnan(hist_r))
    _same(want, P.solve(comm, "rand"), "after the NaN")


# ---- several ranks -------------------------------------------------------------------
def test_slab_ranks_threaded_lsqr():
    """Two ranks as threads (tests/thread_world.py), convdiff11 (c = 2) in slabs
    via oracle.localise_rows, general storage, a blocking and an overlapping
    halo model, one workspace per rank: the reducers, the all-reduces of ut.ut
    and vn.vn, `reduced` in update_v / start / step, the ghost tail of vt and the
    reverse halo update of A^T ut.  Against lsqr_ref on oracle.dist_spmv with the
    rank-ordered dot product; every rank returns the same k and status.

    The transposed reference is the GLOBAL stable-transpose product: it does not
    add a ghost column's contribution in reverse_update's order (the owner's own
    share first, then the neighbour's), so this test is held to the tolerance
    bars of _vs_ref -- k, status, both histories, x and the residual -- not to
    bits."""
    from thread_world import ThreadWorld
    world = 2
    name = "convdiff11_2"
    csr, N = lc.csr_by_name(name)
    T = lc.stable_transpose(csr, N)
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)

    def dist(dot):
        def dd(a, b):
            s = 0.0
            for r in range(world):
                s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
            return s
        return dd

    def spmvt(q):
        return oracle.csr_spmv(*T, q)

    plain = lambda q: oracle.csr_spmv(*csr, q)  # noqa: E731
    bs = {kind: lc.rhs(name, kind, plain) for kind in ("ones", "rand")}
    cases = {}
    for cm in models:
        def spmv(q, cm=cm):
            return oracle.dist_spmv(world, *csr, q, False, cm)
        cases[cm] = {
            (kind, kmax, rtol): _Ref(
                spmv, spmvt, bs[kind], kmax=kmax, rtol=rtol,
                ltol=LTOL if rtol else 0.0,
                dots=(dist(oracle.ddot), dist(lc.dot_chunks64)))
            for kind, kmax, rtol in (("ones", KMAX, RTOL), ("rand", KMAX, RTOL),
                                     ("rand", 30, 0.0))}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.LsqrWorkspace(exec_)
        d_b = exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for cm, refs in cases.items():
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            for (kind, kmax, rtol), ref in refs.items():
                exec_.copy_from_host(d_b, bs[kind][r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist_r, hist_ar, status = host.lsqr(
                    comm, exec_, A, d_b, d_x + 8 * GUARD, kmax, rtol,
                    LTOL if rtol else 0.0, 0.0, ws=ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX and (rtol > 0.0 or k == kmax)
                _vs_ref(k, hist_r, hist_ar, xs, status, ref, (world, cm, kind),
                        kmax=kmax, rtol=rtol, history_only=rtol == 0.0)
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
