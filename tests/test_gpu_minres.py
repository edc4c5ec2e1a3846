"""spmv::minres (preconditioned MINRES for symmetric indefinite systems).

Shapes are minres_cases.py's: shift11 (Poisson 11^3 minus I, 17 negative
eigenvalues), poisson11, saddle500 (a saddle-point matrix with a zero block)
and sas (S shift11 S); right-hand sides A.1 and A.uniform(-1, 1); KMAX = 600,
RTOL = 1e-10.  The reference is minres_cases.minres_ref on oracle.csr_spmv, run
with two summation orders of the dot product (oracle.ddot,
minres_cases.dot_chunks64); the bars, every figure printed before anything is
asserted:
  |k - k_ref| <= 1, status 0
  history over min(k, k_ref, 50) entries within max(1e-9, 10 * dev_ref) of
      hist[0]; a case whose dev_ref exceeds 1e-5 FAILS
  ||x - x_ref|| <= max(1e-8, 10 * xdev_ref) ||x_ref||
  ||b - A x|| / ||b|| <= 10 * max(rtol, the same of x_ref), by oracle.csr_spmv
sas with Jacobi runs 40 steps at rtol = 0 and is held to the history bar alone:
its k at convergence moves by 3 between the reference's own two orders.

X sits between guard words and is filled with a sentinel before every solve."""
import numpy as np
import pytest

import gmres_cases as gc
import ilu0_cases as ic
import minres_cases as mc
import oracle
from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24
SENTINEL = 777.0
KMAX, RTOL = mc.KMAX, mc.RTOL
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
    def __init__(self, spmv, minv, b, kmax=KMAX, rtol=RTOL, dots=None):
        d1, d2 = dots or (oracle.ddot, mc.dot_chunks64)
        self.x, self.k, self.hist, self.status = mc.minres_ref(
            spmv, d1, minv, b, kmax, rtol)
        self.second = mc.minres_ref(spmv, d2, minv, b, kmax, rtol)
        self.b = b
        self.true_res = np.linalg.norm(b - spmv(self.x)) / np.linalg.norm(b)

    def xdev(self):
        return float(np.linalg.norm(self.second[0] - self.x)
                     / np.linalg.norm(self.x))

    def dev(self, n):
        n = min(n, self.second[1])
        if n == 0:
            return 0.0
        return float(np.abs(self.second[2][:n] - self.hist[:n]).max()
                     / self.hist[0])


def _vs_ref(k, hist, x, status, ref, spmv, what, kmax=KMAX, rtol=RTOL,
            history_only=False):
    """every figure is printed before anything is asserted"""
    n = min(k, ref.k, 50)
    dev_ref, xdev_ref = ref.dev(n), ref.xdev()
    dev = float(np.abs(hist[:n] - ref.hist[:n]).max() / ref.hist[0]) if n else 0.0
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res = np.linalg.norm(ref.b - spmv(x)) / np.linalg.norm(ref.b)
    print(what, "k", k, "k_ref", ref.k, "k_ref (second order)", ref.second[1],
          "status", status, "history deviation", dev, "dev_ref", dev_ref,
          "x error", err, "xdev_ref", xdev_ref, "true residual", res,
          "of the reference", ref.true_res)
    assert status == ref.status == 0, (what, status, ref.status)
    assert len(hist) == k + 1, what
    assert dev_ref <= 1e-5, (what, "the reference disagrees with itself", dev_ref)
    assert dev <= max(1e-9, 10 * dev_ref), (what, dev, dev_ref)
    if history_only:
        return
    assert abs(k - ref.k) <= 1, (what, k, ref.k)
    if 0 < k < kmax:
        assert hist[k] / hist[0] < rtol, what
    assert err <= max(1e-8, 10 * xdev_ref), (what, err, xdev_ref)
    assert res <= 10 * max(rtol, ref.true_res), (what, res, ref.true_res)


class _Problem:
    """One matrix (general storage; shift11 also symmetric), its explicit dinv
    on the device, right-hand sides and references (computed once)."""

    def __init__(self, exec_, comm, name):
        self.name, self.exec_ = name, exec_
        self.csr = csr = mc.csr_by_name(name)
        self.N = N = len(csr[0]) - 1
        self.spmv = lambda q: oracle.csr_spmv(*csr, q)
        self.rhs = {kind: mc.rhs(csr, kind, self.spmv) for kind in ("ones", "rand")}
        self.rhs["zero"] = np.zeros(N)
        self.dinv = mc.dinv_by_name(name)
        self.A = {False: host.Matrix.create_matrix(
            comm, exec_, *csr, N, N, [], [], False, host.P2P_NONBLOCKING)}
        if name == "shift11":
            self.A[True] = host.Matrix.create_matrix(
                comm, exec_, *csr, N, N, [], [], True, host.P2P_NONBLOCKING)
        self.d_dinv = exec_.alloc(N + 2)
        exec_.copy_from_host(self.d_dinv, self.dinv)
        self.d_b = exec_.alloc(N + 2)
        self.d_x = exec_.alloc(N + 2 * GUARD + 2)
        self.ws = host.MinresWorkspace(exec_)
        self._ref = {}

    def ref(self, rhs, pre="none", minv=None, **kw):
        key = (rhs, pre, tuple(sorted(kw.items())))
        if key not in self._ref:
            if pre == "dinv":
                minv = lambda q: self.dinv * q
            self._ref[key] = _Ref(self.spmv, minv, self.rhs[rhs], **kw)
        return self._ref[key]

    def solve(self, comm, rhs, pre="none", kmax=KMAX, rtol=RTOL, ws=None,
              x_off=GUARD, b=None, b_off=0, d_dinv=None, symmetric=False,
              finite=True, **kw):
        """-> (k, history, x, status)"""
        e, N = self.exec_, self.N
        bb = self.rhs[rhs] if b is None else b
        e.copy_from_host(self.d_b + 8 * b_off, bb)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD + 2, SENTINEL))
        d_x = self.d_x + 8 * x_off
        if pre == "dinv" and d_dinv is None:
            d_dinv = self.d_dinv
        k, hist, status = host.minres(comm, e, self.A[symmetric],
                                      self.d_b + 8 * b_off, d_x, kmax, rtol,
                                      dinv_ptr=d_dinv, ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD + 2)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[x_off + N:] == SENTINEL), (self.name, "guard behind")
        if finite:
            assert np.all(np.isfinite(x)) and not np.any(x == SENTINEL), self.name
            assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x, status

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_dinv, self.d_b, self.d_x):
            self.exec_.free(p)


SHAPES = ("shift11", "poisson11", "saddle500", "sas")


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


# ---- 2. whole solves against the reference ------------------------------------
@pytest.mark.parametrize("case", sorted(mc.TABLE))
def test_against_the_reference(comm, problems, nt, case):
    shape, rhs, pre = case
    P = problems[shape]
    ref = P.ref(rhs, pre)
    k, hist, x, status = P.solve(comm, rhs, pre)
    assert k < KMAX
    assert np.all(np.diff(hist) <= 0.0), "the residual never grows"
    _vs_ref(k, hist, x, status, ref, P.spmv, case)


@pytest.mark.parametrize("rhs", ["ones", "rand"])
def test_sas_with_jacobi_runs_a_fixed_number_of_steps(comm, problems, nt, rhs):
    P = problems["sas"]
    ref = P.ref(rhs, "dinv", kmax=40, rtol=0.0)
    k, hist, x, status = P.solve(comm, rhs, "dinv", kmax=40, rtol=0.0)
    assert k == ref.k == 40
    _vs_ref(k, hist, x, status, ref, P.spmv, ("sas", rhs), kmax=40, rtol=0.0,
            history_only=True)


def test_symmetric_storage(comm, problems, nt):
    P = problems["shift11"]
    for rhs in ("ones", "rand"):
        k, hist, x, status = P.solve(comm, rhs, symmetric=True)
        _vs_ref(k, hist, x, status, P.ref(rhs), P.spmv, ("symmetric", rhs))


# ---- 3. preconditioners -------------------------------------------------------------
def test_sgs_ilu0_and_amg(comm, problems):
    import test_gpu_amg as ta
    P = problems["poisson11"]
    e, A, N = P.exec_, P.A[False], P.N
    sgs = host.SgsPreconditioner(e, A)
    ilu = host.Ilu0Preconditioner(e, A)
    amg = host.AmgPreconditioner(e, A)
    try:
        sref = gc.SgsRef(P.csr)
        assert np.array_equal(sgs.colors(), sref.colors)
        iref = ic.Ilu0Ref(P.csr, N, ilu.colors(), False)
        fac = iref.factor()
        assert ilu.negative_pivots() == 0
        aref = ta.restate(P.csr, N, False)
        plain = P.ref("rand")
        for name, minv, kw in (("sgs", sref, dict(sgs=sgs)),
                               ("ilu0", lambda r: iref.apply(fac, r),
                                dict(sgs=ilu)),
                               ("amg", aref.apply, dict(amg=amg))):
            ref = P.ref("rand", name, minv=minv)
            k, hist, x, status = P.solve(comm, "rand", name, **kw)
            _vs_ref(k, hist, x, status, ref, P.spmv, ("poisson11", name))
            assert k < plain.k, (name, k, plain.k)
    finally:
        for M in (sgs, ilu, amg):
            M.close()


def test_unit_dinv_has_the_bits_of_no_preconditioner(comm, problems, nt):
    P = problems["shift11"]
    e = P.exec_
    d_one = e.alloc(P.N)
    e.copy_from_host(d_one, np.ones(P.N))
    try:
        want = P.solve(comm, "rand")
        got = P.solve(comm, "rand", "dinv", d_dinv=d_one)
        _same(want, got, "unit dinv")
    finally:
        e.free(d_one)


def test_negative_pivots_are_refused(exec_, comm):
    n = 32  # blocks [[2, 1], [1, 0.25]]: the second pivot is 0.25 - 0.5
    i = np.arange(n // 2)
    csr = gc.to_csr(n, [2 * i, 2 * i, 2 * i + 1, 2 * i + 1],
                    [2 * i, 2 * i + 1, 2 * i, 2 * i + 1],
                    [np.full(n // 2, v) for v in (2.0, 1.0, 1.0, 0.25)])
    A = host.Matrix.create_matrix(comm, exec_, *csr, n, n, [], [], False,
                                  host.P2P_NONBLOCKING)
    M = host.Ilu0Preconditioner(exec_, A)
    d_b, d_x = exec_.alloc(n), exec_.alloc(n)
    try:
        assert M.negative_pivots() == n // 2
        exec_.copy_from_host(d_b, np.ones(n))
        with pytest.raises(host.SpmvHostError, match="pivot"):
            host.minres(comm, exec_, A, d_b, d_x, 10, 1e-10, sgs=M)
    finally:
        M.close()
        A.close()
        exec_.free(d_b), exec_.free(d_x)


# ---- 4. the exits on the device ---------------------------------------------------
def _dense_csr(A):
    n = len(A)
    r, c = np.nonzero(np.ones((n, n)))
    return gc.to_csr(n, [r], [c], [np.asarray(A, np.float64)[r, c]])


@pytest.mark.parametrize("name", ["lanczos", "negative", "singular", "zero_alfa"])
def test_the_exits(exec_, comm, nt, name):
    import test_minres_host as th
    A, b, dinv, (x_ref, k_ref, hist_ref, status_ref), _, status_want = \
        th.exit_case(name)
    n = len(b)
    M = host.Matrix.create_matrix(comm, exec_, *_dense_csr(A), n, n, [], [],
                                  False, host.P2P_NONBLOCKING)
    d_b, d_x, d_d = exec_.alloc(n), exec_.alloc(n), exec_.alloc(n)
    try:
        exec_.copy_from_host(d_b, b)
        exec_.copy_from_host(d_x, np.full(n, SENTINEL))
        if dinv is not None:
            exec_.copy_from_host(d_d, dinv)
        k, hist, status = host.minres(comm, exec_, M, d_b, d_x, 50, 1e-12,
                                      dinv_ptr=d_d if dinv is not None else None)
        x = exec_.copy_to_host(d_x, n)
        print(name, "k", k, "status", status, "x", x, "hist", hist)
        assert (k, status) == (k_ref, status_ref) and status == status_want
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
        assert np.allclose(x, x_ref, rtol=0, atol=1e-14)
    finally:
        M.close()
        for p in (d_b, d_x, d_d):
            exec_.free(p)


def test_a_zero_right_hand_side(comm, problems, nt):
    P = problems["shift11"]
    for pre in ("none", "dinv"):
        k, hist, x, status = P.solve(comm, "zero", pre)
        assert (k, status) == (0, 0) and list(hist) == [0.0]
        assert np.all(x == 0.0)


# ---- 5. frame ---------------------------------------------------------------------
def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), what
    assert a[3] == b[3], (what, a[3], b[3])


@pytest.mark.parametrize("pre", ["none", "dinv"])
def test_x_is_frozen_after_convergence(comm, problems, nt, pre):
    """the host runs up to 16 iterations ahead of the device's `done`: what it
    enqueues after the stop changes nothing"""
    P = problems["shift11"]
    want = P.solve(comm, "ones", pre, poll_every=1)
    assert 0 < want[0] < KMAX
    _same(want, P.solve(comm, "ones", pre, poll_every=16), (pre, "poll 16"))
    _same(want, P.solve(comm, "ones", pre), (pre, "default poll"))


def test_fixed_number_of_steps(comm, problems, nt):
    P = problems["shift11"]
    for kmax in (0, 1, 2, 7):
        k, hist, x, status = P.solve(comm, "ones", kmax=kmax, rtol=0.0)
        assert (k, status) == (kmax, 0) and hist.shape == (kmax + 1,)
        assert np.any(x != 0.0) == (kmax > 0)
        ref = P.ref("ones", kmax=kmax, rtol=0.0)
        assert ref.k == kmax
        dev = np.abs(hist - ref.hist).max() / hist[0]
        print("kmax", kmax, "history deviation", dev)
        assert dev <= 1e-9


def test_unaligned_vectors_keep_the_bits(comm, problems, nt):
    P = problems["saddle500"]
    e = P.exec_
    want = P.solve(comm, "rand", "dinv", kmax=60)
    d_d = e.alloc(P.N + 1)
    e.copy_from_host(d_d + 8, P.dinv)
    try:
        _same(want, P.solve(comm, "rand", "dinv", kmax=60, x_off=GUARD + 1),
              "unaligned x")
        _same(want, P.solve(comm, "rand", "dinv", kmax=60, b_off=1),
              "unaligned b")
        _same(want, P.solve(comm, "rand", "dinv", kmax=60, d_dinv=d_d + 8),
              "unaligned dinv")
        _same(want, P.solve(comm, "rand", "dinv", kmax=60, x_off=GUARD + 1,
                            b_off=1, d_dinv=d_d + 8), "all unaligned")
    finally:
        e.free(d_d)


def test_a_workspace_is_reused_and_grows(comm, problems):
    small, large = problems["saddle500"], problems["shift11"]
    ws = host.MinresWorkspace(small.exec_)
    try:
        want_s = small.solve(comm, "rand", "dinv", kmax=20)
        want_l = large.solve(comm, "rand")
        for _ in range(2):
            _same(want_s, small.solve(comm, "rand", "dinv", kmax=20, ws=ws),
                  "small")
            _same(want_l, large.solve(comm, "rand", ws=ws), "grown")
    finally:
        ws.close()


def test_time_spmv_counts_one_spmv_per_iteration(comm, problems):
    P = problems["shift11"]
    stats = {}
    want = P.solve(comm, "ones", kmax=5, rtol=0.0)
    got = P.solve(comm, "ones", kmax=5, rtol=0.0, time_spmv=True, stats=stats)
    _same(want, got, "timed")
    assert got[0] == 5
    assert stats["spmv_launches"] == 5 and stats["spmv_ms_total"] > 0.0


def test_error_strings(comm, problems):
    P = problems["poisson11"]
    e, A = P.exec_, P.A[False]
    S = host.SgsPreconditioner(e, A)
    i = np.arange(16)
    small = host.Matrix.create_matrix(comm, e, *gc.to_csr(16, [i], [i],
                                                          [np.full(16, 2.0)]),
                                      16, 16, [], [], False, host.P2P_NONBLOCKING)
    other = host.SgsPreconditioner(e, small)
    try:
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.minres(comm, e, A, P.d_b, P.d_x, -1, 1e-8)
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            host.minres(comm, e, A, P.d_b, P.d_x, 5, 1e-8, dinv_ptr=P.d_dinv,
                        sgs=S)
        with pytest.raises(host.SpmvHostError, match="rows"):
            host.minres(comm, e, A, P.d_b, P.d_x, 5, 1e-8, sgs=other)
        with pytest.raises(host.SpmvHostError, match="overlaps b"):
            host.minres(comm, e, A, P.d_b, P.d_b + 8, 5, 1e-8)
        with pytest.raises(host.SpmvHostError, match="overlaps dinv"):
            host.minres(comm, e, A, P.d_b, P.d_dinv, 5, 1e-8, dinv_ptr=P.d_dinv)
        # the executor's stream is restored after a refused call
        k, hist, x, status = P.solve(comm, "ones")
        assert 0 < k < KMAX and status == 0
    finally:
        S.close()
        other.close()
        small.close()


# ---- 6. several ranks -----------------------------------------------------------------
def test_slab_ranks_threaded_minres():
    """Two ranks as threads (tests/thread_world.py), shift11 in slabs, general
    storage, a blocking and an overlapping halo model, one workspace per rank:
    without a preconditioner and (40 steps) with a dinv -- the all-reduces of
    alfa and ry, `reduced` in update_r, the ghost tail of v.  Against minres_ref on
    oracle.dist_spmv with the rank-ordered dot product; every rank returns the
    same k and status."""
    from thread_world import ThreadWorld
    world = 2
    csr = mc.csr_by_name("shift11")
    N = len(csr[0]) - 1
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    dinv = np.random.default_rng(5).uniform(0.5, 2.0, N)

    def dist(dot):
        def dd(a, b):
            s = 0.0
            for r in range(world):
                s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
            return s
        return dd

    bs = {kind: mc.rhs(csr, kind, lambda q: oracle.csr_spmv(*csr, q))
          for kind in ("ones", "rand")}
    cases = {}
    for cm in models:
        def spmv(q, cm=cm):
            return oracle.dist_spmv(world, *csr, q, False, cm)
        cases[cm] = (spmv, {
            (kind, jac, kmax, rtol): _Ref(
                spmv, (lambda q: dinv * q) if jac else None, bs[kind], kmax=kmax,
                rtol=rtol, dots=(dist(oracle.ddot), dist(mc.dot_chunks64)))
            # (with this dinv k at convergence moves by 6 between the
            # reference's own two orders, as on sas: a fixed number of steps)
            for kind, jac, kmax, rtol in (("ones", False, KMAX, RTOL),
                                          ("rand", False, KMAX, RTOL),
                                          ("rand", True, 40, 0.0))})
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.MinresWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        exec_.copy_from_host(d_dinv, dinv[r0:r1])
        for cm, (spmv, refs) in cases.items():
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            for (kind, jac, kmax, rtol), ref in refs.items():
                exec_.copy_from_host(d_b, bs[kind][r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.minres(
                    comm, exec_, A, d_b, d_x + 8 * GUARD, kmax, rtol,
                    dinv_ptr=d_dinv if jac else None, ws=ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX and (rtol > 0.0 or k == kmax)
                _vs_ref(k, hist, xs, status, ref, spmv, (world, cm, kind, jac),
                        kmax=kmax, rtol=rtol, history_only=rtol == 0.0)
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
