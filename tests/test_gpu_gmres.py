"""spmv::gmres (restarted GMRES with a right preconditioner) on one rank.

Shapes are test_gpu_bicgstab.py's, restated in gmres_cases.py: convdiff11
(1 331 rows), convdiff24 (13 824), banded4097, each plain and scaled to S A S;
right-hand sides A.1 and A.uniform(-1, 1); restarts 5 and 30; KMAX = 400, RTOL =
1e-10; without a preconditioner and with Jacobi's dinv.  The reference is
gmres_cases.gmres_ref on oracle.csr_spmv, run with two summation orders of the
dot product (oracle.ddot, gmres_cases.dot_chunked); the bars:
  |k - k_ref| <= 1
  ||x - x_ref|| <= 1e-8 ||x_ref||
  history over min(k, k_ref, 50) entries within max(1e-9, 10 * dev_ref) of
      hist[0]; a case whose dev_ref exceeds 1e-5 FAILS
  ||b - A x|| / ||b|| <= 10 * max(rtol, the same of x_ref), by oracle.csr_spmv
CPU reference iteration counts for orientation: convdiff11 58-93, convdiff24
104-177, banded4097 15-16 with this module's right-hand sides.

Which combinations: Jacobi's dinv on both variants, no preconditioner on the
plain matrices -- the combinations of test_gpu_bicgstab.py, every one of which
converges, and for every one of which the reference's two summation orders
agree on x to 1e-14.  S A S WITHOUT a preconditioner has a test of its own
(test_scaled_without_a_preconditioner): no solve reaches 1e-10 in 400 steps
there (that is what the preconditioner is for) and GMRES stagnates at a
residual of 1e-4 to 1e-5.  The issue's pre-check ("x by at most 1e-14 relative"
between two summation orders) does NOT hold for that combination: the
reference's own two orders give x that differ by 1.9e-4 (convdiff11, uniform
right-hand side, restart 5; 4e-11 or less in the other eleven cases), with the
same k and histories equal to 2e-16.  What a stagnating run determines is k,
the status, the history and the residual, and that test holds those to the
fixed bars above; it makes NO assertion on x (the figure is printed), instead
of a wider one.

Several ranks: test_slab_ranks_threaded_gmres, as test_gpu_bicgstab.py runs
them.

X sits between guard words and is filled with a sentinel before every solve."""
import numpy as np
import pytest

import gmres_cases as gc
import oracle
from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24
SENTINEL = 777.0
KMAX, RTOL = gc.KMAX, gc.RTOL
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
    def __init__(self, spmv, minv, b, m, kmax=KMAX, rtol=RTOL):
        self.x, self.k, self.hist, self.status = gc.gmres_ref(
            spmv, oracle.ddot, minv, b, m, kmax, rtol)
        self.second = gc.gmres_ref(spmv, gc.dot_chunked, minv, b, m, kmax, rtol)
        self.b = b
        self.true_res = np.linalg.norm(b - spmv(self.x)) / np.linalg.norm(b)

    def xdev(self):
        """relative distance of the x of the two summation orders"""
        return float(np.linalg.norm(self.second[0] - self.x)
                     / np.linalg.norm(self.x))

    def dev(self, n):
        """deviation of the two histories over their first n entries, relative
        to hist[0]"""
        n = min(n, self.second[1])
        if n == 0:
            return 0.0
        return float(np.abs(self.second[2][:n] - self.hist[:n]).max()
                     / self.hist[0])


def _vs_ref(k, hist, x, status, ref, spmv, what, kmax=KMAX, rtol=RTOL,
            x_determined=True):
    """every figure is printed before anything is asserted"""
    n = min(k, ref.k, 50)
    dev_ref = ref.dev(n)
    dev = float(np.abs(hist[:n] - ref.hist[:n]).max() / ref.hist[0]) if n else 0.0
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res = np.linalg.norm(ref.b - spmv(x)) / np.linalg.norm(ref.b)
    print(what, "k", k, "k_ref", ref.k, "k_ref (second order)", ref.second[1],
          "status", status, "history deviation", dev, "dev_ref", dev_ref,
          "x error", err, "true residual", res, "of the reference",
          ref.true_res)
    assert status == ref.status == 0, (what, status, ref.status)
    assert abs(k - ref.k) <= 1, (what, k, ref.k)
    assert len(hist) == k + 1, what
    if 0 < k < kmax:
        assert hist[k] / hist[0] < rtol, what
    if x_determined:
        assert err <= 1e-8, (what, err)
    assert res <= 10 * max(rtol, ref.true_res), (what, res, ref.true_res)
    assert dev_ref <= 1e-5, (what, "the reference disagrees with itself", dev_ref)
    assert dev <= max(1e-9, 10 * dev_ref), (what, dev, dev_ref)


class _Problem:
    """One shape: the matrix plain and scaled, Jacobi's dinv of both on the
    device, right-hand sides and references (computed once, never changed)."""

    def __init__(self, exec_, comm, name, variants=("plain", "sas")):
        self.name, self.exec_ = name, exec_
        plain = gc.csr_by_name(name)
        self.csr = {"plain": plain}
        if "sas" in variants:
            self.csr["sas"] = gc.scaled(plain)
        self.N = N = len(plain[0]) - 1
        u = np.random.default_rng(N + 1).uniform(-1, 1, N)
        self.rhs, self.A, self.d_dinv, self.diag = {}, {}, {}, {}
        for var, csr in self.csr.items():
            self.rhs[var] = {"ones": oracle.csr_spmv(*csr, np.ones(N)),
                             "rand": oracle.csr_spmv(*csr, u),
                             "zero": np.zeros(N)}
            self.diag[var] = gc.diag_of(csr)
            self.A[var] = host.Matrix.create_matrix(
                comm, exec_, *csr, N, N, [], [], False, host.P2P_NONBLOCKING)
            if np.all(self.diag[var] > 0):
                self.d_dinv[var] = exec_.alloc(N + 1)
                self.A[var].diagonal(self.d_dinv[var])
                host.jacobi_inverse(exec_, self.d_dinv[var], self.d_dinv[var], N)
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.GmresWorkspace(exec_)
        self._ref = {}

    def spmv(self, var):
        return lambda q: oracle.csr_spmv(*self.csr[var], q)

    def ref(self, var, rhs, m, pre="jacobi", minv=None, **kw):
        key = (var, rhs, m, pre, tuple(sorted(kw.items())))
        if key not in self._ref:
            if pre == "jacobi":
                dinv = 1.0 / self.diag[var]
                minv = lambda q: dinv * q
            elif pre == "none":
                minv = None
            self._ref[key] = _Ref(self.spmv(var), minv, self.rhs[var][rhs], m,
                                  **kw)
        return self._ref[key]

    def solve(self, comm, var, rhs, m, pre="jacobi", kmax=KMAX, rtol=RTOL,
              ws=None, x_off=GUARD, b=None, b_off=0, d_dinv=None, **kw):
        """-> (k, history, x, status)"""
        e, N = self.exec_, self.N
        bb = self.rhs[var][rhs] if b is None else b
        e.copy_from_host(self.d_b + 8 * b_off, bb)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        d_x = self.d_x + 8 * x_off
        if pre == "jacobi" and d_dinv is None:
            d_dinv = self.d_dinv[var]
        k, hist, status = host.gmres(comm, e, self.A[var], self.d_b + 8 * b_off,
                                     d_x, m, kmax, rtol, dinv_ptr=d_dinv,
                                     ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[x_off + N:] == SENTINEL), (self.name, "guard behind")
        assert np.all(np.isfinite(x)) and not np.any(x == SENTINEL), self.name
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x, status

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in list(self.d_dinv.values()) + [self.d_b, self.d_x]:
            self.exec_.free(p)


SHAPES = ("convdiff11", "convdiff24", "banded4097")


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


# ---- 1. against the reference -------------------------------------------------
@pytest.mark.parametrize("m", [5, 30])
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("var", ["plain", "sas"])
@pytest.mark.parametrize("shape", SHAPES)
def test_jacobi_against_the_reference(comm, problems, nt, shape, var, rhs, m):
    P = problems[shape]
    ref = P.ref(var, rhs, m)
    k, hist, x, status = P.solve(comm, var, rhs, m)
    assert k < KMAX
    _vs_ref(k, hist, x, status, ref, P.spmv(var), (shape, var, rhs, m, "jacobi"))


@pytest.mark.parametrize("m", [5, 30])
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("shape", SHAPES)
def test_unpreconditioned_against_the_reference(comm, problems, nt, shape, rhs,
                                                m):
    P = problems[shape]
    ref = P.ref("plain", rhs, m, pre="none")
    k, hist, x, status = P.solve(comm, "plain", rhs, m, pre="none")
    assert k < KMAX
    _vs_ref(k, hist, x, status, ref, P.spmv("plain"), (shape, rhs, m, "none"))


@pytest.mark.parametrize("m", [5, 30])
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("shape", SHAPES)
def test_scaled_without_a_preconditioner(comm, problems, nt, shape, rhs, m):
    """S A S without a preconditioner runs to kmax (see the top of this file):
    k, status, history and true residual to the fixed bars; no assertion on x,
    which a stagnating run does not determine."""
    P = problems[shape]
    ref = P.ref("sas", rhs, m, pre="none")
    k, hist, x, status = P.solve(comm, "sas", rhs, m, pre="none")
    print(shape, rhs, m, "x of the reference's two orders differ by", ref.xdev())
    assert k == ref.k == KMAX and not hist[-1] / hist[0] < RTOL
    _vs_ref(k, hist, x, status, ref, P.spmv("sas"), (shape, "sas", rhs, m, "none"),
            x_determined=False)


# ---- 2. where bicgstab breaks down -----------------------------------------------
@pytest.mark.parametrize("n", [4096, 1330])
def test_skew_matrix_converges_where_bicgstab_stops(exec_, comm, nt, n):
    """b.(A b) = 0 on a skew-symmetric matrix: bicgstab stops at k = 0 with
    status 1; gmres converges (CPU reference: 44 steps at restart 30, 72 at 5)."""
    P = _Problem(exec_, comm, f"skew{n}", variants=("plain",))
    try:
        e = P.exec_
        e.copy_from_host(P.d_b, P.rhs["plain"]["ones"])
        kb, _, sb = host.bicgstab(comm, e, P.A["plain"], P.d_b, P.d_x + 8 * GUARD,
                                  None, KMAX, RTOL)
        assert (kb, sb) == (0, 1)
        for m in (30, 5):
            ref = P.ref("plain", "ones", m, pre="none")
            k, hist, x, status = P.solve(comm, "plain", "ones", m, pre="none")
            print("skew", n, m, "k", k, "k_ref", ref.k)
            assert 0 < k < KMAX
            _vs_ref(k, hist, x, status, ref, P.spmv("plain"), ("skew", n, m))
    finally:
        P.close()


# ---- 3. SGS and Chebyshev as right preconditioners -----------------------------
@pytest.mark.parametrize("shape", ["convdiff11", "convdiff24"])
def test_sgs_right_preconditioner(comm, problems, nt, shape):
    P = problems[shape]
    M = host.SgsPreconditioner(P.exec_, P.A["plain"])
    try:
        sref = gc.SgsRef(P.csr["plain"])
        assert np.array_equal(M.colors(), sref.colors)
        ref = P.ref("plain", "rand", 30, pre="sgs", minv=sref)
        plain = P.ref("plain", "rand", 30, pre="none")
        k, hist, x, status = P.solve(comm, "plain", "rand", 30, pre="sgs", sgs=M)
        _vs_ref(k, hist, x, status, ref, P.spmv("plain"), (shape, "sgs"))
        assert k < plain.k, (k, plain.k)
    finally:
        M.close()


@pytest.mark.parametrize("n", [11, 24])
def test_chebyshev_right_preconditioner(exec_, comm, nt, n):
    P = _Problem(exec_, comm, f"poisson{n}", variants=("plain",))
    try:
        e = P.exec_
        e.copy_from_host(P.d_b, P.rhs["plain"]["rand"])
        d = P.d_dinv["plain"]
        lam = host.lambda_max_estimate(comm, e, P.A["plain"], d, P.d_b, 20)
        lmax = 1.1 * lam
        lmin = lmax / 30
        dinv = 1.0 / P.diag["plain"]
        sp = P.spmv("plain")
        minv = lambda q: gc.chebyshev_apply(sp, q, dinv, 4, lmin, lmax)
        ref = P.ref("plain", "rand", 30, pre="cheb", minv=minv)
        k, hist, x, status = P.solve(comm, "plain", "rand", 30, pre="cheb",
                                     d_dinv=d, cheb=(4, lmin, lmax))
        _vs_ref(k, hist, x, status, ref, sp, ("poisson", n, "chebyshev"))
    finally:
        P.close()


# ---- 4. edges --------------------------------------------------------------------
def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what
    assert a[3] == b[3], (what, a[3], b[3])


@pytest.mark.parametrize("pre", ["jacobi", "none"])
def test_fixed_number_of_steps(comm, problems, nt, pre):
    """rtol = 0 runs to kmax: kmax = 0, restart = 1, restart > kmax, kmax not a
    multiple of restart; against the reference, which stops the same way"""
    P = problems["convdiff11"]
    for m, kmax in ((5, 0), (1, 3), (30, 7), (5, 7), (5, 10), (64, 9)):
        k, hist, x, status = P.solve(comm, "plain", "ones", m, pre=pre, kmax=kmax,
                                     rtol=0.0)
        what = (pre, m, kmax)
        assert (k, status) == (kmax, 0) and hist.shape == (kmax + 1,), what
        assert np.any(x != 0.0) == (kmax > 0), what
        ref = P.ref("plain", "ones", m, pre=pre, kmax=kmax, rtol=0.0)
        assert ref.k == kmax
        if kmax:
            err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
            dev = np.abs(hist - ref.hist).max() / hist[0]
            print(what, "x error", err, "history deviation", dev)
            assert err <= 1e-8 and dev <= 1e-9, (what, err, dev)
        # b = 0: k = 0, x = 0
        k, hist, x, status = P.solve(comm, "plain", "zero", m, pre=pre, kmax=kmax,
                                     rtol=0.0)
        assert (k, status) == (0, 0) and np.all(x == 0.0), what
        assert hist.shape == (1,) and hist[0] == 0.0, what


def _diag_matrix(exec_, comm, d):
    n = len(d)
    rp = np.arange(n + 1, dtype=np.int32)
    ci = np.arange(n, dtype=np.int32)
    return host.Matrix.create_matrix(comm, exec_, rp, ci, np.asarray(d, float), n,
                                     n, [], [], False, host.P2P_NONBLOCKING)


def test_identity_and_diagonal_matrices(exec_, comm, nt):
    n = 4096
    d_b, d_x = exec_.alloc(n), exec_.alloc(n)
    try:
        # A = I, ||b|| = 64 and b / 64 exact: lucky breakdown at k = 1, x == b
        b = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        A = _diag_matrix(exec_, comm, np.ones(n))
        exec_.copy_from_host(d_b, b)
        k, hist, status = host.gmres(comm, exec_, A, d_b, d_x, 30, 50, 1e-10)
        x = exec_.copy_to_host(d_x, n)
        assert (k, status) == (1, 1), (k, status)
        assert np.array_equal(x.view(np.uint64), b.view(np.uint64))
        assert hist[0] == 64.0 and hist[1] == 0.0
        A.close()
        # A = diag(d) with 5 distinct values, restart 64: at most 5 steps (the
        # tolerance or the lucky breakdown, whichever the rounding gives)
        vals = np.array([1.0, 2.0, 3.0, 5.0, 8.0])
        d = vals[np.arange(n) % 5]
        b = np.random.default_rng(3).uniform(-1, 1, n)
        A = _diag_matrix(exec_, comm, d)
        exec_.copy_from_host(d_b, b)
        k, hist, status = host.gmres(comm, exec_, A, d_b, d_x, 64, 50, 1e-12)
        x = exec_.copy_to_host(d_x, n)
        print("diag", k, status, hist)
        assert 1 <= k <= 6 and status in (0, 1)
        assert np.linalg.norm(d * x - b) <= 1e-10 * np.linalg.norm(b)
        A.close()
    finally:
        exec_.free(d_b), exec_.free(d_x)


def test_x_frozen_after_convergence(comm, problems, nt):
    """poll_every = 1 .. 64: however far the host runs ahead of the device's
    stop, and however many cycles it enqueues behind it, x, k and the history
    are those of the stop"""
    P = problems["convdiff11"]
    for m in (5, 30):
        want = P.solve(comm, "plain", "rand", m, rtol=1e-6, poll_every=1)
        assert 1 < want[0] < KMAX and want[3] == 0
        for every in (3, 16, 64, 255):
            got = P.solve(comm, "plain", "rand", m, rtol=1e-6, poll_every=every)
            _same(want, got, (m, every))
        got = P.solve(comm, "plain", "rand", m, rtol=1e-6, x_off=GUARD + 1)
        _same(want, got, (m, "unaligned x"))


def test_unaligned_b_and_dinv_keep_the_bits(exec_, comm, problems, nt):
    P = problems["banded4097"]
    d = exec_.alloc(P.N + 1)
    exec_.copy(d + 8, P.d_dinv["sas"], P.N * 8)
    try:
        for kmax in (KMAX, 9):
            want = P.solve(comm, "sas", "rand", 5, kmax=kmax)
            got = P.solve(comm, "sas", "rand", 5, kmax=kmax, d_dinv=d + 8)
            _same(want, got, (kmax, "unaligned dinv"))
            got = P.solve(comm, "sas", "rand", 5, kmax=kmax, b_off=1)
            _same(want, got, (kmax, "unaligned b"))
    finally:
        exec_.free(d)


def test_unit_dinv_has_the_bits_of_no_preconditioner(exec_, comm, problems, nt):
    P = problems["convdiff11"]
    d_one = exec_.alloc(P.N)
    exec_.copy_from_host(d_one, np.ones(P.N))
    want = P.solve(comm, "plain", "rand", 30, pre="none")
    got = P.solve(comm, "plain", "rand", 30, pre="none", d_dinv=d_one)
    _same(want, got, "dinv = 1")
    exec_.free(d_one)


def test_workspace_reused_and_grown(comm, problems, nt):
    e = problems["convdiff11"].exec_
    shared = host.GmresWorkspace(e)
    plan = [("convdiff11", 30, 5, "none"), ("convdiff24", 40, 30, "jacobi"),
            ("banded4097", 12, 64, "jacobi"), ("convdiff24", 7, 3, "none"),
            ("convdiff11", 40, 30, "jacobi"), ("convdiff11", 0, 5, "jacobi")]
    for shape, kmax, m, pre in plan:
        P = problems[shape]
        fresh = host.GmresWorkspace(e)
        want = P.solve(comm, "plain", "rand", m, pre=pre, kmax=kmax, rtol=1e-6,
                       ws=fresh)
        fresh.close()
        got = P.solve(comm, "plain", "rand", m, pre=pre, kmax=kmax, rtol=1e-6,
                      ws=shared)
        _same(want, got, (shape, kmax, m, pre))
    shared.close()


def test_time_spmv_counts(comm, problems):
    P = problems["convdiff11"]
    stats = {}
    k, hist, x, status = P.solve(comm, "plain", "rand", 5, kmax=12, rtol=0.0,
                                 time_spmv=True, stats=stats)
    assert k == 12 and stats["spmv_launches"] == 12, stats
    assert stats["spmv_ms_total"] > 0.0
    want = P.solve(comm, "plain", "rand", 5, kmax=12, rtol=0.0)
    _same(want, (k, hist, x, status), "time_spmv changes nothing")


def test_error_strings(exec_, comm, problems):
    P = problems["convdiff11"]
    e, A, N = exec_, P.A["plain"], P.N
    dinv = P.d_dinv["plain"]

    def fails(word, *args, **kw):
        before = e.get_stream() if hasattr(e, "get_stream") else None
        with pytest.raises(host.SpmvHostError) as err:
            host.gmres(comm, e, A, *args, **kw)
        assert word in str(err.value), (word, str(err.value))
        if before is not None:
            assert e.get_stream() == before

    fails("overlaps", P.d_b, P.d_b, 5, 10, 1e-8)
    fails("overlaps", P.d_b, P.d_b + 8, 5, 10, 1e-8)
    fails("overlaps", P.d_b, dinv, 5, 10, 1e-8, dinv_ptr=dinv)
    fails("kmax", P.d_b, P.d_x, 5, -1, 1e-8)
    fails("restart", P.d_b, P.d_x, 0, 10, 1e-8)
    fails("restart", P.d_b, P.d_x, 65, 10, 1e-8)
    fails("degree", P.d_b, P.d_x, 5, 10, 1e-8, cheb=(17, 0.1, 2.0))
    fails("bounds", P.d_b, P.d_x, 5, 10, 1e-8, cheb=(4, 2.0, 1.0))
    other = problems["banded4097"]
    M = host.SgsPreconditioner(e, other.A["plain"])
    try:
        fails("rows", P.d_b, P.d_x, 5, 10, 1e-8, sgs=M)
    finally:
        M.close()
    M = host.SgsPreconditioner(e, A)
    try:
        fails("preconditioner", P.d_b, P.d_x, 5, 10, 1e-8, sgs=M, dinv_ptr=dinv)
        fails("preconditioner", P.d_b, P.d_x, 5, 10, 1e-8, sgs=M,
              cheb=(4, 0.1, 2.0))
    finally:
        M.close()
    # the solver still works afterwards
    k, _, _, status = P.solve(comm, "plain", "ones", 30)
    assert 0 < k < KMAX and status == 0


# ---- 5. several ranks ---------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_gmres(world):
    """Ranks as threads (tests/thread_world.py), convdiff8 in slabs, general
    storage, a blocking and an overlapping halo model, ONE workspace per rank
    over all solves: plain with the Jacobi dinv (restarts 5 and 30), S A S with
    it (30), plain without a preconditioner (5) -- the all-reduces of j + 1, j + 1 and 1
    doubles, `reduced` in start and givens, the ghost tail of every v_j.
    Against gmres_ref on oracle.dist_spmv with the rank-ordered dot product;
    every rank returns the same k and status."""
    from thread_world import ThreadWorld
    plain = gc.csr_by_name("convdiff8")
    N = len(plain[0]) - 1
    csrs = {"plain": plain, "sas": gc.scaled(plain)}
    u = np.random.default_rng(world).uniform(-1, 1, N)
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)

    def dist_dot(a, b):
        s = 0.0
        for r in range(world):
            s += oracle.ddot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
        return s

    def dist_dot2(a, b):
        s = 0.0
        for r in range(world):
            s += gc.dot_chunked(a[ranges[r]:ranges[r + 1]],
                                b[ranges[r]:ranges[r + 1]])
        return s

    class Ref(_Ref):
        def __init__(self, spmv, minv, b, m):
            self.x, self.k, self.hist, self.status = gc.gmres_ref(
                spmv, dist_dot, minv, b, m, KMAX, RTOL)
            self.second = gc.gmres_ref(spmv, dist_dot2, minv, b, m, KMAX, RTOL)
            self.b = b
            self.true_res = np.linalg.norm(b - spmv(self.x)) / np.linalg.norm(b)

    cases = {}
    # (every reference costs two numpy solves: restarts are spread over the
    # variants instead of crossed with them)
    for var, jacobi, ms in (("plain", True, (5, 30)), ("sas", True, (30,)),
                            ("plain", False, (5,))):
        rp, ci, va = csrs[var]
        dinv = 1.0 / gc.diag_of(csrs[var])
        minv = (lambda q, dinv=dinv: dinv * q) if jacobi else None
        bs = [oracle.csr_spmv(rp, ci, va, np.ones(N)),
              oracle.csr_spmv(rp, ci, va, u)]
        for cm in models:
            def spmv(q, rp=rp, ci=ci, va=va, cm=cm):
                return oracle.dist_spmv(world, rp, ci, va, q, False, cm)
            cases[(var, jacobi, cm)] = (spmv, bs, {
                (j, m): Ref(spmv, minv, b, m)
                for j, b in enumerate(bs) for m in ms})
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.GmresWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for (var, jacobi, cm), (spmv, bs, refs) in cases.items():
            lrp, lci, lva, gh = oracle.localise_rows(*csrs[var], r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            A.diagonal(d_dinv)
            host.jacobi_inverse(exec_, d_dinv, d_dinv, M)
            for (j, m), ref in refs.items():
                exec_.copy_from_host(d_b, bs[j][r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.gmres(
                    comm, exec_, A, d_b, d_x + 8 * GUARD, m, KMAX, RTOL,
                    dinv_ptr=d_dinv if jacobi else None, ws=ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX
                _vs_ref(k, hist, xs, status, ref, spmv,
                        (world, var, jacobi, cm, j, m))
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
