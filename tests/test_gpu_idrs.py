"""spmv::idrs on the device: whole solves of at most 2000 rows.

  convdiff8, banded2000 and cdpe(10, 5) at s = 1, 4, 8 in general storage,
  poisson8 in symmetric storage; none / dinv / sgs / ILU(0) / amg; convdiff8 on
  two ranks.  The bar is idrs_cases.BAR on the true relative residual; the
  iteration count of EVERY converging solve is held to the restatement's within
  idrs_cases.SPREAD (equality where the spread of its two summation orders is
  zero, which test_idrs_host.py asserts for each of them).
  Bits where the summation order does not enter: poll_every 1 against 16,
  time_spmv, a reused workspace, a workspace grown in s, a clean solve after
  every exit, an x 8 bytes off.
  The exact exits (each verified on the restatement by test_idrs_host.py):
  status 2 on skew2(64), status 1 on the identity, b = 0, kmax = 0, a NaN."""
import numpy as np
import pytest

import idrs_cases as ic
import oracle
from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24
SENTINEL = 777.0
KMAX, RTOL = ic.KMAX, ic.RTOL
BAR, problem, solve = ic.BAR, ic.problem, ic.solve
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


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, exec_):
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


class _Problem:
    """One matrix on the device with its buffers and one workspace"""

    def __init__(self, exec_, comm, csr, symmetric=False):
        self.exec_, self.csr = exec_, csr
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [],
                                           bool(symmetric),
                                           host.P2P_NONBLOCKING)
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD + 1)
        self.d_dinv = exec_.alloc(N + 1)
        self.A.diagonal(self.d_dinv)
        if np.all(ic.diag_of(csr) != 0):
            host.jacobi_inverse(exec_, self.d_dinv, self.d_dinv, N)
        self.ws = host.IdrsWorkspace(exec_)
        self.spmv = ic.fast_spmv(csr)

    def solve(self, comm, b, s, kmax=KMAX, rtol=RTOL, x_off=GUARD, ws=None,
              finite=True, **kw):
        """-> (k, history, x, status)"""
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_b, b)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD + 1, SENTINEL))
        k, hist, status = host.idrs(comm, e, self.A, self.d_b,
                                    self.d_x + 8 * x_off, s, kmax, rtol,
                                    ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD + 1)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), "guard in front"
        assert np.all(buf[x_off + N:] == SENTINEL), "guard behind"
        if finite:
            assert np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
        assert len(hist) == k + 1
        return k, hist.copy(), x, status

    def res(self, b, x):
        return float(np.linalg.norm(b - self.spmv(x)) / np.linalg.norm(b))

    def close(self):
        self.ws.close()
        self.A.close()
        for p in (self.d_b, self.d_x, self.d_dinv):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def problems(exec_, comm):
    ps = {}
    for name in ic.CASES:
        csr, b, _, _ = problem(name)
        ps[name] = _Problem(exec_, comm, csr)
    yield ps
    for p in ps.values():
        p.close()


def _same(a, b, what):
    assert a[0] == b[0] and a[3] == b[3], (what, a[0], b[0], a[3], b[3])
    assert np.array_equal(a[1], b[1]), (what, "history")
    assert np.array_equal(a[2], b[2]), (what, "x")


def _converged(P, b, out, name, s, what, pre=None):
    """every figure is printed before anything is asserted"""
    k, hist, x, status = out
    ref_k = solve(name, s, "device", pre)[1]
    res = P.res(b, x)
    print(what, "k", k, "k of the restatement", ref_k, "status", status,
          "recurrence", hist[-1] / hist[0], "true residual", res)
    assert status == 0 and 0 < k < KMAX, what
    assert hist[k] / hist[0] < RTOL and np.all(hist[1:k] / hist[0] >= RTOL), what
    assert res <= BAR, (what, res)
    assert abs(k - ref_k) <= ic.spread(name, s, pre), (what, k, ref_k)


# ---- 1. against the restatement -------------------------------------------------------
@pytest.mark.parametrize("s", [1, 4, 8])
@pytest.mark.parametrize("name", ic.CASES)
def test_general_storage(comm, problems, nt, name, s):
    P = problems[name]
    b = problem(name)[1]
    out = P.solve(comm, b, s)
    if (name, s) == ("cdpe10", 1):
        # the motivating case: IDR(1) does not reach rtol in 2000 steps
        k, hist, x, status = out
        print(name, s, "k", k, "status", status, hist[-1] / hist[0])
        assert status == 1 or k == KMAX
        assert not hist[-1] / hist[0] < RTOL
        return
    _converged(P, b, out, name, s, (name, s))


@pytest.mark.parametrize("s", [1, 4])
def test_symmetric_storage(exec_, comm, nt, s):
    csr, b, _, _ = problem("poisson8")
    P = _Problem(exec_, comm, csr, symmetric=True)
    try:
        out = P.solve(comm, b, s)
        _converged(P, b, out, "poisson8", s, ("poisson8 symmetric", s))
    finally:
        P.close()


@pytest.mark.parametrize("name,s,pre", ic.PRECONDITIONED)
def test_preconditioners(exec_, comm, problems, nt, name, s, pre):
    assert s == 4
    b = problem(name)[1]
    if name in problems:
        P, own = problems[name], False
    else:
        P, own = _Problem(exec_, comm, problem(name)[0]), True
    M = None
    try:
        plain = P.solve(comm, b, 4)
        kw = {}
        if pre == "dinv":
            kw = dict(dinv_ptr=P.d_dinv)
        elif pre == "sgs":
            M = host.SgsPreconditioner(exec_, P.A)
            kw = dict(sgs=M)
        elif pre == "ilu0":
            M = host.Ilu0Preconditioner(exec_, P.A)
            kw = dict(sgs=M)
        elif pre == "amg":
            M = host.AmgPreconditioner(exec_, P.A)
            kw = dict(amg=M)
        else:
            kw = dict(dinv_ptr=P.d_dinv, cheb=ic.CHEB)
        out = P.solve(comm, b, 4, **kw)
        _converged(P, b, out, name, 4, (name, pre), pre=pre)
        print(pre, "k", out[0], "without", plain[0])
        if pre != "dinv":
            assert out[0] < plain[0], (pre, out[0], plain[0])
        # the same solve again: the same bits
        _same(P.solve(comm, b, 4, **kw), out, (pre, "again"))
    finally:
        if M is not None:
            M.close()
        if own:
            P.close()


# ---- 2. bits where the order does not enter ------------------------------------------------
def test_bits(exec_, comm, problems, nt):
    P = problems["convdiff8"]
    b = problem("convdiff8")[1]
    base = P.solve(comm, b, 4, poll_every=16)
    _same(P.solve(comm, b, 4, poll_every=1), base, "poll_every 1")
    stats = {}
    _same(P.solve(comm, b, 4, time_spmv=True, stats=stats), base, "time_spmv")
    # (the lagging poll: the copy issued at a multiple of poll_every is looked
    # at one poll later, so the host runs ahead by less than two polls)
    assert base[0] <= stats["spmv_launches"] <= base[0] + 2 * 16
    assert stats["spmv_ms_total"] > 0
    _same(P.solve(comm, b, 4, x_off=GUARD + 1), base, "x 8 bytes off")
    _same(P.solve(comm, b, 4, dinv_ptr=P.d_dinv),
          P.solve(comm, b, 4, dinv_ptr=P.d_dinv, x_off=GUARD + 1), "dinv, x off")
    # a fresh workspace, grown in s, then back
    ws = host.IdrsWorkspace(exec_)
    try:
        one = P.solve(comm, b, 1, ws=ws)
        _same(P.solve(comm, b, 4, ws=ws), base, "grown in s")
        _same(P.solve(comm, b, 1, ws=ws), one, "back to s = 1")
        short = P.solve(comm, b, 4, kmax=7, ws=ws)
        assert short[0] == 7 and short[3] == 0
        assert np.array_equal(short[1], base[1][:8])
        _same(P.solve(comm, b, 4, kmax=KMAX + 5, ws=ws)[:3] + (0,),
              base[:3] + (0,), "grown in kmax")
    finally:
        ws.close()
    # another seed is another solve
    other = P.solve(comm, b, 4, seed=5)
    assert other[3] == 0 and not np.array_equal(other[1], base[1])
    assert P.res(b, other[2]) <= BAR


# ---- 3. the exits ----------------------------------------------------------------------------
def test_the_exits_on_one_workspace(exec_, comm, nt):
    ws = host.IdrsWorkspace(exec_)
    S = _Problem(exec_, comm, ic.skew2(64))
    I = _Problem(exec_, comm, ic.identity(64))
    C = _Problem(exec_, comm, ic.convdiff(5))
    try:
        bc = C.spmv(np.random.default_rng(2).uniform(-1, 1, C.N))
        clean = C.solve(comm, bc, 4, ws=ws)
        assert clean[3] == 0 and C.res(bc, clean[2]) <= BAR

        def then_clean(what):
            _same(C.solve(comm, bc, 4, ws=ws), clean, what)

        # status 2: skew2(64), b = e_0, s = 1
        b = np.zeros(64)
        b[0] = 1.0
        ref = ic.idrs_ref(S.spmv, np.dot, None, b, 1, 50, RTOL)
        k, hist, x, status = S.solve(comm, b, 1, kmax=50, ws=ws)
        assert (k, status) == (1, 2) == (ref[1], ref[3])
        assert np.array_equal(x, ref[0]) and abs(x[0]) == 0.5
        assert not x[1:].any()
        assert np.array_equal(hist, [1.0, np.sqrt(2.0)])
        then_clean("after status 2")
        # status 1: A = I, two rows of opposite sign
        i, j = ic.opposite_rows()
        b = np.zeros(64)
        b[i] = b[j] = 1.0
        k, hist, x, status = I.solve(comm, b, 1, kmax=50, ws=ws)
        assert (k, status) == (0, 1) and not x.any() and len(hist) == 1
        then_clean("after status 1")
        # b = 0
        k, hist, x, status = C.solve(comm, np.zeros(C.N), 4, ws=ws)
        assert (k, status) == (0, 0) and not x.any()
        assert np.array_equal(hist, [0.0])
        then_clean("after b = 0")
        # kmax = 0
        k, hist, x, status = C.solve(comm, bc, 4, kmax=0, ws=ws)
        assert (k, status) == (0, 0) and not x.any()
        assert np.array_equal(hist, clean[1][:1])
        then_clean("after kmax = 0")
        # kmax in the middle of a cycle and at an om step
        for kmax in (3, 5):
            k, hist, x, status = C.solve(comm, bc, 4, kmax=kmax, ws=ws)
            assert (k, status) == (kmax, 0)
            assert np.array_equal(hist, clean[1][:kmax + 1])
        # a NaN in b: ends without a hang, at once
        bad = bc.copy()
        bad[17] = np.nan
        k, hist, x, status = C.solve(comm, bad, 4, kmax=50, ws=ws, finite=False)
        assert (k, status) == (0, 1) and not x.any()
        then_clean("after a NaN")
    finally:
        for P in (S, I, C):
            P.close()
        ws.close()


def test_error_strings(comm, problems):
    P = problems["convdiff8"]
    b = problem("convdiff8")[1]
    for kw, name in ((dict(s=0), "s must"), (dict(s=9), "s must"),
                     (dict(s=4, kmax=-1), "kmax"),
                     (dict(s=4, kappa=1.0), "kappa")):
        with pytest.raises(host.SpmvHostError, match=name):
            P.solve(comm, b, **kw)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.idrs(comm, P.exec_, P.A, P.d_b, P.d_b, 4, 5, RTOL)
    out = P.solve(comm, b, 4)
    assert out[3] == 0


# ---- 4. two ranks --------------------------------------------------------------------------------
def test_slab_ranks_threaded_idrs():
    """Ranks as threads (tests/thread_world.py), convdiff8 in two slabs, general
    storage, a blocking and an overlapping halo model, one workspace per rank:
    the reducers, the all-reduces of s, 1, 2 and s + 1 doubles, `reduced` in
    every scalar kernel, the global row of the signs.  Every rank returns the
    same k and status; the bar and the count are those of one rank."""
    from thread_world import ThreadWorld
    world = 2
    csr, b, spmv, _ = problem("convdiff8")
    N = len(csr[0]) - 1
    ranges = oracle.owner_ranges(world, N)
    dinv = 1.0 / ic.diag_of(csr)
    runs = ((1, False), (4, False), (8, False), (4, True))
    # (the restatement's solves, once, in front of the threads)
    ref_ks = {(s, j): solve("convdiff8", s, "device", "dinv" if j else None)[1]
              for s, j in runs}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.IdrsWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        exec_.copy_from_host(d_dinv, dinv[r0:r1])
        lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
        for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            for s, jacobi in runs:
                exec_.copy_from_host(d_b, b[r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.idrs(
                    comm, exec_, A, d_b, d_x + 8 * GUARD, s, KMAX, RTOL,
                    dinv_ptr=d_dinv if jacobi else None, ws=ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                res = np.linalg.norm(b - spmv(xs)) / np.linalg.norm(b)
                print(world, cm, s, jacobi, "k", k, "true residual", res)
                assert status == 0 and 0 < k < KMAX and len(hist) == k + 1
                assert hist[k] / hist[0] < RTOL
                assert res <= BAR, (s, jacobi, res)
                pre = "dinv" if jacobi else None
                ref_k = ref_ks[(s, jacobi)]
                assert abs(k - ref_k) <= ic.spread("convdiff8", s, pre), \
                    (s, jacobi, k, ref_k)
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
