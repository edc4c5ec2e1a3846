"""Whole solves of cg, cg_block, pcg, pcg_chebyshev, pcg_sgs and bicgstab on the
cases of solver_edges.py: breakdowns and zero curvature on exact matrices,
poisoned data, workspace hygiene after either, column isolation of cg_block
beside a poisoned column, and systems scaled by powers of two or negated.

No comparison here has a tolerance.  Every one is equality of integers (k,
status, iteration counts) or solver_edges.same_bits: the raw bits wherever the
expected value is not NaN, NaN (as a class) where and only where it is.  That
is stricter than equality of the NaN / Inf / finite class and holds under the
conditions test_solver_edges_host.py proves: the exact cases have
order-independent sums, the poisoned cases are NaN from a stated iteration on
and exact before it.  The scaling relations are between two GPU solves.

Fixtures, guard words and sentinel are those of test_gpu_pcg.py; X is filled
with the sentinel before every solve."""
import numpy as np
import pytest

import oracle
import solver_edges as se
import test_gpu_pcg as tp
from solver_edges import Result, same_bits
from spmv_amd import _lib, host
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
WS = {"cg": host.CgWorkspace, "pcg": host.PcgWorkspace,
      "pcg_chebyshev": host.ChebyshevWorkspace, "pcg_sgs": host.SgsWorkspace,
      "bicgstab": host.BicgstabWorkspace}
BOTH_PATHS = ("cg", "pcg", "bicgstab")  # reducer and consumer-side reductions
ONE = [s for s in se.SOLVERS if s != "cg_block"]
PLAN_KEYS = ("lat", "slat", "sdia", "sdia_const", "sdia_general", "wdia", "lx",
             "lxw", "lx4", "lx_v32", "sjds", "sym_sj", "xw", "zwalk")


class Dev:
    """One matrix on the device with its buffers; run() is one guarded solve."""

    def __init__(self, exec_, comm, csr, symmetric=False):  # noqa: F811
        self.e, self.comm, self.csr = exec_, comm, csr
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [],
                                           symmetric, host.P2P_NONBLOCKING)
        self.d_b, self.d_dinv = exec_.alloc(N * 8), exec_.alloc(N)
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD)
        self.M = None
        self.ws = {}

    def workspace(self, solver):
        cls = host.CgBlockWorkspace if solver == "cg_block" else WS[solver]
        if solver not in self.ws:
            self.ws[solver] = cls(self.e)
        return self.ws[solver]

    def _guarded(self, n, x_off):
        self.e.copy_from_host(self.d_x, np.full(n + 2 * GUARD, SENTINEL))
        return self.d_x + 8 * x_off

    def _read(self, n, x_off, what):
        buf = self.e.copy_to_host(self.d_x, n + 2 * GUARD)
        assert np.all(buf[:x_off] == SENTINEL), (what, "guard in front")
        assert np.all(buf[x_off + n:] == SENTINEL), (what, "guard behind")
        x = buf[x_off:x_off + n].copy()
        assert not np.any(x == SENTINEL), (what, "x not written")
        return x

    def run(self, solver, b, kmax, rtol, dinv=None, cheb=None, ws=None,
            x_off=GUARD, **kw):
        e, c, A = self.e, self.comm, self.A
        ws = ws or self.workspace(solver)
        if solver not in BOTH_PATHS:
            kw.pop("consumer_reductions", None)
        e.copy_from_host(self.d_b, np.asarray(b, dtype=np.float64))
        if dinv is not None:
            e.copy_from_host(self.d_dinv, dinv)
        d_dinv = self.d_dinv if dinv is not None else None
        d_x = self._guarded(self.N, x_off)
        status = 0
        if solver == "cg":
            k, hist, _, _ = host.cg_ex(c, e, A, self.d_b, d_x, kmax, rtol, ws,
                                       history=True, **kw)
        elif solver == "pcg":
            k, hist = host.pcg(c, e, A, self.d_b, d_x, d_dinv, kmax, rtol, ws,
                               **kw)
        elif solver == "pcg_chebyshev":
            k, hist = host.pcg_chebyshev(c, e, A, self.d_b, d_x, d_dinv, *cheb,
                                         kmax, rtol, ws, **kw)
        elif solver == "pcg_sgs":
            if self.M is None:
                self.M = host.SgsPreconditioner(e, A)
            k, hist = host.pcg_sgs(c, e, A, self.M, self.d_b, d_x, kmax, rtol,
                                   ws, **kw)
        else:
            k, hist, status = host.bicgstab(c, e, A, self.d_b, d_x, d_dinv, kmax,
                                            rtol, ws, **kw)
        return Result(self._read(self.N, x_off, solver), k, hist.copy(), status)

    def run_block(self, B, kmax, rtol, ws=None, x_off=GUARD, **kw):
        """-> (iterations, history, X, the value returned)"""
        n, nrhs = B.shape
        self.e.copy_from_host(self.d_b, np.ascontiguousarray(B))
        d_x = self._guarded(n * nrhs, x_off)
        its, hist, st = host.cg_block(self.comm, self.e, self.A, self.d_b, d_x,
                                      nrhs, kmax, rtol,
                                      ws or self.workspace("cg_block"), **kw)
        X = self._read(n * nrhs, x_off, ("cg_block", nrhs)).reshape(n, nrhs)
        return its.copy(), hist.copy(), X, st["max_iterations"]

    def close(self):
        for w in self.ws.values():
            w.close()
        if self.M is not None:
            self.M.close()
        self.A.close()
        for p in (self.d_b, self.d_dinv, self.d_x):
            self.e.free(p)


@pytest.fixture(scope="module")
def devs(exec_, comm):  # noqa: F811
    """Dev objects by key, created on first use, closed at the end"""
    made = {}

    def get(key, csr, symmetric=False):
        if key not in made:
            made[key] = Dev(exec_, comm, csr, symmetric)
        return made[key]
    yield get
    for d in made.values():
        d.close()


_REFS = {}


def _ref(key, solver, csr, b, kmax, rtol, **kw):
    """references are computed once and shared by both instantiations"""
    key = (key, solver, kmax, rtol)
    if key not in _REFS:
        _REFS[key] = se.reference(solver, csr, b, kmax, rtol, **kw)
    return _REFS[key]


def _same(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what


def _hygiene(devs, solver, ws, what, var):
    """A benign solve on the workspace a poisoned or broken-down solve has just
    used, with that solve's options (path and poll_every), equals the same
    solve on a fresh workspace; x aligned and 8 bytes off."""
    csr = tp._csr("poisson11")
    D = devs("benign", csr)
    b = se.scaled_rhs(csr)
    kw = se.solver_kwargs(solver, csr)
    for x_off in (GUARD, GUARD + 1):
        fresh = WS[solver](D.e)
        want = D.run(solver, b, 30, 1e-6, ws=fresh, x_off=x_off, **kw, **var)
        fresh.close()
        got = D.run(solver, b, 30, 1e-6, ws=ws, x_off=x_off, **kw, **var)
        assert 1 < want.k <= 30 and np.all(np.isfinite(want.x)), what
        _same(got, want, (what, "benign solve afterwards", x_off))


def _hygiene_block(devs, ws, nrhs, what, var):
    """the same for cg_block: `nrhs` benign columns on the workspace `ws`"""
    csr = tp._csr("poisson11")
    D = devs("benign", csr)
    cols = [se.scaled_rhs(csr), se.clean_rhs(D.N)]
    B = np.stack([cols[c % 2] for c in range(nrhs)], axis=1)
    for x_off in (GUARD, GUARD + 1):
        fresh = host.CgBlockWorkspace(D.e)
        want = D.run_block(B, 30, 1e-6, ws=fresh, x_off=x_off, **var)
        fresh.close()
        got = D.run_block(B, 30, 1e-6, ws=ws, x_off=x_off, **var)
        assert np.all(want[0] > 1) and np.all(np.isfinite(want[2])), what
        assert np.array_equal(got[0], want[0]) and got[3] == want[3], what
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]), what


def _variants(solver):
    for poll in (1, 255):
        yield {"poll_every": poll}
    if solver in BOTH_PATHS:
        yield {"poll_every": 255, "consumer_reductions": False}
        yield {"poll_every": 1, "consumer_reductions": False}


# ---- 1. exact cases -----------------------------------------------------------------
@pytest.mark.parametrize("case", se.exact_cases(), ids=lambda c: c.name)
def test_exact_cases(devs, nt, case):  # noqa: F811
    D = devs(("exact", case.block, case.nb), case.csr)
    for solver in case.solvers:
        if solver == "cg_block":
            _exact_block(devs, D, case)
            continue
        kws = [se.solver_kwargs(solver, case.csr, exact=True)]
        if solver == "bicgstab":
            kws = [{"dinv": None}, kws[0], {"dinv": np.full(case.N, 4.0)}]
        for i, kw in enumerate(kws):
            want = _ref((case.name, i), solver, case.csr, case.b, se.KMAX,
                        case.rtol, **kw)
            assert (want.k, want.status) == (case.k, case.status)
            for var in _variants(solver):
                what = (case.name, solver, i, var)
                got = D.run(solver, case.b, se.KMAX, case.rtol, **kw, **var)
                _same(got, want, what)
                if case.status:  # after a breakdown x is the last finite iterate
                    assert np.all(np.isfinite(got.x)), what
                    assert np.all(np.isfinite(got.hist)), what
                _hygiene(devs, solver, D.workspace(solver), what, var)


def _exact_block(devs, D, case):
    """cg_block on an exact case, nrhs 2 (pair kernels) and 3 (row kernels):
    the case in every column but column 1, which is zero"""
    for nrhs in (2, 3):
        B = se.exact_block(case, nrhs)
        its_r, hist_r, X_r = se.reference_block(case.csr, B, se.KMAX, case.rtol)
        for var in ({"poll_every": 1}, {"poll_every": 255}):
            for x_off in (GUARD, GUARD + 1):
                what = (case.name, "cg_block", nrhs, var, x_off)
                its, hist, X, ret = D.run_block(B, se.KMAX, case.rtol,
                                                x_off=x_off, **var)
                assert np.array_equal(its, its_r) and ret == its_r.max(), what
                assert same_bits(hist, hist_r) and same_bits(X, X_r), what
                _hygiene_block(devs, D.workspace("cg_block"), nrhs, what, var)


# ---- 2. poisoned cases ---------------------------------------------------------------
@pytest.mark.parametrize("kind", se.POISONS)
@pytest.mark.parametrize("shape", tp.SHAPES)
def test_poisoned_cases(devs, nt, shape, kind):  # noqa: F811
    plain = tp._csr(shape)
    csr, b = se.poisoned(plain, kind)
    D = devs((shape, kind == "a_nan"), csr)
    for solver in ONE:
        kw = se.solver_kwargs(solver, plain)
        want = _ref((shape, kind), solver, csr, b, se.KMAX, 1e-10, **kw)
        for var in _variants(solver):
            what = (shape, kind, solver, var)
            got = D.run(solver, b, se.KMAX, 1e-10, **kw, **var)
            _same(got, want, what)
            if kind == "b_tiny" and solver != "cg":
                assert got.k == 0 and np.all(got.x == 0.0), what
            else:
                assert got.k == se.KMAX and np.all(np.isnan(got.x)), what
            _hygiene(devs, solver, D.workspace(solver), what, var)


# ---- 3. cg_block: a poisoned column beside live ones -------------------------------------
def _block_check(devs, D, csr, live, poison, nrhs, pos, kmax, rtol, what):
    B = np.stack([poison if c == pos else live[c % len(live)]
                  for c in range(nrhs)], axis=1)
    B0 = B.copy()
    B0[:, pos] = 0.0
    its_r, hist_r, X_r = se.reference_block(csr, B[:, [pos]], kmax, rtol)
    for var in ({"poll_every": 1}, {"poll_every": 255}):
        for x_off in (GUARD, GUARD + 1):
            its, hist, X, ret = D.run_block(B, kmax, rtol, x_off=x_off, **var)
            its0, hist0, X0, _ = D.run_block(B0, kmax, rtol, x_off=x_off, **var)
            w = (what, nrhs, pos, var, x_off)
            assert its0[pos] == 0 and np.all(X0[:, pos] == 0.0), w
            for c in range(nrhs):
                if c == pos:
                    continue
                assert its[c] == its0[c] and np.all(np.isfinite(X[:, c])), (w, c)
                assert same_bits(hist[c], hist0[c]), (w, c)
                assert same_bits(X[:, c], X0[:, c]), (w, c)
            assert its[pos] == its_r[0], (w, its, its_r)
            assert same_bits(hist[pos], hist_r[0]), w
            assert same_bits(X[:, pos], X_r[:, 0]), w
            assert ret == its.max() == kmax, w
            # the poisoned solve once more, then a benign one on its workspace
            D.run_block(B, kmax, rtol, x_off=x_off, **var)
            _hygiene_block(devs, D.workspace("cg_block"), nrhs, w, var)


@pytest.mark.parametrize("nrhs", [2, 3, 4, 5, 8])
def test_cg_block_column_isolation(devs, nt, nrhs):  # noqa: F811
    """The poisoned column first, last, and as the partner of a live column in
    a 16-byte element (column 1 beside column 0; at odd nrhs the pairs shift
    from row to row, so every position is some row's partner)."""
    plain = tp._csr("poisson11")
    D = devs(("poisson11", False), plain)
    N = D.N
    live = [se.scaled_rhs(plain), se.clean_rhs(N)]
    nan_col = se.poisoned(plain, "b_nan")[1]
    case = {c.name: c for c in se.exact_cases()}["curv_k1"]
    E = devs(("exact", case.block, case.nb), case.csr)
    # live columns on the indefinite block matrix: b = (1, 1) per block is an
    # eigenvector (one exact step), b = (2, 2) another
    ev = np.append(np.tile([1.0, 1.0], case.nb), 0.0)
    for pos in sorted({0, 1, nrhs - 1}):
        _block_check(devs, D, plain, live, nan_col, nrhs, pos, se.KMAX, 1e-6,
                     "NaN column")
        _block_check(devs, E, case.csr, [ev, 2.0 * ev], case.b, nrhs, pos, se.KMAX,
                     1e-6, "zero curvature")


# ---- 4. scaling and negation ----------------------------------------------------------------
def _plan(A):
    return {key: A.plan_get(key) for key in PLAN_KEYS}


def _relation(base, got, e_x, e_h, sign, what):
    assert (got.k, got.status) == (base.k, base.status), what
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x)), what
    assert same_bits(got.hist, np.ldexp(base.hist, e_h)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("shape", se.SCALED_SHAPES)
def test_scaled_and_negated_systems(devs, nt, shape, symmetric):  # noqa: F811
    csr = tp._csr(shape)
    b = se.scaled_rhs(csr)
    D = devs((shape, "scaled", 0, 1.0, symmetric), csr, symmetric)
    plan = _plan(D.A)
    K, R = se.SCALED_KMAX, se.SCALED_RTOL
    base = {s: D.run(s, b, K, R, **se.solver_kwargs(s, csr)) for s in ONE}
    B = np.stack([b, se.clean_rhs(D.N), b], axis=1)
    base_block = D.run_block(B, K, R)
    for s in ONE:
        assert 1 < base[s].k < K, (s, base[s].k)
        got = D.run(s, -b, K, R, **se.solver_kwargs(s, csr))
        _relation(base[s], got, 0, 0, -1.0, (shape, s, "-b"))
    assert np.all(base_block[0] > 1) and np.all(base_block[0] < K)
    its, hist, X, _ = D.run_block(-B, K, R)
    assert np.array_equal(its, base_block[0]), (shape, "-B")
    assert same_bits(X, -base_block[2]) and same_bits(hist, base_block[1])
    variants = [(s, t, 1.0) for s, t in se.SCALES] + [(0, 0, -1.0)]
    for s, t, sign in variants:
        S = devs((shape, "scaled", s, sign, symmetric),
                 se.scale_csr(csr, s, sign), symmetric)
        assert _plan(S.A) == plan, (shape, s, sign, _plan(S.A), plan)
        for solver in ONE:
            if sign < 0 and solver not in se.NEGATED_A:
                continue
            what = (shape, symmetric, solver, s, t, sign)
            got = S.run(solver, np.ldexp(b, t), K, R,
                        **se.solver_kwargs(solver, csr, s=s))
            _relation(base[solver], got, t - s, t, sign, what)
            if solver == "pcg_chebyshev":
                kw = se.solver_kwargs(solver, csr, s=s, cheb_bounds=True)
                got = S.run(solver, np.ldexp(b, t), K, R, **kw)
                _relation(base[solver], got, t - s, t, sign, (what, "bounds"))
        its, hist, X, _ = S.run_block(np.ldexp(B, t), K, R)
        assert np.array_equal(its, base_block[0]), (shape, s, t, sign)
        assert S.A.plan_get("mv_form") == D.A.plan_get("mv_form")
        assert same_bits(X, sign * np.ldexp(base_block[2], t - s))
        live = base_block[1] >= 0
        assert same_bits(hist[live], np.ldexp(base_block[1][live], t))
        assert np.all(hist[~live] == -1.0)


def test_absolute_floor(devs, nt):  # noqa: F811
    """rr[0] = 2^-980 b.b < 1e-290: a solver with an absolute floor would stop"""
    csr = tp._csr("poisson11")
    D = devs(("poisson11", "scaled", 0, 1.0, False), csr)
    b = se.clean_rhs(D.N)
    for solver, (s, t, kmax) in se.FLOOR.items():
        S = devs(("poisson11", "scaled", s, 1.0, False), se.scale_csr(csr, s))
        base = D.run(solver, b, kmax, 0.0, **se.solver_kwargs(solver, csr))
        got = S.run(solver, np.ldexp(b, t), kmax, 0.0,
                    **se.solver_kwargs(solver, csr, s=s))
        assert got.k == kmax and got.hist[0] ** 2 < 1e-290
        _relation(base, got, t - s, t, 1.0, (solver, "floor"))


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
def test_narrowed_and_full_values_agree(exec_, comm, nt, symmetric):  # noqa: F811
    """The LX form streams fp32 copies of values that are exact in fp32.
    6 * 2^100 is, 6 * 2^200 is not: in general storage the plan takes the LX
    form and differs in lx_v32 alone; the scaling relation holds bit for bit.
    Symmetric storage runs the same three matrices under the same options;
    lx_v32 may be set there only where the LX form was taken."""
    csr = tp._csr("poisson11")
    b = se.scaled_rhs(csr)
    opts = ((b"lat_min_nnz", 1 << 62, 1 << 20), (b"lx_min_nnz", 0, 1 << 20))
    runs = {}
    for s, narrow in ((0, 1), (100, 1), (200, 0)):
        for k_, v_, _ in opts:
            _lib.call("spmv_hip_ctx_set_option", exec_.context, k_, v_)
        try:
            S = Dev(exec_, comm, se.scale_csr(csr, s), symmetric)
        finally:
            for k_, _, d_ in opts:
                _lib.call("spmv_hip_ctx_set_option", exec_.context, k_, d_)
        lx = S.A.plan_get("lx")
        assert lx == 1 or symmetric, s
        assert S.A.plan_get("lx_v32") == (narrow if lx == 1 else 0), s
        runs[s] = S.run("cg", np.ldexp(b, s), se.SCALED_KMAX, se.SCALED_RTOL)
        S.close()
    assert 1 < runs[0].k < se.SCALED_KMAX
    for s in (100, 200):
        _relation(runs[0], runs[s], 0, s, 1.0, ("lx_v32", symmetric, s))


# ---- 5. two ranks ------------------------------------------------------------------------------
def test_two_thread_ranks():
    """A breakdown-2 case and a NaN case of bicgstab, a zero-curvature case and
    a NaN case of pcg, on two ranks (threads): every rank returns the same k and
    status, and x has the bits of the reference -- the exact cases make the
    all-reduced scalars independent of the order, the NaN cases are NaN from
    iteration 0."""
    from thread_world import ThreadWorld
    cases = {c.name: c for c in se.exact_cases()}
    plain = tp._csr("poisson11")
    nan = se.poisoned(plain, "b_nan")
    jobs = []
    for solver, case in (("bicgstab", cases["ts0_k2"]), ("pcg", cases["curv_k2"])):
        kw = se.solver_kwargs(solver, case.csr, exact=True)
        jobs.append((solver, case.csr, case.b, case.rtol, kw,
                     se.reference(solver, case.csr, case.b, se.KMAX, case.rtol,
                                  **kw)))
        kw = se.solver_kwargs(solver, plain)
        jobs.append((solver, nan[0], nan[1], 1e-10, kw,
                     se.reference(solver, *nan, se.KMAX, 1e-10, **kw)))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        for solver, csr, b, rtol, kw, want in jobs:
            N = len(b)
            ranges = oracle.owner_ranges(2, N)
            r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
            M = r1 - r0
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, host.P2P_NONBLOCKING)
            d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
            d_x = exec_.alloc(M + 2 * GUARD)
            exec_.copy_from_host(d_b, b[r0:r1])
            exec_.copy_from_host(d_dinv, kw["dinv"][r0:r1])
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
            if solver == "pcg":
                k, hist = host.pcg(comm, exec_, A, d_b, d_x + 8 * GUARD, d_dinv,
                                   se.KMAX, rtol)
                status = 0
            else:
                k, hist, status = host.bicgstab(comm, exec_, A, d_b,
                                                d_x + 8 * GUARD, d_dinv, se.KMAX,
                                                rtol)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL)
            assert np.all(buf[GUARD + M:] == SENTINEL)
            ks = tw.gather(rank, np.array([k, status]))
            assert np.all(ks.reshape(-1, 2) == [k, status]), ks
            xs = tw.gather(rank, buf[GUARD:GUARD + M])
            _same(Result(xs, k, hist, status), want, (solver, N, rank))
            A.close()
            for p in (d_b, d_dinv, d_x):
                exec_.free(p)

    tw.run(rank_body, gpu=True)
