"""Whole solves of host.gmres on the cases of gmres_edges.py: breakdowns and
stagnation on exact matrices, r.r == 0 in a later cycle, poisoned data and the
workspace after it, systems scaled by powers of two or negated under every
preconditioner, and the ILU(0) factor and both sweeps under scaling.

No comparison here has a tolerance.  Every one is equality of integers (k,
status) or gmres_edges.same_bits: the raw bits wherever the expected value is
not NaN, NaN (as a class) where and only where it is.  The exact and poisoned
cases are held to gmres_cases.gmres_ref, whose bits do not depend on the order
of a sum there (test_gmres_edges_host.py); the scaling relations are between
two GPU solves.

X sits between guard words and is filled with a sentinel before every solve;
the `nt` fixture of test_gpu_gmres.py runs both instantiations of every vector
kernel."""
import math

import numpy as np
import pytest

import gmres_cases as gc
import gmres_edges as ge
import oracle
import test_gpu_gmres as tg
from gmres_edges import Result, same_bits
from spmv_amd import host
from test_gpu_gmres import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tg.SENTINEL, tg.GUARD
POLLS = (1, 64)  # the host looks at every step / enqueues cycles behind a stop


class Dev:
    """One matrix on the device with its buffers, workspace and (on demand)
    preconditioners; run() is one guarded solve."""

    def __init__(self, exec_, comm, csr):  # noqa: F811
        self.e, self.comm, self.csr = exec_, comm, csr
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], False,
                                           host.P2P_NONBLOCKING)
        self.d_b, self.d_dinv = exec_.alloc(N), exec_.alloc(N)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.GmresWorkspace(exec_)
        self.pre = {}

    def precond(self, kind):
        if kind not in self.pre:
            cls = {"sgs": host.SgsPreconditioner, "ilu0": host.Ilu0Preconditioner}
            self.pre[kind] = cls[kind](self.e, self.A)
        return self.pre[kind]

    def run(self, b, m, kmax, rtol, dinv=None, ws=None, what=None, **kw):
        e, N = self.e, self.N
        e.copy_from_host(self.d_b, np.asarray(b, dtype=np.float64))
        if dinv is not None:
            e.copy_from_host(self.d_dinv, np.asarray(dinv, dtype=np.float64))
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist, status = host.gmres(
            self.comm, e, self.A, self.d_b, self.d_x + 8 * GUARD, m, kmax, rtol,
            dinv_ptr=self.d_dinv if dinv is not None else None,
            ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL), (what, "guard in front")
        assert np.all(buf[GUARD + N:] == SENTINEL), (what, "guard behind")
        x = buf[GUARD:GUARD + N].copy()
        assert not np.any(x == SENTINEL), (what, "x not written")
        return Result(x, k, hist.copy(), status)

    def close(self):
        for M in self.pre.values():
            M.close()
        self.ws.close()
        self.A.close()
        for p in (self.d_b, self.d_dinv, self.d_x):
            self.e.free(p)


@pytest.fixture(scope="module")
def devs(exec_, comm):  # noqa: F811
    """Dev objects by key, created on first use, closed at the end"""
    made = {}

    def get(key, csr):
        if key not in made:
            made[key] = Dev(exec_, comm, csr)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _same(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == want.k + 1, (what, len(got.hist))
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what


# ---- 1. exact cases ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ge.exact_cases(), ids=lambda c: c.id)
def test_exact_cases(devs, nt, case):  # noqa: F811
    for tail in (False, True):
        csr, b = case.system(tail)
        D = devs(("exact", case.name, tail), csr)
        dinv = np.full(D.N, ge.EXACT_DINV)
        for d in (None, dinv):
            minv = None if d is None else ge.jacobi(d)
            want = ge.reference(csr, b, case.restart, ge.KMAX, 0.0, minv=minv)
            assert want.same(case.want(tail)), case.id  # the table
            for poll in POLLS:
                what = (case.id, tail, d is not None, poll)
                got = D.run(b, case.restart, ge.KMAX, 0.0, dinv=d, what=what,
                            poll_every=poll)
                _same(got, want, what)
                if case.status == 1:
                    assert same_bits(oracle.csr_spmv(*csr, got.x), b), what


@pytest.mark.parametrize("tail", [False, True], ids=["n2", "n3"])
def test_rr_underflows_in_the_second_cycle(devs, nt, tail):  # noqa: F811
    """the r.r == 0 stop of the start kernel outside the first cycle, with a
    positive hist[1]"""
    csr, b, m, kmax = ge.under_case(tail)
    D = devs(("under", tail), csr)
    want = ge.reference(csr, b, m, kmax, 0.0)
    assert (want.k, want.status) == (1, 0) and want.hist[1] > 0.0
    for poll in POLLS:
        got = D.run(b, m, kmax, 0.0, what=("under", tail, poll), poll_every=poll)
        _same(got, want, ("under", tail, poll))


# ---- 2. poisoned data ----------------------------------------------------------------------
_CLEAN = {}


def _pre_kwargs(pre, csr, s=0, sign=1.0, D=None):
    """host.gmres's preconditioner arguments for sign * 2^s * csr"""
    if pre == "none":
        return {}
    if pre == "jacobi":
        return {"dinv": sign * np.ldexp(ge.jacobi_dinv(csr), -s)}
    if pre in ("sgs", "ilu0"):
        return {"sgs": D.precond(pre)}
    degree, lmin, lmax = ge.CHEB
    return {"dinv": ge.jacobi_dinv(csr),
            "cheb": (degree, math.ldexp(lmin, s), math.ldexp(lmax, s))}


def _hygiene(devs, shape, pre, m, ws, nt_, what):
    """A clean solve on the workspace a poisoned solve has just used has the
    bits of the same solve on a fresh workspace."""
    plain = ge.csr_of(shape)
    D = devs((shape, "plain"), plain)
    b = ge.scaled_rhs(plain)
    kw = _pre_kwargs(pre, plain)
    key = (shape, pre, m, nt_)
    if key not in _CLEAN:
        fresh = host.GmresWorkspace(D.e)
        _CLEAN[key] = D.run(b, m, 30, 1e-6, ws=fresh, what=what, **kw)
        fresh.close()
        assert 1 < _CLEAN[key].k <= 30, what
        assert np.all(np.isfinite(_CLEAN[key].x)), what
    got = D.run(b, m, 30, 1e-6, ws=ws, what=what, **kw)
    _same(got, _CLEAN[key], (what, "clean solve afterwards"))


@pytest.mark.parametrize("kind", ge.POISONS)
@pytest.mark.parametrize("shape", ge.SHAPES)
def test_poisoned_cases(devs, nt, shape, kind):  # noqa: F811
    plain = ge.csr_of(shape)
    csr, b = ge.poisoned(plain, kind)
    D = devs((shape, "a_nan" if kind == "a_nan" else "plain"), csr)
    x_nan = ge.POISON_OUTCOME[kind][3]
    for pre in ge.PRE_POISON:
        kw = _pre_kwargs(pre, plain)
        for m in ge.RESTARTS:
            want = ge.reference(csr, b, m, ge.POISON_KMAX, ge.POISON_RTOL,
                                minv=ge.minv_of(pre, plain))
            for poll in POLLS:
                what = (shape, kind, pre, m, poll)
                got = D.run(b, m, ge.POISON_KMAX, ge.POISON_RTOL, what=what,
                            poll_every=poll, **kw)
                _same(got, want, what)
                assert np.all(np.isnan(got.x)) if x_nan else \
                    same_bits(got.x, np.zeros(D.N)), what
                _hygiene(devs, shape, pre, m, D.ws, nt, what)


# ---- 3. scaling and negation -------------------------------------------------------------------
def _relation(base, got, e_x, e_h, sign, what):
    assert (got.k, got.status) == (base.k, base.status), \
        (what, got.k, got.status, base.k, base.status)
    assert same_bits(got.hist, np.ldexp(base.hist, e_h)), what
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


@pytest.mark.parametrize("m", ge.RESTARTS)
@pytest.mark.parametrize("shape", ge.SHAPES)
def test_scaled_and_negated_systems(devs, shape, m):
    csr = ge.csr_of(shape)
    b = ge.scaled_rhs(csr)
    K, R = ge.SCALED_KMAX, ge.SCALED_RTOL
    D = devs((shape, "plain"), csr)
    base = {}
    for pre in ge.PRECONDITIONERS:
        base[pre] = D.run(b, m, K, R, what=(shape, m, pre),
                          **_pre_kwargs(pre, csr, D=D))
        assert 1 < base[pre].k < K and base[pre].status == 0, (pre, base[pre].k)
        assert base[pre].hist[-1] / base[pre].hist[0] < R, pre
        got = D.run(-b, m, K, R, **_pre_kwargs(pre, csr, D=D))
        _relation(base[pre], got, 0, 0, -1.0, (shape, m, pre, "-b"))
    for s, t, sign in [(s, t, 1.0) for s, t in ge.SCALES] + [(0, 0, -1.0)]:
        S = devs((shape, "scaled", s, sign), ge.scale_csr(csr, s, sign))
        for pre in ge.PRECONDITIONERS:
            if sign < 0 and pre not in ge.NEGATED_A:
                continue
            what = (shape, m, pre, s, t, sign)
            got = S.run(np.ldexp(b, t), m, K, R, what=what,
                        **_pre_kwargs(pre, csr, s, sign, D=S))
            _relation(base[pre], got, t - s, t, sign, what)


@pytest.mark.parametrize("shape", ge.ILU_SHAPES)
def test_ilu0_and_sgs_under_scaling(devs, shape):
    """2^s A, s = +-100: the ILU(0) factor is the unscaled one times 2^s (l~, u~
    and the pivots d~), the multipliers l~_ik / d~_k are unchanged, and
    sgs_apply of either preconditioner is 2^-s times the unscaled one."""
    csr = gc.csr_by_name(shape)
    D = devs((shape, "plain"), csr)
    e, N = D.e, D.N
    r = np.random.default_rng(N).uniform(-1, 1, N)
    d_r, d_z = e.alloc(N), e.alloc(N + 2 * GUARD)
    e.copy_from_host(d_r, r)

    def apply(M):
        e.copy_from_host(d_z, np.full(N + 2 * GUARD, SENTINEL))
        host.sgs_apply(e, M, d_r, d_z + 8 * GUARD)
        buf = e.copy_to_host(d_z, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + N:] == SENTINEL)
        return buf[GUARD:GUARD + N].copy()

    def multipliers(M, l, d):
        pos = np.zeros(N, np.int64)
        pos[np.argsort(M.colors(), kind="stable")] = np.arange(N)
        return ge.ilu0_multipliers(pos[M.pattern()[0][1]], l, d)

    ilu, sgs = D.precond("ilu0"), D.precond("sgs")
    l, u, d = ilu.factor()
    mult = multipliers(ilu, l, d)
    z_ilu, z_sgs = apply(ilu), apply(sgs)
    assert np.all(np.isfinite(z_ilu)) and np.all(np.isfinite(z_sgs))
    assert np.any(z_ilu != z_sgs) and len(l) > 0 and len(u) > 0
    try:
        for s in ge.ILU_SCALES:
            S = devs((shape, "scaled", s, 1.0), ge.scale_csr(csr, s))
            ilu_s, sgs_s = S.precond("ilu0"), S.precond("sgs")
            assert np.array_equal(ilu_s.colors(), ilu.colors()), (shape, s)
            ls, us, ds = ilu_s.factor()
            assert same_bits(ds, np.ldexp(d, s)), (shape, s, "pivots")
            assert same_bits(ls, np.ldexp(l, s)), (shape, s, "l")
            assert same_bits(us, np.ldexp(u, s)), (shape, s, "u")
            assert same_bits(multipliers(ilu_s, ls, ds), mult), (shape, s)
            assert same_bits(apply(ilu_s), np.ldexp(z_ilu, -s)), (shape, s, "ilu0")
            assert same_bits(apply(sgs_s), np.ldexp(z_sgs, -s)), (shape, s, "sgs")
    finally:
        e.free(d_r), e.free(d_z)


# ---- 4. two ranks --------------------------------------------------------------------------------
def test_two_thread_ranks():
    """perm, shift3 and cyc3 at restart 30 in two slabs cut INSIDE a block (the
    halo carries an element of every basis vector), without a preconditioner
    and with dinv = 0.5: every rank returns the same k and status, and x and
    the history have the bits of one rank."""
    from thread_world import ThreadWorld
    by = {c.id: c for c in ge.exact_cases()}
    jobs = []
    for name in ge.TWO_RANKS:
        case = by[f"{name}-m30"]
        csr, b = case.system(True)
        cut = int(oracle.owner_ranges(2, len(b))[1])
        assert cut % len(case.block) != 0, (name, cut)
        ghosts = [len(oracle.localise_rows(*csr, r0, r1)[3])
                  for r0, r1 in ((0, cut), (cut, len(b)))]
        assert ghosts[1] > 0, (name, ghosts)
        jobs.append((case, csr, b, case.want(True)))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        for case, csr, b, want in jobs:
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
            exec_.copy_from_host(d_dinv, np.full(M, ge.EXACT_DINV))
            for dinv in (None, d_dinv):
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.gmres(comm, exec_, A, d_b, d_x + 8 * GUARD,
                                             case.restart, ge.KMAX, 0.0,
                                             dinv_ptr=dinv)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                _same(Result(xs, k, hist, status), want,
                      (case.id, rank, dinv is not None))
            A.close()
            for p in (d_b, d_dinv, d_x):
                exec_.free(p)

    tw.run(rank_body, gpu=True)
