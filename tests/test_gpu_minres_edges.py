"""Whole solves of host.minres on the cases of minres_edges.py: every exit on
exact block matrices a few workgroups long (with the odd tail), the floor of
scaling, poisoned data and the workspace after it, systems scaled by powers of
two or negated under every preconditioner, and two ranks.

No comparison here has a tolerance.  Every one is equality of integers (k,
status, len(hist) == k + 1) or minres_edges.same_bits: the raw bits wherever
the expected value is not NaN, NaN (as a class) where and only where it is.
The exact, floor and poisoned cases are held to minres_cases.minres_ref, whose
bits do not depend on the order of a sum there (test_minres_edges_host.py; the
two poisoned cases where they do are held to k, status and the NaN / Inf
pattern); the scaling relations are between two GPU solves.

X sits between guard words and is filled with a sentinel before every solve;
the `nt` fixture of test_gpu_minres.py runs both instantiations of every vector
kernel; poll_every = 16 lets the host enqueue 16 iterations behind a stop."""
import numpy as np
import pytest

import minres_cases as mc
import minres_edges as me
import oracle
import test_gpu_minres as tm
from minres_edges import Result, same_bits
from spmv_amd import host
from test_gpu_minres import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tm.SENTINEL, tm.GUARD
POLLS = (1, 16)
BY_NAME = {c.name: c for c in me.exact_cases()}


class Dev:
    """One matrix on the device with its buffers, workspace and (on demand)
    preconditioners; run() is one guarded solve."""

    def __init__(self, exec_, comm, csr, symmetric=False):  # noqa: F811
        self.e, self.comm, self.csr = exec_, comm, csr
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [],
                                           symmetric, host.P2P_NONBLOCKING)
        self.d_b, self.d_dinv = exec_.alloc(N), exec_.alloc(N)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.MinresWorkspace(exec_)
        self.pre = {}

    def precond(self, kind):
        """-> host.minres's keyword for an applied preconditioner"""
        if kind not in self.pre:
            cls = {"sgs": host.SgsPreconditioner, "ilu0": host.Ilu0Preconditioner,
                   "amg": host.AmgPreconditioner}
            self.pre[kind] = cls[kind](self.e, self.A)
            if kind == "ilu0":
                assert self.pre[kind].negative_pivots() == 0
        return {"amg" if kind == "amg" else "sgs": self.pre[kind]}

    def run(self, b, kmax, rtol, dinv=None, ws=None, what=None, **kw):
        e, N = self.e, self.N
        e.copy_from_host(self.d_b, np.asarray(b, dtype=np.float64))
        if dinv is not None:
            e.copy_from_host(self.d_dinv, np.asarray(dinv, dtype=np.float64))
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist, status = host.minres(
            self.comm, e, self.A, self.d_b, self.d_x + 8 * GUARD, kmax, rtol,
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

    def get(key, csr, symmetric=False):
        if key not in made:
            made[key] = Dev(exec_, comm, csr, symmetric)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _same(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == got.k + 1, (what, len(got.hist))
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what


def _both_polls(D, want, what, *args, **kw):
    """the solve with poll_every = 1 and 16 against `want`, and against each
    other: nothing enqueued behind the stop moves x, hist or status"""
    runs = []
    for poll in POLLS:
        runs.append(D.run(*args, what=(what, poll), poll_every=poll, **kw))
        _same(runs[-1], want, (what, poll))
    assert runs[0].same(runs[1]), what
    return runs[0]


# ---- 1. exact cases and the floor ----------------------------------------------------------
@pytest.mark.parametrize("case", me.exact_cases(), ids=lambda c: c.id)
def test_exact_cases(devs, nt, case):  # noqa: F811
    for tail in (False, True):
        csr, b = case.system(tail)
        D = devs(("exact", case.block, case.nb, tail), csr)
        for kmax in case.kmaxes():
            want = me.reference(csr, b, kmax, 0.0, minv=case.minv(tail))
            assert want.same(case.want(tail)), case.id  # the table
            got = _both_polls(D, want, (case.id, tail, kmax), b, kmax, 0.0,
                              dinv=case.dinv(tail))
            if case.status == 1:
                assert same_bits(oracle.csr_spmv(*csr, got.x), b), case.id


@pytest.mark.parametrize("s", me.FLOOR_S)
@pytest.mark.parametrize("name", me.FLOOR_CASES)
def test_floor_cases(devs, nt, name, s):  # noqa: F811
    for case in (BY_NAME[name], BY_NAME[name + "-d"]):
        for tail in (False, True):
            csr, b, d, want = me.floor_case(case, s, tail)
            ref = me.reference(csr, b, me.KMAX, 0.0,
                               minv=None if d is None else me.jacobi(d))
            assert ref.same(want), (case.id, s)  # the table
            D = devs(("floor", case.block, case.nb, tail, s), csr)
            _both_polls(D, want, (case.id, s, tail), b, me.KMAX, 0.0, dinv=d)


# ---- 2. poisoned data ----------------------------------------------------------------------
def _dinv_of(pre, shape, s=0):
    return None if pre != "jacobi" else np.ldexp(mc.dinv_by_name(shape), -s)


def _poisoned_dev(devs, shape, kind):
    csr, b = me.poisoned(me.csr_of(shape), kind)
    key = (shape, "a_nan" if kind == "a_nan" else "plain", False)
    return devs(key, csr), csr, b


@pytest.mark.parametrize("kind", me.POISONS)
@pytest.mark.parametrize("shape", me.POISON_SHAPES)
def test_poisoned_cases(devs, nt, shape, kind):  # noqa: F811
    D, csr, b = _poisoned_dev(devs, shape, kind)
    at_kmax, status, _, x_nan = me.POISON_OUTCOME[kind]
    for pre in me.PRE_POISON:
        want = me.reference(csr, b, me.POISON_KMAX, me.POISON_RTOL,
                            minv=me.minv_of(pre, shape))
        runs = []
        for poll in POLLS:
            what = (shape, kind, pre, poll)
            got = D.run(b, me.POISON_KMAX, me.POISON_RTOL,
                        dinv=_dinv_of(pre, shape), what=what, poll_every=poll)
            if (shape, kind, pre) in me.WEAK:
                assert len(got.hist) == got.k + 1, what
                assert me.pattern(got) == me.pattern(want), what
            else:
                _same(got, want, what)
            # a solve on NaN ends at kmax with status 0
            assert got.k == (me.POISON_KMAX if at_kmax else 0), what
            assert got.status == status, what
            assert np.all(np.isnan(got.x)) if x_nan else \
                same_bits(got.x, np.zeros(D.N)), what
            runs.append(got)
        assert runs[0].same(runs[1]), (shape, kind, pre)


def test_the_workspace_after_poison_and_after_every_exit(devs, nt):  # noqa: F811
    """one MinresWorkspace: a clean solve, then solves that leave w, r and v
    full of NaN, or that left through status 1, 2 and 3 on longer vectors, and
    after each the clean solve again -- with the bits of the first, and of a
    solve on a fresh workspace"""
    shape = "shift11"
    plain = me.csr_of(shape)
    D = devs((shape, "plain", False), plain)
    b = me.scaled_rhs(plain)
    ws, fresh = host.MinresWorkspace(D.e), host.MinresWorkspace(D.e)
    try:
        for pre in me.PRE_POISON:
            dinv = _dinv_of(pre, shape)
            first = D.run(b, 30, 1e-6, dinv=dinv, ws=ws, what=("first", pre))
            assert 1 < first.k <= 30 and first.status == 0
            assert np.all(np.isfinite(first.x)) and np.all(np.isfinite(first.hist))
            assert first.same(D.run(b, 30, 1e-6, dinv=dinv, ws=fresh))
            for kind in ("a_nan", "b_inf"):
                P, _, pb = _poisoned_dev(devs, shape, kind)
                bad = P.run(pb, me.POISON_KMAX, me.POISON_RTOL, dinv=dinv, ws=ws)
                assert np.all(np.isnan(bad.x)) and bad.k == me.POISON_KMAX
                again = D.run(b, 30, 1e-6, dinv=dinv, ws=ws)
                _same(again, first, ("after", kind, pre))
            for name in ("indef", "neg0", "neg1", "sing3-d"):
                case = BY_NAME[name]
                csr, eb = case.system(True)
                E = devs(("exact", case.block, case.nb, True), csr)
                got = E.run(eb, me.KMAX, 0.0, dinv=case.dinv(True), ws=ws)
                _same(got, case.want(True), ("on the shared workspace", name))
                again = D.run(b, 30, 1e-6, dinv=dinv, ws=ws)
                _same(again, first, ("after", name, pre))
    finally:
        ws.close(), fresh.close()


# ---- 3. scaling and negation -------------------------------------------------------------------
def _relation(base, got, e_x, e_h, sign, what):
    assert (got.k, got.status) == (base.k, base.status), \
        (what, got.k, got.status, base.k, base.status)
    assert len(got.hist) == got.k + 1, what
    assert same_bits(got.hist, np.ldexp(base.hist, e_h)), what
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


def _pre_kwargs(pre, shape, D, s=0):
    if pre in ("none", "jacobi"):
        return {"dinv": _dinv_of(pre, shape, s)}
    return D.precond(pre)


@pytest.mark.parametrize("shape,symmetric",
                         [(shape, sym) for shape in me.SCALED
                          for sym in (False, True)
                          if not sym or shape in me.SYMMETRIC])
def test_scaled_and_negated_systems(devs, shape, symmetric):
    csr = me.csr_of(shape)
    b = me.scaled_rhs(csr)
    K, R = me.SCALED_KMAX, me.SCALED_RTOL
    pres = [p for p in me.SCALED[shape]
            if not symmetric or p in ("none", "jacobi")]
    D = devs((shape, "plain", symmetric), csr, symmetric)
    base = {}
    for pre in pres:
        base[pre] = D.run(b, K, R, what=(shape, symmetric, pre),
                          **_pre_kwargs(pre, shape, D))
        assert 1 < base[pre].k <= K and base[pre].status == 0, (pre, base[pre].k)
        got = D.run(-b, K, R, **_pre_kwargs(pre, shape, D))
        _relation(base[pre], got, 0, 0, -1.0, (shape, symmetric, pre, "-b"))
    scalings = [(s, t, 1.0) for s, t in me.PAIRS] + [(0, 0, -1.0)]
    for s in sorted({s for s, _, sign in scalings if sign > 0}):
        S = Dev(D.e, D.comm, me.scale_csr(csr, s), symmetric)
        try:
            for pre in pres:
                kw = _pre_kwargs(pre, shape, S, s)  # built from the scaled matrix
                for t in [t for s2, t, sign in scalings if s2 == s and sign > 0]:
                    what = (shape, symmetric, pre, s, t)
                    got = S.run(np.ldexp(b, t), K, R, what=what, **kw)
                    _relation(base[pre], got, t - s,
                              me.hist_exponent(pre, s, t), 1.0, what)
        finally:
            S.close()
    # (-A, b): x' = -x with the same history; the dinv stays positive
    S = Dev(D.e, D.comm, me.scale_csr(csr, 0, -1.0), symmetric)
    try:
        for pre in [p for p in pres if p in me.NEGATED_A]:
            got = S.run(b, K, R, **_pre_kwargs(pre, shape, S))
            _relation(base[pre], got, 0, 0, -1.0, (shape, symmetric, pre, "-A"))
    finally:
        S.close()


def test_an_odd_s_with_jacobi_breaks_the_history_relation(devs):
    shape, s = "shift11", me.ODD_S
    csr = me.csr_of(shape)
    b = me.scaled_rhs(csr)
    D = devs((shape, "plain", False), csr)
    S = Dev(D.e, D.comm, me.scale_csr(csr, s))
    try:
        for pre in ("none", "jacobi"):
            base = D.run(b, me.SCALED_KMAX, me.SCALED_RTOL,
                         **_pre_kwargs(pre, shape, D))
            got = S.run(b, me.SCALED_KMAX, me.SCALED_RTOL,
                        **_pre_kwargs(pre, shape, S, s))
            if pre == "none":
                _relation(base, got, -s, 0, 1.0, (shape, s, pre))
                continue
            assert len(got.hist) == got.k + 1
            for e in (-51, -50):
                for i in range(min(base.k, got.k) + 1):
                    assert got.hist[i] != np.ldexp(base.hist[i], e), (e, i)
    finally:
        S.close()


# ---- 4. two ranks --------------------------------------------------------------------------------
def test_two_thread_ranks():
    """perm and sing3 in two slabs cut INSIDE a block, b_nan with the NaN in
    rank 1's slab only, and one scaled pair on shift11 with and without Jacobi:
    every rank returns the same k and status (no rank leaves the loop alone),
    and the gathered x and the history have the bits of the reference, or keep
    the relation between two solves on two ranks."""
    from thread_world import ThreadWorld
    jobs = []  # (key, csr, b, dinv, kmax, rtol, want or None)
    for name in me.TWO_RANKS:
        for case in (BY_NAME[name], BY_NAME[name + "-d"]):
            csr, b = case.system(True)
            cut = int(oracle.owner_ranges(2, len(b))[1])
            assert cut % len(case.block) != 0, (name, cut)
            jobs.append((case.id, csr, b, case.dinv(True), me.KMAX, 0.0,
                         case.want(True)))
    shape = "shift11"
    plain = me.csr_of(shape)
    N = len(plain[0]) - 1
    nan_b = me.rank1_nan(N)
    for pre in me.PRE_POISON:
        want = me.reference(plain, nan_b, me.POISON_KMAX, me.POISON_RTOL,
                            minv=me.minv_of(pre, shape))
        assert want.k == me.POISON_KMAX and np.all(np.isnan(want.x))
        jobs.append((("b_nan", pre), plain, nan_b, _dinv_of(pre, shape),
                     me.POISON_KMAX, me.POISON_RTOL, want))
    s, t = me.PAIRS[0]
    b = me.scaled_rhs(plain)
    for pre in me.PRE_POISON:
        jobs.append((("base", pre), plain, b, _dinv_of(pre, shape),
                     me.SCALED_KMAX, me.SCALED_RTOL, None))
        jobs.append((("scaled", pre), me.scale_csr(plain, s), np.ldexp(b, t),
                     _dinv_of(pre, shape, s), me.SCALED_KMAX, me.SCALED_RTOL,
                     None))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        ws = host.MinresWorkspace(exec_)
        kept = {}
        for key, csr, b, dinv, kmax, rtol, want in jobs:
            n = len(b)
            ranges = oracle.owner_ranges(2, n)
            r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
            M = r1 - r0
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, host.P2P_NONBLOCKING)
            d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
            d_x = exec_.alloc(M + 2 * GUARD)
            exec_.copy_from_host(d_b, b[r0:r1])
            if dinv is not None:
                exec_.copy_from_host(d_dinv, dinv[r0:r1])
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
            k, hist, status = host.minres(
                comm, exec_, A, d_b, d_x + 8 * GUARD, kmax, rtol,
                dinv_ptr=d_dinv if dinv is not None else None, ws=ws)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL), key
            assert np.all(buf[GUARD + M:] == SENTINEL), key
            ks = tw.gather(rank, np.array([k, status]))
            assert np.all(ks.reshape(-1, 2) == [k, status]), (key, ks)
            xs = tw.gather(rank, buf[GUARD:GUARD + M])
            got = Result(xs, k, hist.copy(), status)
            if want is not None:
                _same(got, want, (key, rank))
            kept[key] = got
            A.close()
            for p in (d_b, d_dinv, d_x):
                exec_.free(p)
        for pre in me.PRE_POISON:
            base = kept[("base", pre)]
            assert 1 < base.k <= me.SCALED_KMAX and base.status == 0
            _relation(base, kept[("scaled", pre)], t - s,
                      me.hist_exponent(pre, s, t), 1.0, (pre, s, t, rank))
        ws.close()

    tw.run(rank_body, gpu=True)
