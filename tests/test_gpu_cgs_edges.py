"""Whole solves of host.cg_shifted on the cases of cgs_edges.py: every exit on
exact block matrices a few workgroups long (with the odd tail, ns = 1, 3 and
8, an even and an odd ldx), the floor of scaling, poisoned data and shifts and
the workspace after them, scaled and negated systems, and two ranks.

No comparison here has a tolerance: equality of integers (k, iterations,
status) or cgs_edges.same_bits.  The exact, floor and poisoned cases are held to
cgs_cases.cgs_ref wherever its bits do not depend on the order of a sum
(test_cgs_edges_host.py; the WEAK cases to k, iterations, status and the NaN /
Inf pattern); the scaling relations are between two GPU solves.

X sits between guard words, with gaps between the columns, all filled with a
sentinel before every solve and checked after it."""
import numpy as np
import pytest

import cgs_edges as ce
import oracle
import test_gpu_cgs as tg
from cgs_edges import Result, same_bits
from spmv_amd import host
from test_cgs_edges_host import scaled_hist
from test_gpu_cgs import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tg.SENTINEL, tg.GUARD
POLLS = (1, 16)
BY_NAME = {c.name: c for c in ce.exact_cases()}
NS = 8


def _solve(comm, e, A, M, d_b, d_x, b, shifts, kmax, rtol, ldx, ws, **kw):  # noqa: F811
    """one guarded solve on buffers of M and NS * (M + 3) + 2 * GUARD doubles
    -> (Result with X [ns, M])"""
    ns, n = len(shifts), NS * (M + 3) + 2 * GUARD
    assert M <= ldx <= M + 3 and ns <= NS
    e.copy_from_host(d_b, np.asarray(b, np.float64))
    e.copy_from_host(d_x, np.full(n, SENTINEL))
    k, its, hist, status = host.cg_shifted(comm, e, A, d_b, d_x + 8 * GUARD, ldx,
                                           shifts, kmax, rtol, ws=ws, **kw)
    buf = e.copy_to_host(d_x, n)
    keep = np.zeros(n, bool)
    X = np.empty((ns, M))
    for s in range(ns):
        X[s] = buf[GUARD + s * ldx:GUARD + s * ldx + M]
        keep[GUARD + s * ldx:GUARD + s * ldx + M] = True
    assert np.all(buf[~keep] == SENTINEL), "a word outside the columns moved"
    assert not np.any(X == SENTINEL), "x not written"
    return Result(X, k, list(its), hist.copy(), status)


class Dev:
    def __init__(self, exec_, comm, csr, symmetric=False):  # noqa: F811
        self.e, self.comm = exec_, comm
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [],
                                           symmetric, host.P2P_NONBLOCKING)
        self.d_b = exec_.alloc(N)
        self.d_x = exec_.alloc(NS * (N + 3) + 2 * GUARD)
        self.ws = host.CgShiftedWorkspace(exec_)

    def run(self, b, shifts, kmax, rtol, ldx=None, ws=None, **kw):
        return _solve(self.comm, self.e, self.A, self.N, self.d_b, self.d_x, b,
                      shifts, kmax, rtol, ldx or self.N, ws or self.ws, **kw)

    def close(self):
        self.ws.close()
        self.A.close()
        self.e.free(self.d_b), self.e.free(self.d_x)


@pytest.fixture(scope="module")
def devs(exec_, comm):  # noqa: F811
    made = {}

    def get(key, csr, symmetric=False):
        if key not in made:
            made[key] = Dev(exec_, comm, csr, symmetric)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _same(got, want, what):
    assert (got.k, got.its, got.status) == (want.k, want.its, want.status), \
        (what, got.k, got.its, got.status, want.k, want.its, want.status)
    assert same_bits(got.hist, want.hist), (what, got.hist[:, :3])
    assert same_bits(got.x, want.x), what


def _all_ways(D, want, what, b, shifts, kmax, rtol, weak=False):
    """poll_every 1 and 16, ldx = N, N + 1 and N + 2 (an odd ldx takes the
    workspace's copy path): against `want` and against each other"""
    runs = []
    for poll in POLLS:
        for ldx in (D.N, D.N + 1, D.N + 2):
            got = D.run(b, shifts, kmax, rtol, ldx=ldx, poll_every=poll)
            if weak:
                assert ce.pattern(got) == ce.pattern(want), (what, poll, ldx)
            else:
                _same(got, want, (what, poll, ldx))
            runs.append(got)
    for r in runs[1:]:
        assert runs[0].same(r), what
    return runs[0]


@pytest.mark.parametrize("case", ce.exact_cases(), ids=lambda c: c.id)
def test_exact_cases(devs, nt, case):  # noqa: F811
    for tail in (False, True):
        csr, b = case.system(tail)
        D = devs(("exact", case.block, case.nb, tail), csr)
        for kmax in case.kmaxes():
            want = ce.reference(csr, b, case.shifts, kmax, case.rtol)
            assert want.same(case.want(tail, kmax)), case.id  # the table
            got = _all_ways(D, want, (case.id, tail, kmax), b, case.shifts,
                            kmax, case.rtol)
        if case.solved:
            for s, sigma in enumerate(case.shifts):
                if case.its[s] == case.k:
                    assert same_bits(ce.shifted_spmv(csr, sigma, got.x[s]), b)


@pytest.mark.parametrize("s", ce.FLOOR_S)
@pytest.mark.parametrize("name", ce.FLOOR_CASES)
def test_floor_cases(exec_, comm, nt, name, s):  # noqa: F811
    for tail in (False, True):
        csr, b, shifts, want = ce.floor_case(BY_NAME[name], s, tail)
        assert ce.reference(csr, b, shifts, ce.KMAX, 0.0).same(want)
        D = Dev(exec_, comm, csr)
        try:
            _all_ways(D, want, (name, s, tail), b, shifts, ce.KMAX, 0.0)
        finally:
            D.close()


def _poisoned_dev(devs, sym, kind):
    csr, b, shifts = ce.poisoned_case(kind)
    key = ("poisson11", "a_nan" if kind == "a_nan" else "plain", sym)
    return devs(key, csr, sym), b, shifts


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("sym", ce.STORAGES, ids=["general", "symmetric"])
def test_poisoned_cases(devs, nt, sym, kind):  # noqa: F811
    D, b, shifts = _poisoned_dev(devs, sym, kind)
    k, status, _, x_nan = ce.POISON_OUTCOME[kind]
    want = ce.poisoned_reference(sym, kind)
    got = _all_ways(D, want, (sym, kind), b, shifts, ce.POISON_KMAX,
                    ce.POISON_RTOL, weak=(sym, kind) in ce.WEAK)
    assert (got.k, got.status) == (k, status)
    if x_nan is None:  # the huge shift froze and did not disturb the other
        assert got.its == [ce.POISON_KMAX, 1]
        assert same_bits(got.x[1], want.x[1])  # elementwise from b: exact
        alone = D.run(b, (0.0,), ce.POISON_KMAX, ce.POISON_RTOL)
        assert same_bits(got.x[0], alone.x[0])
        assert same_bits(got.hist[0], alone.hist[0])
    else:
        assert np.all(np.isnan(got.x)) if x_nan else \
            same_bits(got.x, np.zeros(got.x.shape))


def test_the_workspace_after_poison_and_after_every_exit(devs, nt):  # noqa: F811
    csr = ce.csr_of()
    b = ce.scaled_rhs(csr)
    for sym in ce.STORAGES:
        D = devs(("poisson11", "plain", sym), csr, sym)
        ws, fresh = (host.CgShiftedWorkspace(D.e) for _ in range(2))
        args = (b, ce.POISON_SHIFTS, 30, 1e-6)
        try:
            first = D.run(*args, ws=ws)
            assert 1 < first.k <= 30 and first.status == 0
            assert np.all(np.isfinite(first.x))
            assert first.same(D.run(*args, ws=fresh))
            for kind in ce.KINDS:
                P, pb, shifts = _poisoned_dev(devs, sym, kind)
                bad = P.run(pb, shifts, ce.POISON_KMAX, ce.POISON_RTOL, ws=ws)
                assert bad.k == ce.POISON_OUTCOME[kind][0], kind
                _same(D.run(*args, ws=ws), first, ("after", kind, sym))
            for case in ce.exact_cases():
                ecsr, eb = case.system(True)
                E = devs(("exact", case.block, case.nb, True), ecsr)
                got = E.run(eb, case.shifts, ce.KMAX, case.rtol, ws=ws)
                _same(got, case.want(True), ("shared workspace", case.id))
                _same(D.run(*args, ws=ws), first, ("after", case.id, sym))
        finally:
            ws.close(), fresh.close()


def _relation(base, got, s, t, sign, what):
    assert (got.k, got.its, got.status) == (base.k, base.its, base.status), what
    assert same_bits(got.hist, scaled_hist(base.hist, t)), what
    assert same_bits(got.x, sign * np.ldexp(base.x, t - s)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


@pytest.mark.parametrize("sym", ce.STORAGES, ids=["general", "symmetric"])
def test_scaled_and_negated_systems(devs, nt, sym):  # noqa: F811
    csr = ce.csr_of()
    b = ce.scaled_rhs(csr)
    K, R, sh = ce.SCALED_KMAX, ce.SCALED_RTOL, ce.POISON_SHIFTS
    D = devs(("poisson11", "plain", sym), csr, sym)
    base = D.run(b, sh, K, R)
    assert 1 < base.k <= K and base.status == 0
    _relation(base, D.run(-b, sh, K, R), 0, 0, -1.0, (sym, "-b"))
    for s in sorted({s for s, _ in ce.PAIRS}):
        S = Dev(D.e, D.comm, ce.scale_csr(csr, s), sym)
        try:
            for t in [t for s2, t in ce.PAIRS if s2 == s]:
                got = S.run(np.ldexp(b, t), tuple(np.ldexp(sh, s)), K, R)
                _relation(base, got, s, t, 1.0, (sym, s, t))
        finally:
            S.close()
    S = Dev(D.e, D.comm, ce.scale_csr(csr, 0, -1.0), sym)
    try:  # (-A, b): status 1 at k = 0, X = 0
        got = S.run(b, sh, K, R)
        assert (got.k, got.its, got.status) == (0, [0] * 3, 1)
        assert same_bits(got.x, np.zeros(got.x.shape))
    finally:
        S.close()


def test_two_thread_ranks():
    """curv2 and early in two slabs cut INSIDE a block, b_nan with the NaN in
    rank 1's slab only, and one scaled pair on poisson11: every rank returns
    the same k, iterations and status, and the gathered X and the histories
    have the reference's bits or keep the relation."""
    from thread_world import ThreadWorld
    jobs = []  # (key, csr, b, shifts, kmax, rtol, want or None)
    for name in ce.TWO_RANKS:
        case = BY_NAME[name]
        csr, b = case.system(True)
        cut = int(oracle.owner_ranges(2, len(b))[1])
        assert cut % len(case.block) != 0, (name, cut)
        jobs.append((name, csr, b, case.shifts, ce.KMAX, case.rtol,
                     case.want(True)))
    plain = ce.csr_of()
    N = len(plain[0]) - 1
    nan_b = ce.rank1_nan(N)
    want = ce.reference(plain, nan_b, ce.POISON_SHIFTS, ce.POISON_KMAX,
                        ce.POISON_RTOL)
    assert (want.k, want.status) == (0, 1)
    jobs.append(("b_nan", plain, nan_b, ce.POISON_SHIFTS, ce.POISON_KMAX,
                 ce.POISON_RTOL, want))
    s, t = ce.PAIRS[0]
    b = ce.scaled_rhs(plain)
    K, R, sh = ce.SCALED_KMAX, ce.SCALED_RTOL, ce.POISON_SHIFTS
    jobs.append(("base", plain, b, sh, K, R, None))
    jobs.append(("scaled", ce.scale_csr(plain, s), np.ldexp(b, t),
                 tuple(np.ldexp(sh, s)), K, R, None))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        ws = host.CgShiftedWorkspace(exec_)
        kept = {}
        for key, csr, b, shifts, kmax, rtol, want in jobs:
            ranges = oracle.owner_ranges(2, len(b))
            r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
            M = r1 - r0
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, host.P2P_NONBLOCKING)
            d_b = exec_.alloc(M)
            d_x = exec_.alloc(NS * (M + 3) + 2 * GUARD)
            loc = _solve(comm, exec_, A, M, d_b, d_x, b[r0:r1], shifts, kmax,
                         rtol, M + 3, ws)
            mine = np.array(loc.its + [loc.k, loc.status])
            ks = tw.gather(rank, mine)
            assert np.all(ks.reshape(2, -1) == mine), (key, ks)
            X = np.stack([tw.gather(rank, loc.x[i]) for i in range(len(shifts))])
            got = Result(X, loc.k, loc.its, loc.hist, loc.status)
            if want is not None:
                _same(got, want, (key, rank))
            kept[key] = got
            A.close()
            exec_.free(d_b), exec_.free(d_x)
        assert 1 < kept["base"].k <= K and kept["base"].status == 0
        _relation(kept["base"], kept["scaled"], s, t, 1.0, (s, t, rank))
        ws.close()

    tw.run(rank_body, gpu=True)
