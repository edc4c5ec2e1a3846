"""Whole solves of host.idrs on the cases of idrs_edges.py: every exit on exact
block matrices a few workgroups long at s = 1, 2, 4, 8 (with the odd tail),
the floor of scaling with and without dinv, poisoned b, A and dinv and the
workspace after them, systems scaled by powers of two or negated under every
preconditioner, and two ranks.

No comparison here has a tolerance: equality of integers (k, status, len(hist)
== k + 1) or idrs_edges.same_bits.  The exact, floor and poisoned cases are held
to idrs_cases.idrs_ref wherever its bits do not depend on the order of a sum
(test_idrs_edges_host.py; the WEAK cases to k, status and the NaN / Inf
pattern); the scaling relations are between two GPU solves.

X sits between guard words and is filled with a sentinel before every solve."""
import numpy as np
import pytest

import idrs_cases as ic
import idrs_edges as ie
import oracle
import test_gpu_idrs as ti
from idrs_edges import Result, same_bits
from spmv_amd import host
from test_gpu_idrs import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = ti.SENTINEL, ti.GUARD
POLLS = (1, 16)


class Dev:
    def __init__(self, exec_, comm, csr):  # noqa: F811
        self.e, self.comm = exec_, comm
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [],
                                           False, host.P2P_NONBLOCKING)
        self.d_b, self.d_dinv = exec_.alloc(N), exec_.alloc(N)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.IdrsWorkspace(exec_)
        self.pre = {}

    def precond(self, kind):
        if kind not in self.pre:
            cls = {"sgs": host.SgsPreconditioner, "ilu0": host.Ilu0Preconditioner,
                   "amg": host.AmgPreconditioner}
            self.pre[kind] = cls[kind](self.e, self.A)
        return {"amg" if kind == "amg" else "sgs": self.pre[kind]}

    def run(self, b, s, kmax, rtol, dinv=None, ws=None, what=None, **kw):
        e, N = self.e, self.N
        e.copy_from_host(self.d_b, np.asarray(b, np.float64))
        if dinv is not None:
            e.copy_from_host(self.d_dinv, np.asarray(dinv, np.float64))
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist, status = host.idrs(
            self.comm, e, self.A, self.d_b, self.d_x + 8 * GUARD, s, kmax, rtol,
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
    assert len(got.hist) == got.k + 1, (what, len(got.hist))
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what


def _both_polls(D, want, what, *args, weak=False, **kw):
    runs = []
    for poll in POLLS:
        got = D.run(*args, what=(what, poll), poll_every=poll, **kw)
        if weak:
            assert len(got.hist) == got.k + 1, what
            assert ie.pattern(got) == ie.pattern(want), (what, poll)
        else:
            _same(got, want, (what, poll))
        runs.append(got)
    assert runs[0].same(runs[1]), what
    return runs[0]


# ---- 1. exact cases and the floor ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ie.SHAPES))
def test_exact_cases(devs, nt, name):  # noqa: F811
    for tail in (False, True):
        csr, b = ie.system(name, tail)
        D = devs(("exact", name, tail), csr)
        for key in sorted(k for k in ie.TABLE if k[0] == name):
            _, s, kmax = key
            want = ie.reference(csr, b, s, kmax, 0.0)
            assert want.same(ie.want(key, tail)), key  # the table
            got = _both_polls(D, want, (key, tail), b, s, kmax, 0.0)
            if key in ie.SOLVED:
                assert same_bits(oracle.csr_spmv(*csr, got.x), b), key


@pytest.mark.parametrize("scale", ie.FLOOR_S)
@pytest.mark.parametrize("name,s", ie.FLOOR_CASES)
def test_floor_cases(exec_, comm, nt, name, s, scale):  # noqa: F811
    for tail in (False, True):
        D = None
        try:
            for pre in ie.PRES:
                csr, b, dinv, want = ie.floor_case(name, s, scale, pre, tail)
                ref = ie.reference(csr, b, s, ie.KMAX, 0.0, dinv=dinv)
                assert ref.same(want), (name, s, scale, pre)  # the table
                D = D or Dev(exec_, comm, csr)
                _both_polls(D, want, (name, s, scale, pre, tail), b, s, ie.KMAX,
                            0.0, dinv=dinv)
        finally:
            if D:
                D.close()


# ---- 2. poisoned data ----------------------------------------------------------------------
def _poisoned_dev(devs, shape, kind, pre):
    csr, b, dinv = ie.poisoned_case(shape, kind, pre)
    return devs((shape, "a_nan" if kind == "a_nan" else "plain"), csr), b, dinv


@pytest.mark.parametrize("kind", ie.KINDS)
@pytest.mark.parametrize("shape", ie.POISON_SHAPES)
def test_poisoned_cases(devs, nt, shape, kind):  # noqa: F811
    k, status, _, x_zero = ie.POISON_OUTCOME[kind]
    for _, _, s, pre in [c for c in ie.poison_combos() if c[:2] == (shape, kind)]:
        combo = (shape, kind, s, pre)
        D, b, dinv = _poisoned_dev(devs, shape, kind, pre)
        want = ie.poisoned_reference(*combo)
        got = _both_polls(D, want, combo, b, s, ie.POISON_KMAX, ie.POISON_RTOL,
                          dinv=dinv, weak=combo in ie.WEAK)
        assert (got.k, got.status) == (s if k is None else k, status), combo
        if x_zero:
            assert same_bits(got.x, np.zeros(D.N)), combo
        else:
            assert np.all(np.isfinite(got.x)) and got.x.any(), combo


def test_the_workspace_after_poison_and_after_every_exit(devs, nt):  # noqa: F811
    """one IdrsWorkspace: a clean solve, each poisoned solve and each exact
    exit, and after each the clean solve again -- with the bits of the first,
    and of a solve on a fresh workspace"""
    shape = "convdiff8"
    D = devs((shape, "plain"), ie.csr_of(shape))
    b = ie.scaled_rhs(shape)
    ws, fresh = host.IdrsWorkspace(D.e), host.IdrsWorkspace(D.e)
    try:
        for pre in ie.PRES:
            dinv = ie.dinv_of(shape) if pre == "dinv" else None
            args = (b, 4, 30, 1e-6)
            first = D.run(*args, dinv=dinv, ws=ws)
            assert 1 < first.k <= 30 and first.status == 0
            assert np.all(np.isfinite(first.x))
            assert first.same(D.run(*args, dinv=dinv, ws=fresh))
            for kind in ie.KINDS:
                if pre == "none" and kind in ie.DINV_POISONS:
                    continue
                P, pb, pd = _poisoned_dev(devs, shape, kind, pre)
                bad = P.run(pb, 4, ie.POISON_KMAX, ie.POISON_RTOL, dinv=pd, ws=ws)
                assert bad.status == ie.POISON_OUTCOME[kind][1], kind
                _same(D.run(*args, dinv=dinv, ws=ws), first, ("after", kind))
            for key in sorted(k for k in ie.TABLE if k[2] == ie.KMAX):
                csr, eb = ie.system(key[0], True)
                E = devs(("exact", key[0], True), csr)
                got = E.run(eb, key[1], ie.KMAX, 0.0, ws=ws)
                _same(got, ie.want(key, True), ("on the shared workspace", key))
                _same(D.run(*args, dinv=dinv, ws=ws), first, ("after", key))
    finally:
        ws.close(), fresh.close()


# ---- 3. scaling and negation -------------------------------------------------------------------
def _relation(base, got, sc, t, sign, what):
    assert (got.k, got.status) == (base.k, base.status), \
        (what, got.k, got.status, base.k, base.status)
    assert len(got.hist) == got.k + 1, what
    assert same_bits(got.hist, np.ldexp(base.hist, t)), what
    assert same_bits(got.x, sign * np.ldexp(base.x, t - sc)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


def _pre_kwargs(pre, shape, D, sc=0):
    if pre == "none":
        return {}
    if pre == "dinv":
        return {"dinv": ie.dinv_of(shape, sc)}
    if pre == "cheb":
        return {"dinv": ie.dinv_of(shape, sc), "cheb": ic.CHEB}
    return D.precond(pre)  # built from the (scaled) matrix of D


@pytest.mark.parametrize("shape", sorted(ie.SCALED))
def test_scaled_and_negated_systems(devs, nt, shape):  # noqa: F811
    csr = ie.csr_of(shape)
    b = ie.scaled_rhs(shape)
    K, R, pres = ie.SCALED_KMAX, ie.SCALED_RTOL, ie.SCALED[shape]
    D = devs((shape, "plain"), csr)
    base = {}
    for pre in pres:
        for s in ie.SCALED_S:
            base[pre, s] = D.run(b, s, K, R, **_pre_kwargs(pre, shape, D))
            assert 1 < base[pre, s].k <= K and base[pre, s].status == 0
            got = D.run(-b, s, K, R, **_pre_kwargs(pre, shape, D))
            _relation(base[pre, s], got, 0, 0, -1.0, (shape, pre, s, "-b"))
    every = ie.PAIRS + (ie.ODD_PAIR,)
    for sc in sorted({sc for sc, _ in every}):
        S = Dev(D.e, D.comm, ie.scale_csr(csr, sc))
        try:
            for pre in pres:
                kw = _pre_kwargs(pre, shape, S, sc)
                ok = ie.pairs(pre) + (ie.ODD_PAIR,)
                for t in [t for sc2, t in ok if sc2 == sc]:
                    for s in ie.SCALED_S:
                        what = (shape, pre, s, sc, t)
                        got = S.run(np.ldexp(b, t), s, K, R, what=what, **kw)
                        _relation(base[pre, s], got, sc, t, 1.0, what)
        finally:
            S.close()
    S = Dev(D.e, D.comm, ie.scale_csr(csr, 0, -1.0))
    try:  # (-A, b): -x, the same history; dinv stays that of +A
        for pre in [p for p in pres if p in ie.NEGATED_A]:
            for s in ie.SCALED_S:
                got = S.run(b, s, K, R, **_pre_kwargs(pre, shape, S))
                _relation(base[pre, s], got, 0, 0, -1.0, (shape, pre, s, "-A"))
    finally:
        S.close()


# ---- 4. two ranks --------------------------------------------------------------------------------
def test_two_thread_ranks():
    """two_i (s = 2) and perm (s = 1) in two slabs cut INSIDE a block, b_nan
    with the NaN in rank 1's slab only, and one scaled pair on convdiff8 with
    and without dinv: every rank returns the same k and status, and the
    gathered x and the history have the reference's bits or keep the relation"""
    from thread_world import ThreadWorld
    jobs = []  # (key, csr, b, s, dinv, kmax, rtol, want or None)
    for name, s in ie.TWO_RANKS:
        csr, b = ie.system(name, True)
        cut = int(oracle.owner_ranges(2, len(b))[1])
        assert cut % 2 != 0, (name, cut)
        jobs.append(((name, s), csr, b, s, None, ie.KMAX, 0.0,
                     ie.want((name, s, ie.KMAX), True)))
    shape = "convdiff8"
    plain = ie.csr_of(shape)
    N = len(plain[0]) - 1
    nan_b = ie.rank1_nan(N)
    K, R = ie.SCALED_KMAX, ie.SCALED_RTOL
    sc, t = ie.PAIRS[0]
    b = ie.scaled_rhs(shape)
    for pre in ie.PRES:
        d = ie.dinv_of(shape) if pre == "dinv" else None
        want = ie.reference(plain, nan_b, 4, ie.POISON_KMAX, ie.POISON_RTOL,
                            dinv=d)
        assert (want.k, want.status) == (0, 1)
        jobs.append((("b_nan", pre), plain, nan_b, 4, d, ie.POISON_KMAX,
                     ie.POISON_RTOL, want))
        jobs.append((("base", pre), plain, b, 4, d, K, R, None))
        jobs.append((("scaled", pre), ie.scale_csr(plain, sc), np.ldexp(b, t), 4,
                     None if d is None else np.ldexp(d, -sc), K, R, None))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        ws = host.IdrsWorkspace(exec_)
        kept = {}
        for key, csr, b, s, dinv, kmax, rtol, want in jobs:
            ranges = oracle.owner_ranges(2, len(b))
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
            k, hist, status = host.idrs(
                comm, exec_, A, d_b, d_x + 8 * GUARD, s, kmax, rtol,
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
        for pre in ie.PRES:
            base = kept["base", pre]
            assert 1 < base.k <= K and base.status == 0
            _relation(base, kept["scaled", pre], sc, t, 1.0, (pre, sc, t, rank))
        ws.close()

    tw.run(rank_body, gpu=True)
