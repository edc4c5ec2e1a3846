"""The cases of gmres_edges.py do what they claim, on gmres_cases.gmres_ref
alone (no GPU): the table of the exact cases under three summation orders, the
outcomes of the poisoned cases, the scaling and negation relations with every
operand recorded, ILU(0) and SGS under scaling, and that no case reaches a
division by an exact zero in the reference's Python floats."""
import math

import numpy as np
import pytest

import gmres_cases as gc
import gmres_edges as ge
import ilu0_cases as ic
import oracle
from gmres_edges import same_bits
from test_solver_edges_host import _healthy, _records_healthy

EXACT = ge.exact_cases()


def _minvs(N):
    return (None, ge.jacobi(np.full(N, ge.EXACT_DINV)))


# ---- a. exact cases ---------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_exact_cases_give_the_table(case):
    """(k, status, history, x) of the table, for both N, with and without dinv =
    0.5, under three summation orders; a zero divisor would raise"""
    bb = ge.DOT(np.array(case.rhs, float), np.array(case.rhs, float)) * case.nb
    assert bb == 1024.0 and case.hist[0] == 32.0  # a power of four: beta = 32
    for tail in (False, True):
        csr, b = case.system(tail)
        N = len(b)
        assert N <= 4097 and N % 2 == int(tail)
        want = case.want(tail)
        assert len(want.hist) == want.k + 1
        for minv in _minvs(N):
            for dot in ge.ORDERS:
                got = ge.reference(csr, b, case.restart, ge.KMAX, 0.0, minv=minv,
                                   dot=dot)
                what = (case.id, tail, minv is not None, dot.__name__)
                assert (got.k, got.status) == (want.k, want.status), what
                assert same_bits(got.hist, want.hist), (what, got.hist)
                assert same_bits(got.x, want.x), what  # +0.0 where the table says 0
        r = b - oracle.csr_spmv(*csr, want.x)
        if case.status == 1:
            assert same_bits(oracle.csr_spmv(*csr, want.x), b), case.id
        else:  # status 2 and stagnation: the true residual is never 0
            assert ge.DOT(r, r) == 1024.0 and np.all(want.x == 0.0), case.id


def test_exact_cases_reach_the_exits_they_are_for():
    by = {c.id: c for c in EXACT}
    assert len(by) == len(EXACT) == 11
    # a stop on the last step of a cycle: step j = restart - 1 is the one that
    # stops (status 1: it is counted in k; status 2: it is discarded)
    for cid, last in (("perm-m2", True), ("cyc3-m3", True), ("shift3-m3", True),
                      ("perm-m30", False), ("cyc3-m30", False),
                      ("shift3-m30", False), ("nil-m30", False)):
        c = by[cid]
        j_stop = c.k - 1 if c.status == 1 else c.k
        assert c.status in (1, 2) and (j_stop == c.restart - 1) == last, cid
    # status 2 with no column kept, and with two
    assert (by["nil-m30"].status, by["nil-m30"].k) == (2, 0)
    assert (by["shift3-m30"].status, by["shift3-m30"].k) == (2, 2)
    # status 1 beyond j = 0 of the first cycle
    assert by["perm-m30"].k == 2 and by["cyc3-m30"].k == 3
    # stagnation: whole cycles of jn = restart columns up to kmax
    for cid in ("perm-m1", "shift3-m2", "cyc3-m2"):
        c = by[cid]
        assert (c.k, c.status) == (ge.KMAX, 0) and ge.KMAX % c.restart == 0
        assert np.all(c.hist == 32.0) and np.all(c.xblock == 0.0)


def test_the_two_rank_cut_is_inside_a_block():
    by = {c.id: c for c in EXACT}
    for name in ge.TWO_RANKS:
        c = by[f"{name}-m30"]
        N = len(c.system(True)[1])
        cut = int(oracle.owner_ranges(2, N)[1])
        assert 0 < cut < N - 1 and cut % len(c.block) != 0, (name, cut)


def test_a_zero_divisor_raises_in_the_reference():
    """what `no case reaches such a division` rests on: Python floats raise.
    The one divisor no comparison guards is a == 0 under a NaN b."""
    with pytest.raises(ZeroDivisionError):
        gc.rotation(0.0, float("nan"))
    assert gc.rotation(float("nan"), 0.0) == (1.0, 0.0)
    c, s = gc.rotation(float("nan"), 1.0)  # |b| > |a| is false on a NaN
    assert math.isnan(c) and math.isnan(s)


@pytest.mark.parametrize("tail", [False, True])
def test_under_case_stops_on_rr_in_the_second_cycle(tail):
    csr, b, m, kmax = ge.under_case(tail)
    runs = [ge.reference(csr, b, m, kmax, 0.0, dot=dot) for dot in ge.ORDERS]
    got = runs[0]
    assert got.same(runs[1]) and got.same(runs[2])
    assert (got.k, got.status) == (1, 0) and m == 1 and kmax > 1
    assert len(got.hist) == 2 and got.hist[1] > np.finfo(float).tiny
    assert got.hist[0] ** 2 > np.finfo(float).tiny  # b.b is a normal number
    r = b - oracle.csr_spmv(*csr, got.x)
    assert np.any(r != 0.0) and np.all(r * r == 0.0) and ge.DOT(r, r) == 0.0
    # every row and every dot product has at most two nonzero terms
    assert np.diff(csr[0]).max() == 2 and np.count_nonzero(b) == 2


# ---- b. poisoned data ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ge.POISONS)
@pytest.mark.parametrize("shape", ge.SHAPES)
def test_poisoned_outcomes(shape, kind):
    plain = ge.csr_of(shape)
    csr, b = ge.poisoned(plain, kind)
    at_kmax, status, h0, x_nan = ge.POISON_OUTCOME[kind]
    for pre in ge.PRE_POISON:
        minv = ge.minv_of(pre, plain)
        for m in ge.RESTARTS:
            got = ge.reference(csr, b, m, ge.POISON_KMAX, ge.POISON_RTOL,
                               minv=minv)
            what = (shape, kind, pre, m)
            assert got.k == (ge.POISON_KMAX if at_kmax else 0), what
            assert got.status == status and len(got.hist) == got.k + 1, what
            assert np.all(np.isnan(got.hist[1:])), what
            if h0 == "nan":
                assert np.isnan(got.hist[0]), what
            elif h0 == "exact":  # integers: the same in any order
                bb = ge.DOT(b, b)
                assert bb == ge.dot_chunked(b, b) == ge.dot_reversed(b, b)
                assert same_bits(got.hist[:1], np.array([math.sqrt(bb)])), what
            else:
                assert same_bits(got.hist[:1],
                                 np.array([np.inf if h0 == "inf" else h0])), what
            if x_nan:
                assert np.all(np.isnan(got.x)), what
            else:
                assert same_bits(got.x, np.zeros(len(b))), what


def test_mutant_stop_test_that_stops_on_nan(monkeypatch):
    """`res / hist[0] >= rtol -> go on` in place of `< rtol -> stop`: the
    poisoned cases that run to kmax tell the two apart"""
    true_givens = gc.gmres_givens

    def mutant(j, h, ww, cs, sn, g, hist0, k, kmax, rtol):
        st = true_givens(j, h, ww, cs, sn, g, hist0, k, kmax, rtol)
        if not st["done"] and not st["res"] / hist0 >= rtol:
            st.update(done=True, inv=None)
        return st

    plain = ge.csr_of("convdiff11")
    for kind in ("b_nan", "b_inf", "a_nan"):
        csr, b = ge.poisoned(plain, kind)
        true = ge.reference(csr, b, 5, ge.POISON_KMAX, ge.POISON_RTOL)
        with monkeypatch.context() as mp:
            mp.setattr(gc, "gmres_givens", mutant)
            got = ge.reference(csr, b, 5, ge.POISON_KMAX, ge.POISON_RTOL)
        assert true.k == ge.POISON_KMAX and got.k == 1, (kind, got.k)


# ---- c. scaled and negated systems ----------------------------------------------------------
def _relation(base, got, e_x, e_h, sign=1.0):
    assert (got.k, got.status) == (base.k, base.status)
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x))
    assert same_bits(got.hist, np.ldexp(base.hist, e_h))
    _healthy(base.x, got.x), _healthy(base.hist, got.hist)


@pytest.mark.parametrize("m", ge.RESTARTS)
@pytest.mark.parametrize("pre", ge.PRECONDITIONERS)
@pytest.mark.parametrize("shape", ge.SHAPES)
def test_scaling_relations_hold_on_the_reference(shape, pre, m):
    csr = ge.csr_of(shape)
    b = ge.scaled_rhs(csr)

    def run(s, t, sign_a=1.0, sign_b=1.0):
        rec = []
        got = ge.reference(ge.scale_csr(csr, s, sign_a), sign_b * np.ldexp(b, t),
                           m, ge.SCALED_KMAX, ge.SCALED_RTOL,
                           minv=ge.minv_of(pre, csr, s, sign_a), record=rec)
        return got, rec

    base, rec0 = run(0, 0)
    assert 1 < base.k < ge.SCALED_KMAX and base.status == 0, base.k
    assert base.hist[-1] / base.hist[0] < ge.SCALED_RTOL
    for s, t in ge.SCALES:
        got, rec = run(s, t)
        _relation(base, got, t - s, t)
        _records_healthy(rec0, rec)
    got, rec = run(0, 0, sign_b=-1.0)
    _relation(base, got, 0, 0, -1.0)
    _records_healthy(rec0, rec)
    if pre in ge.NEGATED_A:
        got, rec = run(0, 0, sign_a=-1.0)
        _relation(base, got, 0, 0, -1.0)
        _records_healthy(rec0, rec)


@pytest.mark.parametrize("shape", ge.ILU_SHAPES)
def test_ilu0_and_sgs_under_scaling_on_the_restatement(shape):
    csr = gc.csr_by_name(shape)
    N = len(csr[0]) - 1
    colours = ic.greedy_colours(csr, N)
    ref = ic.Ilu0Ref(csr, N, colours, False)
    l, u, d = ref.factor()
    mult = ge.ilu0_multipliers(ref.parts[0]["cpos"], l, d)
    r = np.random.default_rng(N).uniform(-1, 1, N)
    z_ilu, z_sgs = ref.apply((l, u, d), r), gc.SgsRef(csr)(r)
    for s in ge.ILU_SCALES:
        A = ge.scale_csr(csr, s)
        ref_s = ic.Ilu0Ref(A, N, colours, False)
        ls, us, ds = ref_s.factor()
        assert same_bits(ds, np.ldexp(d, s)), (shape, s, "pivots")
        assert same_bits(ls, np.ldexp(l, s)) and same_bits(us, np.ldexp(u, s))
        assert same_bits(ge.ilu0_multipliers(ref_s.parts[0]["cpos"], ls, ds),
                         mult), (shape, s, "multipliers")
        assert same_bits(ref_s.apply((ls, us, ds), r), np.ldexp(z_ilu, -s))
        assert same_bits(gc.SgsRef(A)(r), np.ldexp(z_sgs, -s)), (shape, s)
        for v in (l, u, d, ls, us, ds, mult, z_ilu, z_sgs):
            _healthy(v, v)
