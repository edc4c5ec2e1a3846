"""The cases of solver_edges.py do what they claim, on the references alone, and
they reject mutants of the references (no GPU)."""
import math

import numpy as np
import pytest

import solver_edges as se
import test_gpu_pcg as tp
from solver_edges import same_bits

EXACT = se.exact_cases()
SHAPES = tp.SHAPES


# ---- a. the search and the exact cases -------------------------------------------
def test_the_search_finds_the_named_blocks():
    f2 = se.search_blocks(2, se.simulate_bicgstab, {(1, "tt0"), (1, "ts0")})
    assert f2[(1, "tt0")] == se.TT0 and f2[(1, "ts0")] == se.TS0
    f3 = se.search_blocks(3, se.simulate_bicgstab,
                          {(1, "rho0"), (2, "ts0"), (2, "bd1")})
    assert f3[(1, "rho0")] == se.RHO0 and f3[(2, "ts0")] == se.TS0_2
    assert f3[(2, "bd1")] == se.BD1_2
    assert se.search_blocks(2, se.simulate_cg, {(1, "curv")}) == \
        {(1, "curv"): se.CURV1}
    # no 2 x 2 block has zero curvature at k = 2 under cg()'s square roots
    assert se.search_blocks(2, se.simulate_cg, {(2, "curv")}) == {}
    assert se.search_blocks(3, se.simulate_cg, {(2, "curv")}) == \
        {(2, "curv"): se.CURV2}
    assert se.simulate_bicgstab(*se.TWO_I) == (1, "tt0")


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_exact_cases_hit_their_branch(case):
    assert 1000 <= case.N <= 5000 and case.N % 2 == 1
    sim = se.simulate_bicgstab if case.solvers == se.BI else se.simulate_cg
    k_event = case.at
    assert sim(case.block, case.rhs) == (k_event, case.event)
    for solver in case.solvers:
        if solver == "cg_block":
            # the block of the GPU test: the case, a zero column, the case
            B = se.exact_block(case, 3)
            its, hist, X = se.reference_block(case.csr, B, se.KMAX, case.rtol)
            one = se.reference("cg", case.csr, case.b, se.KMAX, case.rtol)
            assert list(its) == [case.k, 0, case.k]
            for c in (0, 2):
                assert same_bits(hist[c], one.hist) and same_bits(X[:, c], one.x)
            assert np.all(X[:, 1] == 0.0) and hist[1, 0] == 0.0
            assert np.all(hist[1, 1:] == -1.0)
            continue
        kw = se.solver_kwargs(solver, case.csr, exact=True)
        ref = se.reference(solver, case.csr, case.b, se.KMAX, case.rtol, **kw)
        assert (ref.k, ref.status) == (case.k, case.status), (solver, ref.k)
        assert len(ref.hist) == ref.k + 1
        if solver != "cg":  # exact: the bits do not depend on the order of sums
            for dot in (se.dot_chunked, se.dot_reversed):
                assert ref.same(se.reference(solver, case.csr, case.b, se.KMAX,
                                             case.rtol, dot=dot, **kw)), solver
        if case.event == "curv":
            # finite up to the event, then Inf for one entry at the most, then
            # NaN to the end; x entirely NaN
            assert np.all(np.isfinite(ref.hist[:k_event]))
            assert np.all(np.isnan(ref.hist[k_event + 1:]))
            assert np.all(np.isnan(ref.x))
        else:
            assert np.all(np.isfinite(ref.x)) and np.all(np.isfinite(ref.hist))
            assert np.any(ref.x != 0.0) == (ref.k > 0)
    if case.event == "curv":
        # cg and pcg with a unit dinv: the same bits (sqrt(rr)^2 == rr)
        a = se.reference("cg", case.csr, case.b, se.KMAX, 0.0)
        b = se.reference("pcg", case.csr, case.b, se.KMAX, 0.0,
                         dinv=np.ones(case.N))
        assert a.same(b)
    if case.solvers == se.BI:
        # with a power of two as dinv the event is the same one
        kw = {"dinv": np.full(case.N, 4.0)}
        ref = se.reference("bicgstab", case.csr, case.b, se.KMAX, case.rtol, **kw)
        assert (ref.k, ref.status) == (case.k, case.status)
        assert ref.same(se.reference("bicgstab", case.csr, case.b, se.KMAX,
                                     case.rtol, dot=se.dot_chunked, **kw))


# ---- b. poisoned cases ---------------------------------------------------------------
NAN_FROM = {"b_nan": 0, "b_inf": 1, "b_huge": 1, "a_nan": 1}


@pytest.mark.parametrize("kind", se.POISONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_poisoned_cases_are_nan_from_where_they_say(shape, kind):
    csr, b = se.poisoned(tp._csr(shape), kind)
    for solver in se.SOLVERS:
        if solver == "cg_block":
            continue
        kw = se.solver_kwargs(solver, tp._csr(shape))
        ref = se.reference(solver, csr, b, se.KMAX, 1e-10, **kw)
        what = (shape, kind, solver)
        if kind == "b_tiny" and solver != "cg":
            assert ref.k == 0 and ref.status == 0, what
            assert np.all(ref.x == 0.0) and same_bits(ref.hist, np.zeros(1)), what
            continue
        assert ref.k == se.KMAX and ref.status == 0, what
        j = 1 if kind == "b_tiny" else NAN_FROM[kind]
        assert np.all(np.isnan(ref.hist[j:])) and np.all(np.isnan(ref.x)), what
        if j:
            want = 0.0 if kind == "b_tiny" else \
                math.sqrt(se.DOT(b, b)) if kind == "a_nan" else np.inf
            assert same_bits(ref.hist[:1], np.array([want])), what
            # ... in any order of the sum
            assert se.DOT(b, b) == se.dot_chunked(b, b) == se.dot_reversed(b, b)


# ---- c. scaled and negated systems -----------------------------------------------------
LO, HI = 2.0 ** -1000, 2.0 ** 1000


def _healthy(a, b):
    """no element of either run subnormal, infinite or NaN, or zero where the
    other is not -- with 22 binades to spare at either end, so that the one
    rounding by which cg()'s sqrt(rr)^2 differs from rr cannot matter"""
    for v in (a, b):
        assert np.all(np.isfinite(v))
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI)
    assert np.array_equal(a == 0, b == 0)


def _relation(base, got, e_x, e_h, sign=1.0):
    assert (got.k, got.status) == (base.k, base.status)
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x))
    assert same_bits(got.hist, np.ldexp(base.hist, e_h))
    _healthy(base.x, got.x), _healthy(base.hist, got.hist)


def _records_healthy(rec_a, rec_b):
    """every operand and result of every SpMV and dot product of two runs:
    r, p, z, A p, v, s, t, ... and rr, rz, p.Ap, rho, rv, ts, tt"""
    assert len(rec_a) == len(rec_b) and len(rec_a) > 0
    for a, b in zip(rec_a, rec_b):
        _healthy(a, b)


def _recorded(solver):
    """cg()'s reference is compiled C and cannot record: its scalars and
    vectors are those of pcg with a unit dinv (rz = rr) up to the rounding of
    sqrt(rr)^2, so that restatement records in its place"""
    return "pcg" if solver == "cg" else solver


def _kwargs(solver, csr, recorded, **kw):
    if solver == "cg" and recorded:
        return {"dinv": np.ones(len(csr[0]) - 1)}
    return se.solver_kwargs(solver, csr, **kw)


@pytest.mark.parametrize("solver", [s for s in se.SOLVERS if s != "cg_block"])
@pytest.mark.parametrize("shape", se.SCALED_SHAPES)
def test_scaling_relations_hold_on_the_references(shape, solver):
    csr = tp._csr(shape)
    b = se.scaled_rhs(csr)

    def run(c, rhs, record=None, **kw):
        return se.reference(_recorded(solver) if record is not None else solver,
                            c, rhs, se.SCALED_KMAX, se.SCALED_RTOL,
                            record=record, **kw)

    def pair(c, rhs, **opts):
        """the solve for the relation, and its recording"""
        rec = []
        run(c, rhs, record=rec, **_kwargs(solver, csr, True, **opts))
        return run(c, rhs, **_kwargs(solver, csr, False, **opts)), rec

    base, rec0 = pair(csr, b)
    assert 1 < base.k < se.SCALED_KMAX
    for s, t in se.SCALES:
        got, rec = pair(se.scale_csr(csr, s), np.ldexp(b, t), s=s)
        _relation(base, got, t - s, t)
        _records_healthy(rec0, rec)
        if solver == "pcg_chebyshev":
            got, rec = pair(se.scale_csr(csr, s), np.ldexp(b, t), s=s,
                            cheb_bounds=True)
            _relation(base, got, t - s, t)
            _records_healthy(rec0, rec)
    got, rec = pair(csr, -b)
    _relation(base, got, 0, 0, -1.0)
    _records_healthy(rec0, rec)
    if solver in se.NEGATED_A:
        got, rec = pair(se.scale_csr(csr, 0, -1.0), b)
        _relation(base, got, 0, 0, -1.0)
        _records_healthy(rec0, rec)


@pytest.mark.parametrize("solver", sorted(se.FLOOR))
def test_floor_pairs_hold_on_the_references(solver):
    """(s, t) with rr[0] = 2^-980 b.b, the case closest to 2^-1022"""
    csr = tp._csr("poisson11")
    b = se.clean_rhs(len(csr[0]) - 1)
    s, t, kmax = se.FLOOR[solver]
    runs = []
    for c, rhs, e in ((csr, b, 0), (se.scale_csr(csr, s), np.ldexp(b, t), s)):
        rec = []
        se.reference(_recorded(solver), c, rhs, kmax, 0.0, record=rec,
                     **_kwargs(solver, csr, True, s=e))
        runs.append((se.reference(solver, c, rhs, kmax, 0.0,
                                  **_kwargs(solver, csr, False, s=e)), rec))
    (base, rec0), (got, rec) = runs
    assert got.k == kmax and got.hist[0] ** 2 < 1e-290
    _relation(base, got, t - s, t)
    _records_healthy(rec0, rec)


# ---- mutants ------------------------------------------------------------------------------
def _pcg_mutant(stop):
    """test_gpu_pcg._pcg_ref with another stop rule: stop(rr, rr0, rtol)"""
    def ref(spmv, dot, b, dinv, kmax, rtol):
        x = np.zeros(len(b))
        r = np.array(b, dtype=np.float64)
        z = dinv * r
        p = z.copy()
        rz, rr0 = dot(r, z), dot(r, r)
        hist = [math.sqrt(rr0)]
        k = 0
        if rr0 == 0.0 or stop(rr0, rr0, -1.0):
            return x, 0, np.array(hist)
        while k < kmax:
            k += 1
            Ap = spmv(p)
            alpha = rz / dot(p, Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            z = dinv * r
            rz_new, rr = dot(r, z), dot(r, r)
            hist.append(math.sqrt(rr))
            if stop(rr, rr0, rtol):
                break
            beta = rz_new / rz
            rz = rz_new
            p = beta * p + z
        return x, k, np.array(hist)
    return ref


def _true_stop(rr, rr0, rtol):
    return math.sqrt(rr) / math.sqrt(rr0) < rtol


def test_the_restated_pcg_is_the_reference():
    csr, b = se.poisoned(tp._csr("poisson11"), "b_nan")
    kw = se.solver_kwargs("pcg", tp._csr("poisson11"))
    assert se.reference("pcg", csr, b, se.KMAX, 1e-10, **kw).same(
        se.reference("pcg", csr, b, se.KMAX, 1e-10, ref=_pcg_mutant(_true_stop),
                     **kw))


def test_mutant_stop_test_that_stops_on_nan():
    """`rnorm / rnorm0 >= rtol -> go on`"""
    mutant = _pcg_mutant(lambda rr, rr0, rtol:
                         not math.sqrt(rr) / math.sqrt(rr0) >= rtol)
    plain = tp._csr("poisson11")
    for kind in ("b_nan", "b_inf", "b_huge", "a_nan"):
        csr, b = se.poisoned(plain, kind)
        kw = se.solver_kwargs("pcg", plain)
        true = se.reference("pcg", csr, b, se.KMAX, 1e-10, **kw)
        got = se.reference("pcg", csr, b, se.KMAX, 1e-10, ref=mutant, **kw)
        assert true.k == se.KMAX and got.k <= 1, kind


def _bicgstab_swapped(spmv, dot, b, dinv, kmax, rtol):
    """test_gpu_bicgstab._bicgstab_ref with the two tests at the end of an
    iteration in the other order"""
    x = np.zeros(len(b))
    r = np.array(b, dtype=np.float64)
    rhat, p = r.copy(), r.copy()
    rho = rr0 = dot(r, r)
    hist = [math.sqrt(rr0)]
    k = status = 0
    if rr0 == 0.0:
        return x, 0, np.array(hist), 0
    while k < kmax:
        ph = p if dinv is None else dinv * p
        v = spmv(ph)
        rv = dot(rhat, v)
        if rv == 0.0:
            status = 1
            break
        alpha = rho / rv
        s = r - alpha * v
        sh = s if dinv is None else dinv * s
        t = spmv(sh)
        ts, tt = dot(t, s), dot(t, t)
        omega = 0.0 if tt == 0.0 else ts / tt
        x = x + alpha * ph
        x = x + omega * sh
        r = s - omega * t
        rr, rho_new = dot(r, r), dot(rhat, r)
        k += 1
        hist.append(math.sqrt(rr))
        if omega == 0.0 or rho_new == 0.0:  # the mutation: this test first
            status = 2
            break
        if math.sqrt(rr) / math.sqrt(rr0) < rtol:
            break
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
    return x, k, np.array(hist), status


def test_mutant_breakdown_before_tolerance():
    case = {c.name: c for c in EXACT}["2I_rtol"]
    true = se.reference("bicgstab", case.csr, case.b, se.KMAX, case.rtol)
    got = se.reference("bicgstab", case.csr, case.b, se.KMAX, case.rtol,
                       ref=_bicgstab_swapped)
    assert (true.k, true.status) == (1, 0) and (got.k, got.status) == (1, 2)
    # on a case without a breakdown the swapped restatement is the reference
    case = {c.name: c for c in EXACT}["ts0_k2"]
    assert se.reference("bicgstab", case.csr, case.b, 1, 0.0).same(
        se.reference("bicgstab", case.csr, case.b, 1, 0.0,
                     ref=_bicgstab_swapped))


def _block_case():
    """poisson11, nrhs 3: a live column, a NaN column, a live column"""
    csr = tp._csr("poisson11")
    N = len(csr[0]) - 1
    live = se.scaled_rhs(csr)
    B = np.stack([live, se.poisoned(csr, "b_nan")[1], se.clean_rhs(N)], axis=1)
    return csr, B


def test_mutant_cg_block_ends_with_the_first_column():
    csr, B = _block_case()
    its, hist, X = se.reference_block(csr, B, se.KMAX, 1e-4)
    assert its[1] == se.KMAX and 1 < its[0] < its[2] < se.KMAX
    # the mutant: every column ends at the smallest count
    its_m, hist_m, X_m = se.reference_block(csr, B, int(its.min()), 1e-4)
    assert its_m[2] != its[2] and not same_bits(X_m[:, 2], X[:, 2])
    assert its_m.max() != its.max()


def test_mutant_frozen_column_takes_a_zero_step():
    """A stopped column updated with alpha = 0 instead of not being written:
    harmless while the kernel keeps the columns apart.  Modelled with the leak
    it would expose: x_c += 0 * (p_c + the neighbours' p)."""
    csr, B = _block_case()
    its, hist, X = se.reference_block(csr, B, se.KMAX, 1e-4)
    assert its[0] < its[1] and np.all(np.isfinite(X[:, 0]))
    assert np.all(np.isnan(X[:, 1]))
    with np.errstate(all="ignore"):
        leak = X[:, 0] + 0.0 * (X[:, 0] + X[:, 1])
    assert not same_bits(leak, X[:, 0])
    # ... and the GPU test compares the live column with the solve in which
    # its neighbour is a zero column: the same bits on the reference
    B0 = B.copy()
    B0[:, 1] = 0.0
    its0, hist0, X0 = se.reference_block(csr, B0, se.KMAX, 1e-4)
    for c in (0, 2):
        assert its0[c] == its[c] and same_bits(X0[:, c], X[:, c])
        assert same_bits(hist0[c], hist[c])
    assert its0[1] == 0 and np.all(X0[:, 1] == 0.0)


def test_mutant_zero_rule_applied_to_cg():
    def mutant(spmv, dot, b, kmax, rtol):
        if dot(b, b) == 0.0:
            return np.zeros(len(b)), 0, np.zeros(1)
        raise AssertionError("only the zero rule is modelled")
    plain = tp._csr("poisson11")
    csr, b = se.poisoned(plain, "b_tiny")
    true = se.reference("cg", csr, b, se.KMAX, 1e-10)
    got = se.reference("cg", csr, b, se.KMAX, 1e-10, ref=mutant)
    assert true.k == se.KMAX and np.all(np.isnan(true.x)) and got.k == 0


def test_mutant_absolute_floor():
    """`rr < 1e-290 -> stop`: the scaled systems with t = -200 put rr[0] near
    2^-400 and do not reach it; the pair FLOOR of the GPU test does."""
    mutant = _pcg_mutant(lambda rr, rr0, rtol:
                         _true_stop(rr, rr0, rtol) or rr < 1e-290)
    csr = tp._csr("poisson11")
    b = se.clean_rhs(len(csr[0]) - 1)
    s, t, kmax = se.FLOOR["pcg"]
    kws = se.solver_kwargs("pcg", csr, s=s)
    true = se.reference("pcg", se.scale_csr(csr, s), np.ldexp(b, t), kmax, 0.0,
                        **kws)
    got = se.reference("pcg", se.scale_csr(csr, s), np.ldexp(b, t), kmax, 0.0,
                       ref=mutant, **kws)
    assert true.k == kmax and got.k < kmax
