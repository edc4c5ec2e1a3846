"""The cases of lsqr_edges.py do what they claim, on lsqr_cases.lsqr_ref alone
(no GPU): the table of the exact cases and of the scaling floor under three
summation orders, the outcomes of the poisoned cases and which of them the
device is held to bit for bit, the scaling and negation relations with every
operand recorded, and four mutants of the restatement that the cases tell from
the real one.

Every zero test of lsqr is on a square root (>= 0 or NaN), so `== 0` turned
into `<= 0` is the same program; the mutant of that family is the guard `beta
!= 0` (true on a NaN) turned into `beta > 0` (false on one)."""
import numpy as np
import pytest

import lsqr_cases as lc
import lsqr_edges as le
import oracle
from lsqr_cases import _div, _sqrt, f
from lsqr_edges import same_bits

EXACT = le.exact_cases()
BY_NAME = {c.name: c for c in EXACT}
LO, HI = 2.0 ** -900, 2.0 ** 1000


def _equal(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == len(got.hist_ar) == got.k + 1, what
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.hist_ar, want.hist_ar), (what, got.hist_ar[:4])
    assert same_bits(got.x, want.x), what  # +0.0 where the table says 0


# ---- a. exact cases ---------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_exact_cases_give_the_table(case):
    assert case.k <= 1 and len(case.hist) == len(case.hist_ar) == case.k + 1
    for tail in (False, True):
        csr, ncols, b = case.system(tail)
        M = len(b)
        assert 1000 <= M <= 4097 and ncols <= 4097
        assert M == len(case.block) * case.nb + int(tail)
        if case.name != "zero":
            assert le.DOT(b, b) == 1024.0  # beta = 32, ib = 2^-5
        want = case.want(tail)
        for kmax in case.kmaxes():
            for dot in le.ORDERS:
                got = le.reference(csr, ncols, b, kmax, 0.0, case.ltol,
                                   case.damp, dot=dot)
                _equal(got, want, (case.id, tail, kmax, dot.__name__))
        Ax = oracle.csr_spmv(*csr, want.x)
        assert same_bits(Ax, b) == (case.solved or case.name == "zero"), case.id


def test_the_rows_reach_the_exits_they_are_for():
    assert len(BY_NAME) == len(EXACT) == 9
    assert sorted((c.k, c.status) for c in EXACT) == \
        [(0, 0), (0, 2), (0, 2), (1, 1)] + [(1, 2)] * 5
    # beta == 0 against alpha_n == 0 with beta != 0: hist_r[1]
    assert BY_NAME["two_i"].hist[1] == 0.0 and BY_NAME["tall_an0"].hist[1] > 0.0
    assert BY_NAME["tall_an0"].hist_ar[1] == 0.0
    assert BY_NAME["ltol"].hist_ar[1] > 0.0 and BY_NAME["ltol"].hist[1] > 0.0
    assert len(BY_NAME["tall4"].block) == 4
    # sqrt(2): one rounding away from 32 / sqrt(2)
    assert abs(BY_NAME["ltol"].hist[1] - 32.0 / np.sqrt(2.0)) <= 2.0 ** -47
    # the damped solution, and the minimum-norm one
    assert abs(BY_NAME["damped"].xblock[0] - 0.25) <= 2.0 ** -54
    assert np.all(BY_NAME["wide4"].xblock == 0.25)


def test_the_narrow_blocks_of_the_issue_meet_sqrt_2():
    """[[1],[1]] with b = (1,1) and [[1,1]]: alpha * alpha = 2 whatever NB is,
    ia rounds and the first step does not end the process exactly"""
    for block, rhs, nb in ((((1,), (1,)), (1, 1), 512), (((1, 1),), (1,), 1024)):
        csr, ncols, b = le.rect_system(block, rhs, nb, False)
        got = le.reference(csr, ncols, b, 1, 0.0)
        assert got.hist_ar[0] == 32.0 * np.sqrt(2.0)


def test_the_two_rank_cases_are_cut_inside_a_block():
    for name in le.TWO_RANKS:
        c = BY_NAME[name]
        csr, ncols, b = c.system(True)
        assert ncols == len(b)  # square: rows and columns share one map
        cut = int(oracle.owner_ranges(2, len(b))[1])
        assert 0 < cut < len(b) - 1 and cut % len(c.block) != 0, (name, cut)
    # and the halo of the first is not empty
    csr, _, b = BY_NAME[le.TWO_RANKS[0]].system(True)
    cut = int(oracle.owner_ranges(2, len(b))[1])
    assert len(oracle.localise_rows(*csr, 0, cut)[3]) > 0


# ---- b. the floor of scaling ----------------------------------------------------------------
@pytest.mark.parametrize("s", le.FLOOR_S)
@pytest.mark.parametrize("name", le.FLOOR_CASES)
def test_floor_cases_give_the_table(name, s):
    case = BY_NAME[name]
    for tail in (False, True):
        csr, ncols, b, damp, want = le.floor_case(case, s, tail)
        for dot in le.ORDERS:
            got = le.reference(csr, ncols, b, le.KMAX, 0.0, case.ltol, damp,
                               dot=dot)
            _equal(got, want, (case.id, s, tail, dot.__name__))
    # beyond +-510 the answer is wrong: only s = -520 is the unscaled row
    assert (le.FLOOR[s] == "scaled") == (s == -520)


# ---- c. poisoned data ---------------------------------------------------------------------------
def _poisoned_runs(shape, kind):
    return [le.poisoned_reference(shape, kind, dot=dot) for dot in le.ORDERS]


@pytest.mark.parametrize("kind", le.KINDS)
@pytest.mark.parametrize("shape", le.POISON_SHAPES)
def test_poisoned_outcomes(shape, kind):
    k, status, h0, x_nan = le.POISON_OUTCOME[kind]
    runs = _poisoned_runs(shape, kind)
    got, what = runs[0], (shape, kind)
    bits = got.same(runs[1]) and got.same(runs[2])
    print(shape, kind, "k", got.k, "status", got.status, "hist_r[0]", got.hist[0],
          "held to bits" if bits else "held to (k, status, NaN and Inf pattern)")
    assert bits == (what not in le.WEAK), what
    assert le.pattern(got) == le.pattern(runs[1]) == le.pattern(runs[2]), what
    assert (got.k, got.status) == (k, status), what
    assert len(got.hist) == len(got.hist_ar) == got.k + 1, what
    if h0 == "nan":
        assert np.isnan(got.hist[0]), what
    elif h0 == "finite":
        assert np.isfinite(got.hist[0]) and got.hist[0] > 0.0, what
    else:
        assert same_bits(got.hist[:1], np.array([np.inf if h0 == "inf" else h0]))
    if x_nan is None:
        assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(got.hist))
    else:
        assert np.all(np.isnan(got.x)) if x_nan else \
            same_bits(got.x, np.zeros(len(got.x))), what
    if kind in ("b_nan", "b_inf", "a_nan"):
        assert np.all(np.isnan(got.hist[1:])) and np.all(np.isnan(got.hist_ar))
    if kind == "damp_huge":  # the wrong answer that looks converged
        assert got.hist[1] == 0.0 and np.isnan(got.hist_ar[1])
    if kind == "damp_tiny":  # the solve without damp, bit for bit
        csr, ncols, b, _ = le.poisoned_case(shape, kind)
        plain = le.reference(csr, ncols, b, le.POISON_KMAX, le.POISON_RTOL,
                             le.POISON_LTOL, 0.0)
        assert got.same(plain)


def test_the_weak_share():
    combos = [(shape, kind) for shape in le.POISON_SHAPES for kind in le.KINDS]
    assert le.WEAK <= set(combos)
    assert 4 * len(le.WEAK) <= len(combos), (len(le.WEAK), len(combos))
    for kind in le.DAMP_POISONS:  # damp * damp leaves the range
        d = le.DAMP_POISONS[kind]
        assert d * d in (0.0, np.inf) and np.isfinite(d) and d > 0.0
    for shape in le.POISON_SHAPES:
        b = le.damp_rhs(len(le.csr_of(shape)[0][0]) - 1)
        assert np.log2(le.DOT(b, b)) % 2 == 0


# ---- d. scaled and negated systems ------------------------------------------------------------
def _healthy(a, b):
    for v in (a, b):
        assert np.all(np.isfinite(v))
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), nz.min()
    assert np.array_equal(a == 0, b == 0)


def _relation(base, got, s, t, sign=1.0):
    assert (got.k, got.status) == (base.k, base.status)
    assert same_bits(got.x, sign * np.ldexp(base.x, t - s))
    assert same_bits(got.hist, np.ldexp(base.hist, t))
    assert same_bits(got.hist_ar, np.ldexp(base.hist_ar, s + t))
    for u, v in ((base.x, got.x), (base.hist, got.hist),
                 (base.hist_ar, got.hist_ar)):
        _healthy(u, v)


def _scaled_run(shape, kind, damp, s=0, t=0, sign_a=1.0, sign_b=1.0):
    csr, ncols = le.csr_of(shape)
    b = le.scaled_rhs(shape, kind)
    rec = []
    got = le.reference(le.scale_csr(csr, s, sign_a), ncols,
                       sign_b * np.ldexp(b, t), le.SCALED_KMAX, le.SCALED_RTOL,
                       le.SCALED_LTOL, float(np.ldexp(damp, s)), record=rec)
    return got, rec


@pytest.mark.parametrize("shape,kind,damp", le.SCALED)
def test_scaling_relations_hold_on_the_reference(shape, kind, damp):
    base, rec0 = _scaled_run(shape, kind, damp)
    print(shape, kind, damp, "k", base.k, "status", base.status)
    assert 1 < base.k <= le.SCALED_KMAX
    assert base.status == (1 if (shape, kind) == ("tall", "rand") else 0)
    runs = [(s, t, 1.0, 1.0) for s, t in le.PAIRS] + [(0, 0, 1.0, -1.0),
                                                     (0, 0, -1.0, 1.0)]
    for s, t, sa, sb in runs:
        got, rec = _scaled_run(shape, kind, damp, s, t, sa, sb)
        _relation(base, got, s, t, sa * sb)
        assert len(rec) == len(rec0) > 0
        for u, v in zip(rec0, rec):
            _healthy(u, v)


# ---- mutants of the restatement -------------------------------------------------------------
def _restated(mutant=None):
    """lsqr_ref once more, with one line changed per mutant"""
    def ref(spmv, spmvt, dot, b, kmax, rtol, ltol, damp):
        with np.errstate(all="ignore"):
            ut = np.array(b, np.float64)
            beta = _sqrt(dot(ut, ut))
            hist_r, hist_ar = [beta], [0.0]
            x = np.zeros(len(spmvt(ut)))
            if beta == 0.0:
                return x, 0, np.array(hist_r), np.array(hist_ar), 0
            ib = _div(1.0, beta)
            vt = spmvt(ut) * f(ib)
            alpha = _sqrt(dot(vt, vt))
            hist_ar[0] = alpha * beta
            if alpha == 0.0:
                return x, 0, np.array(hist_r), np.array(hist_ar), 2
            ia = _div(1.0, alpha)
            w = vt * f(ia)
            phibar, rhobar, anorm2, psi2 = beta, alpha, 0.0, 0.0
            k = status = 0
            while k < kmax:
                ut = spmv(vt) * f(ia) - f(alpha) * (ut * f(ib))
                beta = _sqrt(dot(ut, ut))
                anorm2 = anorm2 + alpha * alpha + beta * beta + damp * damp
                guard = beta > 0.0 if mutant == "beta_gt" else beta != 0.0
                if guard or mutant == "no_beta_guard":
                    ib = _div(1.0, beta)
                    vn = spmvt(ut) * f(ib) - f(beta) * (vt * f(ia))
                    alpha_n = _sqrt(dot(vn, vn))
                else:
                    vn, alpha_n = vt, 0.0
                rhobar1 = _sqrt(rhobar * rhobar + damp * damp)
                cs1 = _div(rhobar, rhobar1)
                sn1 = _div(damp, rhobar1)
                psi = sn1 * phibar
                phibar = cs1 * phibar
                psi2 = psi2 + psi * psi
                rho = _sqrt(rhobar1 * rhobar1 + beta * beta)
                cs = _div(rhobar1, rho)
                sn = _div(beta, rho)
                theta = sn * alpha_n
                rhobar = -cs * alpha_n
                phi = cs * phibar
                phibar = sn * phibar
                x = x + f(_div(phi, rho)) * w
                k += 1
                hist_r.append(_sqrt(phibar * phibar + psi2))
                hist_ar.append(abs(phibar * alpha_n * cs))
                if mutant == "kmax_first" and k == kmax:
                    break
                if beta == 0.0 or (alpha_n == 0.0 and mutant != "no_an0"):
                    status = 2
                    break
                r = _div(hist_r[k], hist_r[0])
                if (not r >= rtol) if mutant == "stop_not_ge" else r < rtol:
                    break
                if _div(hist_ar[k], _sqrt(anorm2) * hist_r[k]) < ltol:
                    status = 1
                    break
                vt = vn
                alpha = alpha_n
                ia = _div(1.0, alpha)
                w = vt * f(ia) - f(_div(theta, rho)) * w
            return x, k, np.array(hist_r), np.array(hist_ar), status
    return ref


_POISON_WANT = {}


@pytest.fixture(scope="module")
def poison_want():
    for shape in le.POISON_SHAPES:
        for kind in le.KINDS:
            _POISON_WANT[(shape, kind)] = le.poisoned_reference(shape, kind)
    return _POISON_WANT


def _failures(ref):
    """the ids of the exact, floor and poisoned cases (tail row, first order)
    that the restatement `ref` does not pass"""
    bad = []

    def check(cid, got, want, bits=True):
        ok = got.same(want) if bits else le.pattern(got) == le.pattern(want)
        if not (ok and len(got.hist) == len(got.hist_ar) == got.k + 1):
            bad.append(cid)

    for case in EXACT:
        csr, ncols, b = case.system(True)
        for kmax in case.kmaxes():
            check((case.id, kmax), le.reference(csr, ncols, b, kmax, 0.0,
                                                case.ltol, case.damp, ref=ref),
                  case.want(True))
    for name in le.FLOOR_CASES:
        for s in le.FLOOR_S:
            case = BY_NAME[name]
            csr, ncols, b, damp, want = le.floor_case(case, s, True)
            check((name, s), le.reference(csr, ncols, b, le.KMAX, 0.0,
                                          case.ltol, damp, ref=ref), want)
    for key, want in _POISON_WANT.items():
        check(key, le.poisoned_reference(*key, ref=ref), want,
              key not in le.WEAK)
    return bad


def test_the_restatement_of_this_file_is_the_reference(poison_want):
    assert _failures(lc.lsqr_ref) == []
    assert _failures(_restated()) == []


@pytest.mark.parametrize("mutant,caught_by", [
    # alpha_n == 0 dropped from the breakdown test: 1 / 0 goes on to kmax
    ("no_an0", ("tall_an0", le.KMAX)),
    # the division 1 / beta moved in front of the test that guards it
    ("no_beta_guard", ("two_i", le.KMAX)),
    # beta != 0 written as beta > 0: a NaN "ends the bidiagonalisation"
    ("beta_gt", ("tall", "b_nan")),
    # the stop written as !(res / hist0 >= rtol): a NaN "converges"
    ("stop_not_ge", ("convdiff11_2", "a_nan")),
    # the kmax test in front of the breakdown test: status 0 where they coincide
    ("kmax_first", ("ltol", 1)),
])
def test_mutants_of_the_restatement_fail(poison_want, mutant, caught_by):
    bad = _failures(_restated(mutant))
    print(mutant, "fails", bad)
    assert caught_by in bad
