"""The cases of minres_edges.py do what they claim, on minres_cases.minres_ref
alone (no GPU): the table of the exact cases and of the scaling floor under
three summation orders, the search behind the second status-2 case, the
outcomes of the poisoned cases and which of them the device is held to bit for
bit, the scaling and negation relations with every operand recorded, and four
mutants of the restatement that the cases tell from the real one."""
import math

import numpy as np
import pytest

import minres_cases as mc
import minres_edges as me
import oracle
from minres_edges import same_bits

EXACT = me.exact_cases()
BY_NAME = {c.name: c for c in EXACT}
LO, HI = 2.0 ** -900, 2.0 ** 1000


def _equal(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == got.k + 1, what
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what  # +0.0 where the table says 0


# ---- the reference's scalar part ---------------------------------------------------------
def _scripted(values):
    """a dot product that returns the given values in turn"""
    it = iter(values)
    return lambda a, b: np.float64(next(it))


@pytest.mark.parametrize("ry0,ry1,want", [
    # ry at the start, ry of the first step -> (k, status, hist as text)
    (-1.0, None, (0, 2, "0.0")),
    (-np.inf, None, (0, 2, "0.0")),
    (-0.0, None, (0, 0, "-0.0")),       # not < 0; sqrt(-0.0) == 0: the zero rule
    (np.nan, 1.0, (2, 0, "nan nan nan")),   # NaN is not < 0 and not == 0
    # sqrt(inf) = inf, 1 / inf = 0; phibar = sn * inf, inf / inf is not < rtol
    (np.inf, 1.0, (2, 0, "inf inf inf")),
    (4.0, -1.0, (0, 2, "2.0")),
    (4.0, np.nan, (2, 0, "2.0 nan nan")),
    (4.0, np.inf, (2, 0, "2.0 nan nan")),   # gamma = inf, sn = inf / inf
])
def test_the_scalar_part_follows_the_kernels_branches_and_never_raises(
        ry0, ry1, want):
    """minres_ref works in Python floats with math.sqrt: a negative ry is caught
    by `ry < 0` before the square root, as in start and step, a NaN or Inf
    passes through sqrt and every quotient without an exception"""
    dots = [ry0] + ([] if ry1 is None else [1.0, ry1, 1.0, ry1])
    with np.errstate(all="ignore"):
        x, k, hist, status = mc.minres_ref(lambda q: q, _scripted(dots), None,
                                           np.ones(2), 2, 1e-10)
    assert (k, status) == want[:2] and len(hist) == k + 1
    assert " ".join(str(float(h)) for h in hist) == want[2]


# ---- a. exact cases ---------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_exact_cases_give_the_table(case):
    """(k, status, history, x) of the table, for both N, at kmax = 40 and at the
    step of the exit, under three summation orders"""
    assert case.k <= 2 and len(case.hist) == case.k + 1
    for tail in (False, True):
        csr, b = case.system(tail)
        N = len(b)
        assert N <= 4097 and N % 2 == int(tail)
        d = case.dinv(tail)
        bMb = me.DOT(b, b if d is None else d * b)
        if case.name == "neg0":
            assert bMb < 0.0
        else:  # a power of four: beta1 and 1 / beta1 are powers of two
            assert bMb == case.hist[0] ** 2 and math.log2(bMb) % 2 == 0
        want = case.want(tail)
        for kmax in case.kmaxes():
            for dot in me.ORDERS:
                got = me.reference(csr, b, kmax, 0.0, minv=case.minv(tail),
                                   dot=dot)
                _equal(got, want, (case.id, tail, kmax, dot.__name__))
        Ax = oracle.csr_spmv(*csr, want.x)
        if case.status == 1:
            assert same_bits(Ax, b), case.id
        else:
            assert np.any(Ax != b), case.id


def test_the_rows_reach_the_exits_they_are_for():
    assert len(BY_NAME) == len(EXACT) == 10
    assert sorted(c.status for c in EXACT) == [1] * 6 + [2, 2, 3, 3]
    for name in ("two_i", "perm", "indef", "sing3"):
        c, d = BY_NAME[name], BY_NAME[name + "-d"]
        assert c.dinv_block is None and set(d.dinv_block) == {me.EXACT_DINV}
        assert (c.k, c.status) == (d.k, d.status)
        assert same_bits(c.xblock, d.xblock)
    # the kmax stop and the exit in one step
    assert BY_NAME["two_i"].kmaxes() == (me.KMAX, 1)
    assert BY_NAME["sing3"].kmaxes() == (me.KMAX, 3)
    assert BY_NAME["neg0"].kmaxes() == (me.KMAX, 0)
    assert BY_NAME["neg1"].kmaxes() == (me.KMAX, 2)
    # status 2 with and without an iterate; x of neg1 is not the x of k = 0
    assert BY_NAME["neg0"].k == 0 and BY_NAME["neg1"].k == 1
    assert np.any(BY_NAME["neg1"].xblock != 0.0)
    # sqrt(2): one rounding away from 32 / sqrt(2) and from 0.5
    assert abs(me.H_R2 - 32.0 / math.sqrt(2.0)) <= 2.0 ** -48
    assert me.X_R2 == 0.5 - 2.0 ** -53


def test_alfa_is_zero_twice_on_perm_and_the_singular_block_is_singular():
    c = BY_NAME["perm"]
    csr, b = c.system(True)
    rec = []
    me.reference(csr, b, me.KMAX, 0.0, record=rec)
    # _recording: spmv appends 2 arrays, dot 3; an iteration is spmv, v.Av, r2.y
    scalars = [float(a[0]) for a in rec if a.shape == (1,)]
    assert scalars[0] == 1024.0 and scalars[1] == 0.0 and scalars[3] == 0.0
    block = np.array(me.SING3[0], float)
    assert np.linalg.matrix_rank(block) == 2
    null = np.array([1.0, 0.0, -1.0])
    assert np.all(block @ null == 0.0) and null @ np.array(me.SING3[1]) != 0.0


def test_the_search_finds_the_second_status_2_case():
    assert me.search_negative(2) is None
    A, b, dinv, nb, k = me.search_negative(3)
    assert (A, b) == me.NEG1 and dinv == me.NEG1_DINV
    assert (nb, k) == (me.NEG1_NB, 1) == (BY_NAME["neg1"].nb, BY_NAME["neg1"].k)


def test_the_two_rank_cases_are_cut_inside_a_block():
    for name in me.TWO_RANKS:
        c = BY_NAME[name]
        N = len(c.system(True)[1])
        cut = int(oracle.owner_ranges(2, N)[1])
        assert 0 < cut < N - 1 and cut % len(c.block) != 0, (name, cut)
    for shape in me.POISON_SHAPES:
        N = len(me.csr_of(shape)[0]) - 1
        b = me.rank1_nan(N)
        cut = int(oracle.owner_ranges(2, N)[1])
        assert np.all(np.isfinite(b[:cut])) and np.isnan(b[cut:]).sum() == 1


# ---- b. the floor of scaling ----------------------------------------------------------------
@pytest.mark.parametrize("s", me.FLOOR_S)
@pytest.mark.parametrize("name", me.FLOOR_CASES)
def test_floor_cases_give_the_table(name, s):
    for case in (BY_NAME[name], BY_NAME[name + "-d"]):
        for tail in (False, True):
            csr, b, d, want = me.floor_case(case, s, tail)
            for dot in me.ORDERS:
                got = me.reference(csr, b, me.KMAX, 0.0,
                                   minv=None if d is None else me.jacobi(d),
                                   dot=dot)
                _equal(got, want, (case.id, s, tail, dot.__name__))
    # what the table says: beyond +-510 only the preconditioned rows are right
    plain = me.FLOOR[(name, s)]
    unscaled = BY_NAME[name]
    right = (plain[0], plain[1]) == (unscaled.k, unscaled.status) and \
        same_bits(np.array(plain[3], float), np.ldexp(unscaled.xblock, -s))
    assert right == (s == -520), (name, s)


# ---- c. poisoned data ---------------------------------------------------------------------------
def _poisoned_runs(shape, kind, pre):
    plain = me.csr_of(shape)
    csr, b = me.poisoned(plain, kind)
    minv = me.minv_of(pre, shape)
    return b, [me.reference(csr, b, me.POISON_KMAX, me.POISON_RTOL, minv=minv,
                            dot=dot) for dot in me.ORDERS]


@pytest.mark.parametrize("kind", me.POISONS)
@pytest.mark.parametrize("shape", me.POISON_SHAPES)
def test_poisoned_outcomes(shape, kind):
    at_kmax, status, h0, x_nan = me.POISON_OUTCOME[kind]
    for pre in me.PRE_POISON:
        b, runs = _poisoned_runs(shape, kind, pre)
        got = runs[0]
        what = (shape, kind, pre)
        bits = got.same(runs[1]) and got.same(runs[2])
        print(shape, kind, pre, "k", got.k, "status", got.status, "hist[0]",
              got.hist[0], "held to bits" if bits else
              "held to (k, status, NaN and Inf pattern)")
        assert bits == (what not in me.WEAK), what
        # the weaker comparison holds for every case
        assert me.pattern(got) == me.pattern(runs[1]) == me.pattern(runs[2]), what
        assert got.k == (me.POISON_KMAX if at_kmax else 0), what
        assert got.status == status and len(got.hist) == got.k + 1, what
        assert np.all(np.isnan(got.hist[1:])), what
        if h0 == "nan":
            assert np.isnan(got.hist[0]), what
        elif h0 == "finite":
            assert np.isfinite(got.hist[0]) and got.hist[0] > 0.0, what
            if pre == "none":  # integers: the same in any order
                assert got.hist[0] == math.sqrt(me.DOT(b, b)), what
        else:
            assert same_bits(got.hist[:1],
                             np.array([np.inf if h0 == "inf" else h0])), what
        assert np.all(np.isnan(got.x)) if x_nan else \
            same_bits(got.x, np.zeros(len(b))), what
        if kind == "b_tiny":
            assert np.all(b != 0.0) and me.DOT(b, b) == 0.0


def test_enough_poisoned_cases_keep_the_bit_comparison():
    kinds = {kind for _, kind, _ in me.WEAK}
    assert len(set(me.POISONS) - kinds) >= 3
    assert len(me.POISONS) == 5 == len(me.POISON_OUTCOME)


# ---- d. scaled and negated systems ------------------------------------------------------------
def _healthy(a, b):
    """no element of either run infinite, NaN or below 2^-900, or zero where
    the other is not"""
    for v in (a, b):
        assert np.all(np.isfinite(v))
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), nz.min()
    assert np.array_equal(a == 0, b == 0)


def _records_healthy(rec_a, rec_b):
    assert len(rec_a) == len(rec_b) and len(rec_a) > 0
    for a, b in zip(rec_a, rec_b):
        _healthy(a, b)


def _relation(base, got, e_x, e_h, sign=1.0):
    assert (got.k, got.status) == (base.k, base.status)
    assert same_bits(got.x, sign * np.ldexp(base.x, e_x))
    assert same_bits(got.hist, np.ldexp(base.hist, e_h))
    _healthy(base.x, got.x), _healthy(base.hist, got.hist)


def _scaled_run(shape, pre, symmetric, s=0, t=0, sign_a=1.0, sign_b=1.0):
    csr = me.csr_of(shape)
    b = me.scaled_rhs(csr)
    rec = []
    A = me.scale_csr(csr, s, sign_a)
    got = me.reference(A, sign_b * np.ldexp(b, t), me.SCALED_KMAX,
                       me.SCALED_RTOL, minv=me.minv_of(pre, shape, s),
                       record=rec, spmv=me.spmv_of(A, symmetric))
    return got, rec


SCALED_CASES = [(shape, pre, sym) for shape, pres in me.SCALED.items()
                for pre in pres
                for sym in ((False, True) if shape in me.SYMMETRIC else (False,))
                if not (sym and pre not in ("none", "jacobi"))]


@pytest.mark.parametrize("shape,pre,symmetric", SCALED_CASES)
def test_scaling_relations_hold_on_the_reference(shape, pre, symmetric):
    base, rec0 = _scaled_run(shape, pre, symmetric)
    print(shape, pre, symmetric, "k", base.k, "status", base.status,
          "hist[k] / hist[0]", base.hist[-1] / base.hist[0])
    assert 1 < base.k <= me.SCALED_KMAX and base.status == 0
    for s, t in me.PAIRS:
        assert s % 2 == 0
        got, rec = _scaled_run(shape, pre, symmetric, s, t)
        _relation(base, got, t - s, me.hist_exponent(pre, s, t))
        _records_healthy(rec0, rec)
    got, rec = _scaled_run(shape, pre, symmetric, sign_b=-1.0)
    _relation(base, got, 0, 0, -1.0)
    _records_healthy(rec0, rec)
    if pre in me.NEGATED_A:
        got, rec = _scaled_run(shape, pre, symmetric, sign_a=-1.0)
        _relation(base, got, 0, 0, -1.0)
        _records_healthy(rec0, rec)


def test_an_odd_s_with_jacobi_breaks_the_history_relation():
    """s = 101: sqrt(ry) picks up a sqrt(2), so no power of two carries one
    history into the other -- the exponent rule t - s / 2 is for even s only"""
    base, _ = _scaled_run("shift11", "jacobi", False)
    got, _ = _scaled_run("shift11", "jacobi", False, me.ODD_S, 0)
    assert me.hist_exponent("jacobi", me.ODD_S, 0) == -50  # what the rule says
    for e in (-51, -50):
        for i in range(min(base.k, got.k) + 1):  # not one entry fits
            assert got.hist[i] != math.ldexp(base.hist[i], e), (e, i)
    ratio = got.hist[0] / base.hist[0] * 2.0 ** 50 * math.sqrt(2.0)
    assert abs(ratio - 1.0) <= 2.0 ** -50
    # without a preconditioner the same s is exact
    base, _ = _scaled_run("shift11", "none", False)
    got, _ = _scaled_run("shift11", "none", False, me.ODD_S, 0)
    _relation(base, got, -me.ODD_S, 0)


# ---- mutants of the restatement -------------------------------------------------------------
def _restated(mutant=None):
    """minres_ref once more, with one line changed per mutant"""
    f = np.float64

    def ref(spmv, dot, minv, b, kmax, rtol):
        apply = (lambda q: q) if minv is None else minv
        b = np.asarray(b, np.float64)
        x = np.zeros(len(b))
        r1 = r2 = b.copy()
        y = apply(r2)
        ry = float(dot(r2, y))
        if (not ry >= 0.0) if mutant == "not_ge" else ry < 0.0:
            return x, 0, np.array([0.0]), 2
        beta1 = math.sqrt(ry)
        hist = [beta1]
        if beta1 == 0.0:
            return x, 0, np.array(hist), 0
        oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, \
            -1.0, 0.0
        w = np.zeros(len(b))
        w2 = np.zeros(len(b))
        k = status = 0
        v = y * f(1.0 / beta)
        while k < kmax:
            Av = spmv(v)
            alfa = float(dot(v, Av))
            if k == 0:
                t = Av - f(alfa / beta) * r2
            else:
                t = (Av - f(beta / oldb) * r1) - f(alfa / beta) * r2
            r1 = r2
            r2 = t
            y = apply(r2)
            ry = float(dot(r2, y))
            if (not ry >= 0.0) if mutant == "not_ge" else ry < 0.0:
                status = 2
                break
            oldb = beta
            beta = math.sqrt(ry)
            if mutant == "beta_first" and beta == 0.0:
                status = 1
                break
            oldeps = epsln
            delta = cs * dbar + sn * alfa
            gbar = sn * dbar - cs * alfa
            epsln = sn * beta
            dbar = -cs * beta
            gamma = math.sqrt(gbar * gbar + beta * beta)
            if gamma == 0.0:
                if mutant != "no_gamma":
                    status = 3
                    break
                gamma = f(gamma)  # IEEE's 0 / 0 and 1 / 0, as a device would
            cs = float(gbar / gamma)
            sn = float(beta / gamma)
            phi = cs * phibar
            phibar = sn * phibar
            w1 = w2
            w2 = w
            w = ((v - f(oldeps) * w1) - f(delta) * w2) * f(1.0 / gamma)
            x = x + f(phi) * w
            k += 1
            hist.append(abs(phibar))
            if beta == 0.0:
                status = 1
                break
            if (not hist[k] / hist[0] >= rtol) if mutant == "stop_not_ge" \
                    else hist[k] / hist[0] < rtol:
                break
            v = y * f(1.0 / beta)
        return x, k, np.array(hist), status
    return ref


def _failures():
    """the ids of the exact, floor and poisoned cases (tail row, first order)
    that the current mc.minres_ref does not pass"""
    bad = []

    def check(cid, got, want, bits=True):
        ok = got.same(want) if bits else me.pattern(got) == me.pattern(want)
        if not (ok and len(got.hist) == got.k + 1):
            bad.append(cid)

    for case in EXACT:
        csr, b = case.system(True)
        for kmax in case.kmaxes():
            check((case.id, kmax),
                  me.reference(csr, b, kmax, 0.0, minv=case.minv(True)),
                  case.want(True))
    for name in me.FLOOR_CASES:
        for s in me.FLOOR_S:
            for case in (BY_NAME[name], BY_NAME[name + "-d"]):
                csr, b, d, want = me.floor_case(case, s, True)
                check((case.id, s), me.reference(
                    csr, b, me.KMAX, 0.0,
                    minv=None if d is None else me.jacobi(d)), want)
    for shape in me.POISON_SHAPES:
        for kind in me.POISONS:
            for pre in me.PRE_POISON:
                want = _POISON_WANT[(shape, kind, pre)]
                csr, b = me.poisoned(me.csr_of(shape), kind)
                got = me.reference(csr, b, me.POISON_KMAX, me.POISON_RTOL,
                                   minv=me.minv_of(pre, shape))
                check((shape, kind, pre), got, want,
                      (shape, kind, pre) not in me.WEAK)
    return bad


_POISON_WANT = {}


@pytest.fixture(scope="module")
def poison_want():
    for shape in me.POISON_SHAPES:
        for kind in me.POISONS:
            for pre in me.PRE_POISON:
                _POISON_WANT[(shape, kind, pre)] = \
                    _poisoned_runs(shape, kind, pre)[1][0]
    return _POISON_WANT


def test_the_restatement_of_this_file_is_the_reference(poison_want, monkeypatch):
    assert _failures() == []
    monkeypatch.setattr(mc, "minres_ref", _restated())
    assert _failures() == []


@pytest.mark.parametrize("mutant,caught_by", [
    # beta == 0 tested before hist[k] is written (and before x moves)
    ("beta_first", ("two_i", me.KMAX)),
    # gamma == 0 dropped: 0 / 0 goes on to kmax
    ("no_gamma", ("sing3", me.KMAX)),
    # ry < 0 written as !(ry >= 0): a NaN stops the solve with status 2
    ("not_ge", ("shift11", "b_nan", "none")),
    # the stop written as !(res / hist0 >= rtol): a NaN "converges"
    ("stop_not_ge", ("saddle500", "a_nan", "jacobi")),
])
def test_mutants_of_the_restatement_fail(poison_want, monkeypatch, mutant,
                                         caught_by):
    monkeypatch.setattr(mc, "minres_ref", _restated(mutant))
    bad = _failures()
    print(mutant, "fails", bad)
    assert caught_by in bad
