"""The cases of cgs_edges.py do what they claim, on cgs_cases.cgs_ref alone (no
GPU): the exact table and the scaling floor under three summation orders, the
search behind the `early` row, the poisoned outcomes and the WEAK share, the
scaling and negation relations with every operand recorded, and mutants of the
reference (its own source with ONE line replaced) that the tables tell from it.

rr and rrn are sums of squares (>= 0 or NaN), so `rr == 0` turned into `rr <= 0`
is the same program; the mutant of that family is `not pq > 0` turned into `pq
<= 0`, which differs on a NaN."""
import inspect

import numpy as np
import pytest

import cgs_cases as cc
import cgs_edges as ce
from cgs_edges import same_bits

EXACT = ce.exact_cases()
BY_NAME = {c.name: c for c in EXACT}
LO, HI = 2.0 ** -900, 2.0 ** 1000


def _equal(got, want, what):
    assert (got.k, got.its, got.status) == (want.k, want.its, want.status), \
        (what, got.k, got.its, got.status)
    assert same_bits(got.hist, want.hist), (what, got.hist[:, :3])
    assert same_bits(got.x, want.x), what


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_exact_cases_give_the_table(case):
    for tail in (False, True):
        csr, b = case.system(tail)
        assert 1000 <= len(b) <= 4097 and len(b) % 2 == int(tail)
        assert ce.DOT(b, b) == (0.0 if case.name == "zero" else 1024.0)
        for kmax in case.kmaxes():
            want = case.want(tail, kmax)
            for dot in ce.ORDERS:
                got = ce.reference(csr, b, case.shifts, kmax, case.rtol, dot=dot)
                _equal(got, want, (case.id, tail, kmax, dot.__name__))
        want = case.want(tail)
        for s, sigma in enumerate(case.shifts):
            exact = same_bits(ce.shifted_spmv(csr, sigma, want.x[s]), b)
            if case.name != "zero":
                assert exact == (case.solved and case.its[s] == case.k), case.id


def test_the_rows_reach_the_exits_they_are_for():
    assert sorted((c.k, c.status) for c in EXACT) == \
        [(0, 0), (0, 1), (0, 1), (1, 0), (1, 0), (1, 0), (1, 1), (2, 0)]
    assert ce.search_early() == ce.EARLY
    e = BY_NAME["early"]
    assert e.its == [2, 1] and e.rtol > 0.0  # one stops, the other goes on
    assert len(BY_NAME["two_i_ns1"].shifts) == 1
    assert len(BY_NAME["two_i_ns8"].shifts) == cc.MAX_NS
    # a status-1 row at kmax = its k: the breakdown is not found
    for name in ("curv1", "curv2", "negative"):
        c = BY_NAME[name]
        assert c.want(True, c.k).status == 0 and c.want(True).status == 1
    assert np.any(BY_NAME["curv2"].xblocks[0])  # X is the iterate of k = 1


def test_the_two_rank_cases_are_cut_inside_a_block():
    import oracle
    for name in ce.TWO_RANKS:
        c = BY_NAME[name]
        N = len(c.system(True)[1])
        cut = int(oracle.owner_ranges(2, N)[1])
        assert 0 < cut < N - 1 and cut % len(c.block) != 0, (name, cut)


@pytest.mark.parametrize("s", ce.FLOOR_S)
@pytest.mark.parametrize("name", ce.FLOOR_CASES)
def test_floor_cases_give_the_table(name, s):
    for tail in (False, True):
        csr, b, shifts, want = ce.floor_case(BY_NAME[name], s, tail)
        for dot in ce.ORDERS:
            _equal(ce.reference(csr, b, shifts, ce.KMAX, 0.0, dot=dot), want,
                   (name, s, tail, dot.__name__))


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("sym", ce.STORAGES)
def test_poisoned_outcomes(sym, kind):
    k, status, h0, x_nan = ce.POISON_OUTCOME[kind]
    runs = [ce.poisoned_reference(sym, kind, dot=dot) for dot in ce.ORDERS]
    got, what = runs[0], (sym, kind)
    bits = got.same(runs[1]) and got.same(runs[2])
    print(sym, kind, "k", got.k, got.its, "status", got.status, "bits", bits)
    assert bits == (what not in ce.WEAK), what
    assert ce.pattern(got) == ce.pattern(runs[1]) == ce.pattern(runs[2]), what
    assert (got.k, got.status) == (k, status), what
    col0 = got.hist[:, 0]
    if h0 == "nan":
        assert np.all(np.isnan(col0))
    elif h0 == "finite":
        assert np.all(np.isfinite(col0)) and np.all(col0 > 0)
    else:
        assert np.all(col0 == (np.inf if h0 == "inf" else h0))
    if x_nan is None:
        assert np.all(np.isfinite(got.x)) and got.its == [ce.POISON_KMAX, 1]
        # the shift froze at once with x = b / sigma to a rounding or two (a *
        # rhon = 1e-300) and did not disturb the other
        b1 = ce.poisoned_case(kind)[1]
        assert np.all(np.abs(got.x[1] / (b1 * 1e-300) - 1.0) <= 2.0 ** -50)
        assert got.hist[1, 1] < 1e-290 and np.all(got.hist[1, 2:] == -1.0)
        csr, b, _ = ce.poisoned_case(kind)
        alone = ce.reference(csr, b, (0.0,), ce.POISON_KMAX, ce.POISON_RTOL,
                             symmetric=sym)
        assert same_bits(got.x[0], alone.x[0])
        assert same_bits(got.hist[0], alone.hist[0])
    else:
        assert np.all(np.isnan(got.x)) if x_nan else \
            same_bits(got.x, np.zeros(got.x.shape)), what


def test_the_weak_share():
    combos = [(sym, kind) for sym in ce.STORAGES for kind in ce.KINDS]
    assert ce.WEAK <= set(combos) and 4 * len(ce.WEAK) <= len(combos)


# ---- d. scaled and negated systems ------------------------------------------------------------
def _healthy(a, b):
    for v in (a, b):
        assert np.all(np.isfinite(v))
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), nz.min()
    assert np.array_equal(a == 0, b == 0)


def _run(sym, s=0, t=0, sign_a=1.0, sign_b=1.0):
    csr = ce.csr_of()
    b = ce.scaled_rhs(csr)
    rec = []
    got = ce.reference(ce.scale_csr(csr, s, sign_a), sign_b * np.ldexp(b, t),
                       tuple(np.ldexp(ce.POISON_SHIFTS, s)), ce.SCALED_KMAX,
                       ce.SCALED_RTOL, record=rec, symmetric=sym)
    return got, rec


def scaled_hist(hist, t):
    return np.where(hist < 0, hist, np.ldexp(hist, t))


@pytest.mark.parametrize("sym", ce.STORAGES)
def test_scaling_relations_hold_on_the_reference(sym):
    base, rec0 = _run(sym)
    assert 1 < base.k <= ce.SCALED_KMAX and base.status == 0
    assert len(set(base.its)) == 3  # the shifts stop at different steps
    for s, t, sb in [(s, t, 1.0) for s, t in ce.PAIRS] + [(0, 0, -1.0)]:
        got, rec = _run(sym, s, t, sign_b=sb)
        assert (got.k, got.its, got.status) == (base.k, base.its, 0)
        assert same_bits(got.x, sb * np.ldexp(base.x, t - s))
        assert same_bits(got.hist, scaled_hist(base.hist, t))
        assert len(rec) == len(rec0) > 0
        for u, v in zip(rec0, rec):
            _healthy(u, v)
    # the pair that is dropped: the reference itself leaves the relation
    got, _ = _run(sym, -400, -300)
    assert not same_bits(got.x, np.ldexp(base.x, 100))
    # (-A, b): the status-1 case
    got, _ = _run(sym, sign_a=-1.0)
    assert (got.k, got.status) == (0, 1) and not got.x.any()


# ---- mutants: the reference's own source with one line replaced -----------------------------------
MUTANTS = {
    # `not pq > 0` as `pq <= 0`: a NaN goes on
    "pq_le": ("if not pq > 0.0:", "if pq <= 0.0:"),
    # the rrn == 0 stop dropped: the next step finds pq == 0, status 1
    "no_rrn0": ("if rrn == 0.0:", "if False:"),
    # the rtol test true on a NaN
    "stop_not_ge": ("if hist[s, k] / hist[s, 0] < rtol:",
                    "if not hist[s, k] / hist[s, 0] >= rtol:"),
    # a stopped shift still moves its direction and is kept active
    "no_freeze": ("                continue\n", "                pass\n"),
}


def _mutant(name):
    src = inspect.getsource(cc._cgs_ref)
    if name is not None:
        old, new = MUTANTS[name]
        assert src.count(old) == 1, (name, src.count(old))
        src = src.replace(old, new)
    ns = dict(vars(cc))
    exec(src, ns)
    inner = ns["_cgs_ref"]

    def ref(spmv, dot, b, shifts, kmax, rtol):
        with np.errstate(all="ignore"):
            return inner(spmv, dot, b, shifts, kmax, rtol)
    return ref


_WANT = {}


@pytest.fixture(scope="module")
def poison_want():
    for sym in ce.STORAGES:
        for kind in ce.KINDS:
            _WANT[(sym, kind)] = ce.poisoned_reference(sym, kind)
    return _WANT


def _failures(ref):
    bad = []
    for case in EXACT:
        csr, b = case.system(True)
        for kmax in case.kmaxes():
            got = ce.reference(csr, b, case.shifts, kmax, case.rtol, ref=ref)
            if not got.same(case.want(True, kmax)):
                bad.append((case.id, kmax))
    for name in ce.FLOOR_CASES:
        for s in ce.FLOOR_S:
            csr, b, shifts, want = ce.floor_case(BY_NAME[name], s, True)
            if not ce.reference(csr, b, shifts, ce.KMAX, 0.0, ref=ref).same(want):
                bad.append((name, s))
    for key, want in _WANT.items():
        got = ce.poisoned_reference(*key, ref=ref)
        ok = got.same(want) if key not in ce.WEAK else \
            ce.pattern(got) == ce.pattern(want)
        if not ok:
            bad.append(key)
    return bad


def test_the_unpatched_source_is_the_reference(poison_want):
    assert _failures(cc.cgs_ref) == [] and _failures(_mutant(None)) == []


@pytest.mark.parametrize("mutant,caught_by", [
    ("pq_le", (False, "b_nan")),
    ("no_rrn0", ("two_i", ce.KMAX)),
    ("stop_not_ge", (True, "b_huge")),
    ("no_freeze", ("early", ce.KMAX)),
])
def test_mutants_of_the_reference_fail(poison_want, mutant, caught_by):
    bad = _failures(_mutant(mutant))
    print(mutant, "fails", bad)
    assert caught_by in bad
