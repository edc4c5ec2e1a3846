"""The cases of idrs_edges.py do what they claim, on idrs_cases.idrs_ref alone
(no GPU): the exact table and the scaling floor under three summation orders,
the poisoned outcomes and the WEAK share, the scaling and negation relations
with every operand recorded, and mutants of the reference (its own source with
ONE line replaced) that the tables tell from it."""
import inspect

import numpy as np
import pytest

import idrs_cases as ic
import idrs_edges as ie
import oracle
from idrs_edges import same_bits

LO, HI = 2.0 ** -900, 2.0 ** 1000


def _equal(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == got.k + 1, what
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.x, want.x), what


@pytest.mark.parametrize("key", sorted(ie.TABLE), ids=str)
def test_exact_cases_give_the_table(key):
    name, s, kmax = key
    for tail in (False, True):
        csr, b = ie.system(name, tail)
        assert 1000 <= len(b) <= 4097 and len(b) % 2 == int(tail)
        want = ie.want(key, tail)
        for dot in ie.ORDERS:
            _equal(ie.reference(csr, b, s, kmax, 0.0, dot=dot), want,
                   (key, tail, dot.__name__))
        if b.any():
            solved = same_bits(oracle.csr_spmv(*csr, want.x), b)
            assert solved == (key in ie.SOLVED), key


def test_the_rows_reach_the_exits_they_are_for():
    T = ie.TABLE
    P = ic.shadow_signs(0, 2048, 1)[0]
    b = ie.system("q0", False)[1]
    assert P @ b == 0.0 and b @ b == 1024.0  # p_0 . b == 0 on thousands of rows
    assert P[:1024] @ ie.system("two_i", False)[1] != 0.0
    for s in (1, 2, 4, 8):
        assert T["q0", s, ie.KMAX][:2] == (0, 1)            # status 1 at q = 0
        assert T["two_i", s, 1][:2] == (1, 0)               # kmax inside a cycle
        assert T["perm", s, 2][:2] == (2, 0)
    assert [T["two_i", s, ie.KMAX][1] for s in (1, 2, 4, 8)] == [2, 1, 1, 1]
    assert T["perm", 1, 2][:2] == (2, 0) and T["perm", 1, ie.KMAX][:2] == (2, 1)
    # skew at s = 1: tt > 0, t.r == 0, and om is NaN (not zero) by the kappa rule
    csr, b = ie.system("skew", True)
    rec = []
    ie.reference(csr, b, 1, ie.KMAX, 0.0, record=rec)
    scalars = [float(a[0]) for a in rec if a.shape == (1,)]
    tr, tt = scalars[-2], scalars[-1]
    assert tr == 0.0 and tt > 0.0
    st = ic.new_state(1, 0.0, ie.KMAX)
    st["rr"] = 512.0
    ic.idrs_omega(st, tr, tt)
    assert st["status"] == 2
    # two_i at s = 1: the first branch
    csr, b = ie.system("two_i", True)
    rec = []
    ie.reference(csr, b, 1, ie.KMAX, 0.0, record=rec)
    assert float(rec[-1][0]) == 0.0  # tt == 0


def test_the_two_rank_cases_are_cut_inside_a_block():
    for name, s in ie.TWO_RANKS:
        N = len(ie.system(name, True)[1])
        cut = int(oracle.owner_ranges(2, N)[1])
        assert 0 < cut < N - 1 and cut % 2 != 0, (name, cut)


@pytest.mark.parametrize("pre", ie.PRES)
@pytest.mark.parametrize("scale", ie.FLOOR_S)
@pytest.mark.parametrize("name,s", ie.FLOOR_CASES)
def test_floor_cases_give_the_table(name, s, scale, pre):
    for tail in (False, True):
        csr, b, dinv, want = ie.floor_case(name, s, scale, pre, tail)
        for dot in ie.ORDERS:
            _equal(ie.reference(csr, b, s, ie.KMAX, 0.0, dinv=dinv, dot=dot),
                   want, (name, s, scale, pre, tail, dot.__name__))


@pytest.mark.parametrize("combo", ie.poison_combos(), ids=str)
def test_poisoned_outcomes(combo):
    shape, kind, s, pre = combo
    k, status, h0, x_zero = ie.POISON_OUTCOME[kind]
    runs = [ie.poisoned_reference(*combo, dot=dot) for dot in ie.ORDERS]
    got = runs[0]
    bits = got.same(runs[1]) and got.same(runs[2])
    assert bits == (combo not in ie.WEAK), combo
    assert ie.pattern(got) == ie.pattern(runs[1]) == ie.pattern(runs[2]), combo
    assert (got.k, got.status) == (s if k is None else k, status), combo
    assert len(got.hist) == got.k + 1
    if h0 == "nan":
        assert np.isnan(got.hist[0])
    elif h0 == "finite":
        assert np.isfinite(got.hist[0]) and got.hist[0] > 0
    else:
        assert got.hist[0] == (np.inf if h0 == "inf" else h0)
    if x_zero:
        assert same_bits(got.x, np.zeros(len(got.x)))
    else:
        assert np.all(np.isfinite(got.x)) and got.x.any()
        assert np.all(np.isinf(got.hist))


def test_the_weak_share():
    combos = ie.poison_combos()
    assert len(combos) == 48 and ie.WEAK <= set(combos)
    assert 4 * len(ie.WEAK) <= len(combos)


# ---- d. scaled and negated systems ------------------------------------------------------------
def _healthy(a, b):
    for v in (a, b):
        assert np.all(np.isfinite(v))
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), nz.min()
    assert np.array_equal(a == 0, b == 0)


def _run(shape, pre, s, sc=0, t=0, sign_a=1.0, sign_b=1.0):
    rec = []
    got = ie.reference(ie.scale_csr(ie.csr_of(shape), sc, sign_a),
                       sign_b * np.ldexp(ie.scaled_rhs(shape), t), s,
                       ie.SCALED_KMAX, ie.SCALED_RTOL,
                       minv=ie.minv_of(pre, shape, sc), record=rec)
    return got, rec


@pytest.mark.parametrize("s", ie.SCALED_S)
@pytest.mark.parametrize("shape,pre", [(sh, p) for sh, ps in ie.SCALED.items()
                                       for p in ps])
def test_scaling_relations_hold_on_the_reference(shape, pre, s):
    base, rec0 = _run(shape, pre, s)
    assert 1 < base.k <= ie.SCALED_KMAX and base.status == 0
    runs = [(sc, t, 1.0, 1.0) for sc, t in ie.pairs(pre) + (ie.ODD_PAIR,)]
    runs.append((0, 0, 1.0, -1.0))
    if pre in ie.NEGATED_A:
        runs.append((0, 0, -1.0, 1.0))
    for sc, t, sa, sb in runs:
        got, rec = _run(shape, pre, s, sc, t, sa, sb)
        assert (got.k, got.status) == (base.k, base.status), (sc, t, sa, sb)
        assert same_bits(got.x, sa * sb * np.ldexp(base.x, t - sc))
        assert same_bits(got.hist, np.ldexp(base.hist, t))
        assert len(rec) == len(rec0) > 0
        if pre in ("none", "dinv"):  # (the others multiply inside B^-1 too)
            for u, v in zip(rec0, rec):
                _healthy(u, v)
    if pre == "none":  # the dropped pair: the reference leaves the relation
        got, _ = _run(shape, pre, s, *ie.PAIRS[-1])
        assert not same_bits(got.x, np.ldexp(base.x, 100))


# ---- mutants: the reference's own source with one line replaced -----------------------------------
PIV = "if M[q][q] == 0.0 or not math.isfinite(M[q][q]):"
OM = "if om == 0.0 or not math.isfinite(om):"
MUTANTS = {
    # `== 0` as `<= 0`: a negative pivot ends the solve
    "piv_le": (PIV, "if M[q][q] <= 0.0 or not math.isfinite(M[q][q]):"),
    # the pivot's finiteness is not tested: be = f / NaN goes on
    "piv_finite": (PIV, "if M[q][q] == 0.0:"),
    # om's finiteness is not tested: the NaN of the kappa rule goes on
    "om_finite": (OM, "if om == 0.0:"),
    # the stop test true on a NaN
    "stop_not_ge": ("return _div(hist[k], hist[0]) < rtol or k == kmax",
                    "return not _div(hist[k], hist[0]) >= rtol or k == kmax"),
    # the pivot test moved behind the division it guards and the updates
    "piv_late": (PIV, "if False:"),
}


def _mutant(name):
    src = inspect.getsource(ic._idrs_ref)
    if name is not None:
        old, new = MUTANTS[name]
        assert src.count(old) == 1, (name, src.count(old))
        src = src.replace(old, new)
    ns = dict(vars(ic))
    exec(src, ns)
    inner = ns["_idrs_ref"]

    def ref(spmv, dot, minv, b, s, kmax, rtol, kappa=ic.KAPPA, seed=0, row0=0):
        with np.errstate(all="ignore"):
            return inner(spmv, dot, minv, b, s, kmax, rtol, kappa, seed, row0)
    return ref


_WANT = {}


@pytest.fixture(scope="module")
def poison_want():
    for c in ie.poison_combos():
        _WANT[c] = ie.poisoned_reference(*c)
    return _WANT


def _failures(ref):
    bad = []
    for key in sorted(ie.TABLE):
        name, s, kmax = key
        csr, b = ie.system(name, True)
        got = ie.reference(csr, b, s, kmax, 0.0, ref=ref)
        if not (got.same(ie.want(key, True)) and len(got.hist) == got.k + 1):
            bad.append(key)
    for name, s in ie.FLOOR_CASES:
        for scale in ie.FLOOR_S:
            for pre in ie.PRES:
                csr, b, dinv, want = ie.floor_case(name, s, scale, pre, True)
                got = ie.reference(csr, b, s, ie.KMAX, 0.0, dinv=dinv, ref=ref)
                if not got.same(want):
                    bad.append((name, s, scale, pre))
    for c, want in _WANT.items():
        got = ie.poisoned_reference(*c, ref=ref)
        ok = got.same(want) if c not in ie.WEAK else \
            ie.pattern(got) == ie.pattern(want)
        if not ok:
            bad.append(c)
    return bad


def test_the_unpatched_source_is_the_reference(poison_want):
    assert _failures(ic.idrs_ref) == [] and _failures(_mutant(None)) == []


@pytest.mark.parametrize("mutant,caught_by", [
    ("piv_le", ("skew", 1, ie.KMAX)),
    ("piv_finite", ("convdiff8", "b_nan", 1, "none")),
    ("om_finite", ("skew", 1, ie.KMAX)),
    ("stop_not_ge", ("cdpe10", "b_huge", 4, "dinv")),
    ("piv_late", ("q0", 4, ie.KMAX)),
])
def test_mutants_of_the_reference_fail(poison_want, mutant, caught_by):
    bad = _failures(_mutant(mutant))
    print(mutant, "fails", bad)
    assert caught_by in bad
