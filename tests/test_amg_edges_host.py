"""amg_edges.py held to its claims on the restatement alone (no GPU): the
scaling relations hold bit for bit on amg_cases.AmgRef with every operand finite
and normal, the bad-bound matrices pass the diagonal test and are refused for
their bound, and the NaN pair leaves a finite bound."""
import numpy as np
import pytest

import amg_edges as ae
import solver_edges as se
import test_gpu_amg as ta
from special_values import same_bits

_BASE = {}


def _base(name, symmetric):
    key = (name, symmetric)
    if key not in _BASE:
        csr = ae.csr_of(name)
        n = len(csr[0]) - 1
        _BASE[key] = (csr, n, ta.restate(csr, n, symmetric, **ae.OPTIONS))
    return _BASE[key]


def test_the_large_pair_is_larger():
    s, t = ae.LARGE
    assert abs(s) > 100 and abs(t) > 200 and ae.LARGE in ae.PAIRS
    assert set(se.SCALES) <= set(ae.PAIRS)
    assert max(abs(2 * t), abs(2 * t - s), abs(t - s)) < 900


@pytest.mark.parametrize("name", ae.MATRICES)
def test_scaling_relations_on_the_restatement(name):
    for sym in ae.storages(name):
        csr, n, ref = _base(name, sym)
        assert len(ref.levels) >= 3 or name != "poisson11"
        r = ae.clean_rhs(csr)
        z = ref.apply(r)
        record = ae.recorded(ref)
        assert same_bits(ref.apply(r), z)  # recording changes nothing
        record += [r, z]
        for s, t in ae.PAIRS:
            got = ta.restate(se.scale_csr(csr, s), n, sym, **ae.OPTIONS)
            assert len(got.levels) == len(ref.levels), (name, sym, s)
            for a, b in zip(got.levels, ref.levels):
                assert a["lmax"] == b["lmax"], (name, sym, s)
                assert same_bits(a["csr"][2], np.ldexp(b["csr"][2], s))
                assert same_bits(a["dinv"], np.ldexp(b["dinv"], -s))
                assert ("step" in a) == ("step" in b)
                if "step" in a:
                    assert np.array_equal(a["step"]["agg"], b["step"]["agg"])
            rec2 = ae.recorded(got)
            zs = got.apply(np.ldexp(r, t))
            assert same_bits(zs, np.ldexp(z, t - s)), (name, sym, s, t)
            assert ae.all_normal(rec2 + [zs, np.ldexp(r, t)]), (name, sym, s, t)
        assert ae.all_normal(record), (name, sym)


def test_poisons_cover_every_value_and_row():
    full = ae.poisons(100)
    assert len(full) == 12 and {r for _, r in full} == {0, 50, 99}
    few = ae.poisons(100, few=True)
    assert len(few) == 4 and {r for _, r in few} == {0, 50, 99}
    for some in (full, few):
        vals = [v for v, _ in some]
        assert any(np.isnan(v) for v in vals) and np.inf in vals \
            and -np.inf in vals and 1e300 in vals
    r = ae.poisoned(np.ones(5), np.nan, 4)
    assert np.isnan(r[4]) and np.all(r[:4] == 1.0)


def test_bad_bounds_pass_the_diagonal_test_and_are_refused_for_the_bound():
    csr, n, _ = _base("poisson11", False)
    for make in (ae.tiny_diagonal, ae.huge_pairs):
        bad = make(csr)
        d = ae.diag_of(bad)
        assert np.all(np.isfinite(bad[2])) and np.all(d > 0.0), make.__name__
        for sym in (False, True):
            with np.errstate(all="ignore"):
                with pytest.raises(ValueError, match="row-sum bound"):
                    ta.restate(bad, n, sym, **ae.OPTIONS)
    assert ae.diag_of(ae.tiny_diagonal(csr)).min() == 1e-310
    huge = ae.huge_pairs(csr)
    assert np.sum(huge[2] == 1e308) == 4
    assert np.sum(huge[2][ae.row_of(huge) == 665] == 1e308) == 2


def test_a_nan_far_from_the_diagonal_leaves_a_finite_bound():
    csr, n, ref = _base("poisson11", False)
    bad, i = ae.nan_far(csr, ref)
    assert np.sum(np.isnan(bad[2])) == 2
    for sym in (False, True):
        with np.errstate(all="ignore"):
            got = ta.restate(bad, n, sym, frozen=_base("poisson11", sym)[2],
                             **ae.OPTIONS)
            assert all(np.isfinite(L["lmax"]) and L["lmax"] > 0
                       for L in got.levels)
            assert np.any(np.isnan(got.levels[1]["csr"][2]))
            z = got.apply(ae.clean_rhs(csr))
        assert np.any(np.isnan(z))
