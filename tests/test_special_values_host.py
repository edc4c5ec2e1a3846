"""CPU checks of tests/special_values.py, on every pattern that
test_gpu_special_values.py uses: the numpy restatement equals the oracle, each
recipe S1 ... S5 reaches its target in the reference (so the GPU comparisons
are not vacuous), and the oracle's own C loop agrees with the restatement on
S1, S4 and S5."""
import numpy as np
import pytest

import oracle
import special_values as sv

NAMES = sorted(sv.patterns())


def _oracle(p, va, diag, x, alpha, beta, y0):
    if p.sym:
        return oracle.csr_spmv_sym(p.rp, p.ci, va, diag, x, alpha, beta, y0)
    return oracle.csr_spmv(p.rp, p.ci, va, x, alpha, beta, y0)


def _ref(p, va, diag, x, alpha, beta, y0, dtype):
    if p.sym:
        return sv.ref_spmv_sym(p.rp, p.ci, va, diag, x, alpha, beta, y0, dtype)
    return sv.ref_spmv(p.rp, p.ci, va, x, alpha, beta, y0, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_oracle_on_finite_data(name, dtype):
    p = sv.patterns()[name]
    rng = np.random.default_rng(len(p.ci))
    va = rng.uniform(-1, 1, len(p.ci)).astype(dtype)
    diag = rng.uniform(-1, 1, p.N).astype(dtype) if p.sym else None
    x = rng.uniform(-1, 1, p.ncols).astype(dtype)
    y0 = rng.uniform(-1, 1, p.N).astype(dtype)
    for alpha, beta in ((2.0, 1.0), (1.0, -0.25), (-0.5, 1.5)):
        assert sv.same_bits(_ref(p, va, diag, x, alpha, beta, y0, dtype),
                            _oracle(p, va, diag, x, alpha, beta, y0)), (alpha, beta)
    for alpha in (1.0, -0.5):  # beta == 0: the bits differ only at a zero
        got = _ref(p, va, diag, x, alpha, 0.0, y0, dtype)
        want = _oracle(p, va, diag, x, alpha, 0.0, None)
        assert np.array_equal(got, want), alpha
        diff = sv.bits(got) != sv.bits(want)
        assert (want[diff] == 0).all()


def test_same_bits_sees_signs_and_nan_classes():
    a = np.array([0.0, np.inf, np.nan, 1.0])
    assert sv.same_bits(a, a.copy())
    assert sv.same_bits(a, np.array([0.0, np.inf, -np.nan, 1.0]))
    assert not sv.same_bits(a, np.array([-0.0, np.inf, np.nan, 1.0]))
    assert not sv.same_bits(a, np.array([0.0, -np.inf, np.nan, 1.0]))
    assert not sv.same_bits(a, np.array([0.0, np.inf, 2.0, 1.0]))
    assert not sv.same_bits(a, np.array([0.0, np.inf, np.nan, np.nan]))
    assert not sv.same_bits(a.astype(np.float32), a)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_recipes_hit_their_targets(name, dtype):
    p = sv.patterns()[name]
    # S1 / S2
    d1, d2 = p.data("S1", dtype), p.data("S2", dtype)
    y1 = {ab: p.ref(d1, *ab) for ab in d1.ab}
    y2 = {ab: p.ref(d2, *ab) for ab in d2.ab}
    for ab in d1.ab:
        c1, c2 = sv.classes(y1[ab]), sv.classes(y2[ab])
        assert (c1 == 3).any() and (c1 == 1).any() and (c1 == 2).any(), (name, ab)
        assert (c1 == 0).sum() * 2 >= p.N and (c2 == 0).sum() * 2 >= p.N, (name, ab)
        # NaN only because of a stored zero: that row has no NaN in S1 (its
        # entry under the Inf column makes it +-Inf there)
        assert ((c2 == 3) & (c1 != 3)).any(), (name, ab)
    # S3
    d3 = p.data("S3", dtype)
    y3 = {ab: p.ref(d3, *ab) for ab in d3.ab}
    zeros = np.concatenate([y3[ab] for ab in d3.ab if ab[1] == 0])
    assert (zeros == 0).all()
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any(), name
    if p.sym:
        assert np.signbit(y3[(1.0, 0.0)]).any(), name
    # S4
    d4 = p.data("S4", dtype)
    y4 = p.ref(d4, 1.0, 0.0)
    c4 = sv.classes(y4)
    assert (c4 == 1).any() and ((c4 == 2) | (c4 == 3)).any() and (c4 == 0).any(), name
    rci, rva = sv.reversed_rows(p.rp, p.ci, d4.va)
    if p.sym:
        yr = sv.ref_spmv_sym(p.rp, rci, rva, d4.diag, d4.x, 1.0, 0.0, d4.y0, dtype)
    else:
        yr = sv.ref_spmv(p.rp, rci, rva, d4.x, 1.0, 0.0, d4.y0, dtype)
    assert (sv.classes(yr) != c4).any(), name
    # S5
    d5 = p.data("S5", dtype)
    y5 = p.ref(d5, 1.0, 0.0)
    assert sv.subnormal(y5).sum() * 4 >= p.N, (name, sv.subnormal(y5).mean())
    if not p.sym and dtype == np.float64:
        dm = p.data("S5m")
        assert dm.va.dtype == np.float32
        assert sv.subnormal(dm.va).sum() * 4 >= len(dm.va)
        ym = sv.ref_spmv(p.rp, p.ci, dm.va.astype(np.float64), dm.x, 1.0, 0.0,
                         dm.y0, np.float64)
        assert np.isfinite(ym).all() and (ym != 0).sum() * 2 >= p.N


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_on_special_values(name, dtype):
    """The C loop itself on S1 (beta != 0), S4 and S5."""
    p = sv.patterns()[name]
    for recipe in ("S1", "S4", "S5"):
        d = p.data(recipe, dtype)
        for alpha, beta in d.ab:
            if beta == 0 and recipe == "S1":
                continue
            want = _oracle(p, d.va, d.diag, d.x, alpha, beta,
                           None if beta == 0 else d.y0)
            got = p.ref(d, alpha, beta)
            if beta == 0:  # `+ 0 * out`: only the sign of a zero may differ
                assert np.array_equal(sv.classes(got), sv.classes(want))
                ok = ~np.isnan(want)
                assert np.array_equal(got[ok], want[ok]), (name, recipe)
            else:
                assert sv.same_bits(got, want), (name, recipe, alpha, beta)


@pytest.mark.parametrize("name", [n for n in NAMES if sv.patterns()[n].ncols
                                  >= sv.patterns()[n].N + 3])
def test_ghost_recipes_hit_their_targets(name):
    """G0: a finite dot; G1: x[:N] finite and the dot NaN -- through y alone;
    G2: the dot is the infinity of alpha's sign."""
    p = sv.patterns()[name]
    for recipe, check in (("G0", np.isfinite), ("G1", np.isnan), ("G2", np.isinf)):
        d = p.data(recipe)
        assert np.isfinite(d.x[:p.N]).all()
        assert sv.same_bits(p.ref(d, 2.0, 1.0),
                            _oracle(p, d.va, d.diag, d.x, 2.0, 1.0, d.y0)), recipe
        for alpha, beta in d.ab:
            y = p.ref(d, alpha, beta)
            w = sv.want_dot(d, p.N, y)
            assert check(w), (recipe, alpha, w)
            if recipe == "G2":
                assert np.sign(w) == np.sign(alpha)
                assert (np.isinf(y)).any() and not np.isnan(y).any()
            if recipe == "G1":
                assert np.isnan(y).any() and np.isfinite(y).sum() * 2 >= p.N
