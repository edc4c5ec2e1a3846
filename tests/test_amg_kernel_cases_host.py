"""amg_kernel_cases.py held to its claims on the CPU alone: every generated step
passes the rules of amg_is_sound; the kernel restatements and amg_cases.AmgRef
reproduce each other on the steps of a real hierarchy; and every edge that
test_gpu_amg_kernels.py relies on is present in the case that is said to hold
it."""
import numpy as np
import pytest

import amg_cases as ac
import amg_kernel_cases as kc
import gmres_cases as gc
import test_gpu_amg as ta
import test_gpu_pcg as tp
from special_values import same_bits

CUS = 256  # the wrap cases are sized from the device; any count shows soundness


def _steps():
    for c in kc.galerkin_cases() + [kc.galerkin_wrap(CUS)]:
        yield "galerkin " + c.name, c.step
    for c in kc.restrict_cases() + [kc.restrict_wrap(CUS)]:
        yield "restrict " + c.name, c.step
    for c in kc.diag_cases():
        if c.form == "xrow":
            yield c.name, c.step
    for n in kc.STREAM_SIZES + (kc.stream_wrap(CUS),):
        yield f"prolong {n}", kc.prolong_case(n)[0]


def test_every_generated_step_is_sound():
    count = 0
    for name, step in _steps():
        assert kc.is_sound(step), name
        count += 1
    assert count > 30


def test_the_restated_rules_refuse_what_plan_create_refuses():
    """the corruptions of test_gpu_amg's plan test, on its hand-built step"""
    good = kc.make_step([0, 0, 1, 2, 1], [3, 2, 3, 2],
                        [0, 1, ~0, 2, 3, 4, ~2, 5, 8, ~4], 9, 5,
                        xrow_ptr=[0, 2, 4, 6, 8, 10],
                        xrow_src=[0, ~0, 1, ~1, 2, ~2, 3, ~3, 4, ~4])
    assert kc.is_sound(good)

    def corrupt(key, index, value):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v)
               for k, v in good.items()}
        bad[key][index] = value
        return bad
    for key, index, value in (("agg", 2, 3), ("agg", 0, -1), ("agg", 4, 2),
                              ("member", 4, 5), ("member", 1, 0),
                              ("member_ptr", 1, 5), ("member_ptr", 0, 1),
                              ("member_ptr", 3, 4), ("src", 3, 9), ("src", 2, ~5),
                              ("src_ptr", 2, 2), ("src_ptr", 0, 1),
                              ("xrow_src", 0, 9), ("xrow_ptr", 2, 1)):
        assert not kc.is_sound(corrupt(key, index, value)), (key, index, value)
    swapped = dict(good, member=np.array([1, 0, 2, 4, 3], np.int32))
    assert not kc.is_sound(swapped)
    for key, value in (("coarse_rows", 6), ("num_diagonal", 4), ("num_values", 8),
                       ("fine_rows", -1)):
        assert not kc.is_sound(dict(good, **{key: value})), key


@pytest.mark.parametrize("symmetric", [False, True])
def test_kernel_restatements_and_amgref_agree(symmetric):
    """Poisson 11^3, three levels: the coarse values, d, dinv and lmax of every
    level from the kernel restatements; with one smoothing step the cycle of
    level 0 is pre-smoother, restrict, the coarse cycle, prolong and post0, and
    assembled from the kernel restatements it must be AmgRef.apply."""
    csr = tp._csr("poisson11")
    n = len(csr[0]) - 1
    ref = ta.restate(csr, n, symmetric, min_coarse_rows=20, smooth_degree=1,
                     coarse_scale=1.6)
    assert len(ref.levels) >= 3
    sym, diag = symmetric, None
    for l, L in enumerate(ref.levels):
        rp, ci, va = L["csr"]
        rows = L["n"]
        if sym:
            diag = L["d"]
            ptr, _, src = ac.expand(rp, ci, rows, True)
            got = kc.diag_ref(rows, va, xrow_ptr=ptr, xrow_src=src, diagonal=diag)
        else:
            got = kc.diag_ref(rows, va, rp, ci, rows)
        assert same_bits(got[0], L["d"]) and same_bits(got[1], L["dinv"]), l
        assert got[2] == 0 and got[3] == L["lmax"], (l, got[3], L["lmax"])
        if "step" in L:
            st = L["step"]
            step = kc.make_step(st["agg"], np.diff(st["src_ptr"]), st["src"],
                                len(va), rows if sym else 0)
            assert kc.is_sound(step), l
            assert np.array_equal(step["member"], st["member"])
            assert np.array_equal(step["member_ptr"], st["member_ptr"])
            coarse = kc.galerkin_ref(step, va, diag)
            assert same_bits(coarse, ref.levels[l + 1]["csr"][2]), l
        sym, diag = False, None
    L = ref.levels[0]
    st = L["step"]
    step = kc.make_step(st["agg"])
    r = ref.levels[0]["spmv"](np.random.default_rng(4).uniform(-1, 1, n))
    _, b = gc.chebyshev_coefficients(1, L["lmin"], L["lmax"])
    z = b[0] * (L["dinv"] * r)  # cheb_apply0, degree 1
    rc = kc.restrict_ref(step, r, L["spmv"](z))
    z = kc.prolong_ref(step, 1.6, ref.cycle(1, rc), z)
    _, z = kc.post0_ref(b[0], L["spmv"](z), r, L["dinv"], z)
    assert same_bits(z, ref.apply(r))
    assert np.all(np.isfinite(z)) and np.any(z != 0.0)


# ---- the edges are where the GPU test expects them -----------------------------------
def test_galerkin_edges_are_present():
    cases = {c.name: c for c in kc.galerkin_cases()}
    lens = np.diff(cases["lengths"].step["src_ptr"])
    assert sorted(lens.tolist()) == [1, 2, 3, 64, 65, kc.LONG] and kc.LONG >= 2000
    assert lens[cases["lengths"].claims["long_list"]] >= 2000
    src = cases["lengths"].step["src"]
    assert np.any(src >= 0) and np.any(src < 0)  # both arrays
    sp = cases["special"]
    out = kc.galerkin_ref(sp.step, sp.values, sp.diagonal)
    zero = out == 0.0
    assert set(np.flatnonzero(zero & np.signbit(out))) \
        == set(sp.claims["negative_zero"])
    assert np.flatnonzero(zero & ~np.signbit(out)).tolist() == [1]
    assert set(np.flatnonzero(np.isnan(out))) == set(sp.claims["nan"])
    assert out[9] == np.inf
    # from 0.0 the lone -0.0 would be +0.0: the mutation has something to hit
    with np.errstate(all="ignore"):
        from0 = ac.seq_sum(sp.step["src_ptr"],
                           ac.values_of(sp.step["src"], sp.values, sp.diagonal),
                           from_zero=True)
    assert not same_bits(from0, out)
    assert [c.step["coarse_nnz"] for c in kc.galerkin_cases()[2:]] \
        == [1, 255, 256, 257]
    wrap = kc.galerkin_wrap(CUS)
    assert wrap.step["coarse_nnz"] == kc.grid_cap(CUS) * 256 + 300
    assert np.diff(wrap.step["src_ptr"]).max() <= 4


def test_diag_edges_are_present():
    cases = kc.diag_cases()
    assert sorted({c.n for c in cases}) == sorted(kc.DIAG_SIZES)
    assert kc.DIAG_SIZES[-1] == 65536 + 257
    seen = {"general": set(), "xrow": set()}
    for c in cases:
        d, dinv, bad, gmax, g = c.ref()
        is_bad = ~np.isfinite(d) | ~(d > 0.0)
        assert bad == c.bad == int(is_bad.sum()), c.name
        assert sorted(c.kinds) == np.flatnonzero(is_bad).tolist(), c.name
        seen[c.form] |= set(c.kinds.values())
        variant = c.name.split("-")[1]
        if variant == "bad":
            want = {r for r in (0, 63, 64, c.n - 1, 65536, 65536 + 63)
                    if 0 <= r < c.n}
            assert want <= set(c.kinds), c.name
            if c.n >= 192:  # one whole wavefront
                assert set(range(128, 192)) <= set(c.kinds), c.name
            if c.n > 65536 + 128:  # ... and one of the second round
                assert set(range(65536 + 64, 65536 + 128)) <= set(c.kinds)
        else:
            # a NaN g beside finite ones, d good; the maximum is finite and
            # sits in the last row (of the last round)
            if c.n >= 63:
                assert len(c.gnan) >= 1, c.name
            assert np.all(np.isnan(g[c.gnan])) and not np.any(is_bad[c.gnan])
            if c.n > 0:
                assert c.max_row == c.n - 1 and np.isfinite(gmax), c.name
                assert g[c.max_row] == gmax, c.name
                others = np.delete(g, c.max_row)
                assert not np.any(others >= gmax), c.name
            if c.n > 65536:
                assert any(r >= 65536 for r in c.gnan), c.name
                assert any(r >= 65536 for r in c.kinds), c.name
            with np.errstate(all="ignore"):
                assert c.n < 63 or np.isnan(np.max(g))  # a plain maximum is lost
        if c.form == "general" and c.n >= 5:
            # ghost columns are there and carry weight: kept, they move g
            assert np.any(c.colind >= c.n)
            full = kc.diag_ref(c.n, c.values, c.rowptr, c.colind, c.cols)
            assert not same_bits(full[4], g), c.name
    assert seen["general"] == set(kc.BAD_KINDS)
    assert seen["xrow"] == set(kc.BAD_DIAGONAL)
    big = [c for c in cases if c.n > 65536 and c.form == "general"][0]
    on = big.colind == np.repeat(np.arange(big.n), np.diff(big.rowptr))
    assert np.bincount(np.repeat(np.arange(big.n), np.diff(big.rowptr))[on],
                       minlength=big.n).max() == 2  # duplicates 1, 2 and 3, -3
    xr = [c for c in cases if c.n == 257 and c.form == "xrow"][0]
    assert len(xr.empty) > 0 and np.all(xr.ref()[4][xr.empty] == 0.0)


def test_restrict_edges_are_present():
    cases = {c.name: c for c in kc.restrict_cases()}
    sizes = np.diff(cases["sizes"].step["member_ptr"])
    assert sorted(sizes.tolist()) == [1, 1, 2, 2, 3, kc.LONG]
    assert sizes[cases["sizes"].claims["long_list"]] >= 2000
    mem = cases["sizes"].step["member"]
    assert np.any(np.diff(mem[:6]) != 1)  # gathered, not contiguous
    sp = cases["special"]
    out = kc.restrict_ref(sp.step, sp.r, sp.w)
    zero = out == 0.0
    assert tuple(np.flatnonzero(zero & ~np.signbit(out))) \
        == sp.claims["positive_zero"]
    assert tuple(np.flatnonzero(zero & np.signbit(out))) \
        == sp.claims["negative_zero"]
    assert tuple(np.flatnonzero(np.isnan(out))) == sp.claims["nan"]
    # r and w added separately differ from the difference first
    c = cases["sizes"]
    with np.errstate(all="ignore"):
        apart = ac.seq_sum(c.step["member_ptr"], c.r[c.step["member"]]) \
            - ac.seq_sum(c.step["member_ptr"], c.w[c.step["member"]])
    assert not same_bits(apart, kc.restrict_ref(c.step, c.r, c.w))
    assert [c.step["coarse_rows"] for c in kc.restrict_cases()[2:]] \
        == [1, 256, 257]
    wrap = kc.restrict_wrap(CUS)
    assert wrap.step["coarse_rows"] > kc.grid_cap(CUS) * 256
    assert np.diff(wrap.step["member_ptr"]).max() <= 2


def test_stream_edges_are_present():
    assert kc.STREAM_SIZES == (1, 2, 3, 2047, 2048, 2049, 4097)
    assert kc.stream_wrap(CUS) == 2 * 8 * CUS * 1024 + 2 * 1024 + 3
    assert set(kc.SCALES) == {1.0, 0.5, 1.6, np.inf, 0.0} \
        and any(s == 0.0 and np.signbit(s) for s in kc.SCALES)
    for n in (3, 2049):
        step, e, z = kc.prolong_case(n)
        for v in (e, z) + kc.post0_case(n):
            if len(v) >= 3:
                assert np.any(np.isnan(v)) or np.any(np.isinf(v)) \
                    or np.any((v == 0.0) & np.signbit(v)), n
        if n == 3:
            continue
        out = kc.prolong_ref(step, -0.0, e, z)
        assert np.any((out == 0.0) & np.signbit(out))  # -0.0 + -0.0 * e
        # the mutants of the issue differ from the restatement here
        with np.errstate(all="ignore"):
            assert not same_bits(np.float64(1.6) * z, kc.prolong_ref(step, 1.6, e, z))
            w, r, dinv, zz = kc.post0_case(n)
            assert not same_bits(zz + 1.6 * (dinv * r - w),
                                 kc.post0_ref(1.6, w, r, dinv, zz)[1])
    vals = np.concatenate([np.concatenate(kc.post0_case(2049)),
                           kc.prolong_case(2049)[1], kc.prolong_case(2049)[2]])
    assert np.any(np.isnan(vals)) and np.any(vals == np.inf) \
        and np.any(vals == -np.inf) and np.any((vals == 0.0) & np.signbit(vals))
