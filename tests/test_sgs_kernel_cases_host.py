"""CPU checks that hold sgs_layout.py and sgs_kernel_cases.py to their claims:

(a) sgs_layout reproduces the arrays of host/ilu0_build.h and host/sgs_build.h
    on the builders' own colourings.  host.ilu0_symbolic returns ptr, cpos,
    src, slot, sliced_col and long_col, compared directly; len, slice_ptr,
    color_slice and color_long are not returned, so they are compared with
    what the builder's slots and color_start say about them (a slot IS
    slice_ptr[s] + 64 k + lane, and a long row is a row of negative slots).
(b) every case reaches the decision points it is named after, and the cases
    together pin every point of sgs_kernel_cases.REQUIRED;
(c) three restatements agree bit for bit on every case and recipe:
    ilu0_cases.Ilu0Ref.apply on the matrix's own values, test_gpu_sgs.Sweeps
    .apply, and sgs_layout.sweep on the sliced arrays (whatever the prefill);
(d) the overflow recipe tells summation orders apart;
(e) the pivot recipe's counts are what the case states, at the lanes it states;
and three deliberately wrong kernels (sgs_layout.sweep's mutants) each differ
from the reference somewhere."""
import numpy as np
import pytest

import ilu0_cases as ic
import sgs_kernel_cases as kc
import sgs_layout as sl
import special_values as sv
import test_ilu0_host as th
from spmv_amd import host
from test_gpu_sgs import Sweeps, ragged_spd


# ---- (a) the layout against the C++ builders ------------------------------------------
def _builder_says(part, color_start):
    """len, slice_ptr (None where a slice holds no entry), color_slice and
    color_long as the builder's ptr, slot and color_start imply them"""
    ptr, slot = part["ptr"], part["slot"]
    n = len(ptr) - 1
    lens = np.diff(ptr)
    first = slot[np.minimum(ptr[:-1], max(len(slot) - 1, 0))] if len(slot) else lens
    is_long = (lens > 0) & (first < 0)
    ln = np.where(is_long, -1, lens)
    color_slice, color_long, slice_ptr = [0], [0], []
    for c in range(len(color_start) - 1):
        c0, c1 = int(color_start[c]), int(color_start[c + 1])
        for p0 in range(c0, c1, 64):
            at = {int(first[p] - (p - p0)) for p in range(p0, min(p0 + 64, c1))
                  if ln[p] > 0}
            assert len(at) <= 1
            slice_ptr.append(at.pop() if at else None)
        color_slice.append(color_slice[-1] + (c1 - c0 + 63) // 64)
        color_long.append(int(np.sum(is_long[:c1])))
    assert n == int(color_start[-1])
    return ln, slice_ptr, color_slice, color_long


def _same_as_builder(csr, what):
    n = len(csr[0]) - 1
    sym = host.ilu0_symbolic(csr[0], csr[1], n)
    colours, nc = host.sgs_color(csr[0], csr[1], n)
    assert np.array_equal(sym["colors"], colours), what
    lay = sl.layout(ic.Ilu0Ref(csr, n, colours, False))
    assert lay["num_colors"] == nc == sym["num_colors"], what
    for key in ("perm", "color_start"):
        assert np.array_equal(lay[key], sym[key]), (what, key)
    for h in ("before", "after"):
        got, want = lay[h], sym[h]
        for key in ("ptr", "cpos", "src", "slot"):
            assert got[key].dtype == want[key].dtype, (what, h, key)
            assert np.array_equal(got[key], want[key]), (what, h, key)
        s = got["sliced"]
        assert np.array_equal(s["col"], want["sliced_col"]), (what, h)
        assert np.array_equal(s["long_col"], want["long_col"]), (what, h)
        ln, slice_ptr, color_slice, color_long = _builder_says(
            want, sym["color_start"])
        assert np.array_equal(s["len"], ln), (what, h, "len")
        assert np.array_equal(s["color_slice"], color_slice), (what, h)
        assert np.array_equal(s["color_long"], color_long), (what, h)
        assert len(s["slice_ptr"]) == len(slice_ptr) + 1, (what, h)
        assert s["slice_ptr"][0] == 0 and s["long_ptr"][0] == 0
        assert s["slice_ptr"][-1] == len(want["sliced_col"]), (what, h)
        assert s["long_ptr"][-1] == len(want["long_col"]), (what, h)
        assert np.all(np.diff(s["slice_ptr"]) % 64 == 0), (what, h)
        for i, at in enumerate(slice_ptr):
            assert at is None or s["slice_ptr"][i] == at, (what, h, i)
        # _sliced, as test_gpu_ilu0.py builds its input from the builder's output
        old = sl._sliced(sym, want)
        for key in sl.SLICED_KEYS:
            a, b = old[key], s[key]
            assert (a is None and len(b) == 0) or np.array_equal(a, b), (what, key)
    return sym


@pytest.mark.parametrize("name", th.NAMES)
def test_layout_equals_the_builders(name):
    sym = _same_as_builder(th._csr(name), name)
    if name == "arrow130":  # a long row
        assert len(sym["before"]["long_col"]) == 129


def test_layout_equals_the_builders_on_the_ragged_matrix():
    sym = _same_as_builder(ragged_spd(), "ragged3001")
    for h in ("before", "after"):  # slices and long rows, both parts
        assert len(sym[h]["long_col"]) > 64 and len(sym[h]["sliced_col"]) > 0


def test_long_threshold_is_a_parameter():
    case = kc.cases()["rows_of_64_65_127_128_129_192"]
    part = case.ref.parts[0]
    for thr, want in ((64, 5), (65, 4), (128, 2), (192, 0)):
        s, slot = sl.slice_part(case.ref.color_start, part["ptr"], part["col"],
                                None, thr)
        assert len(s["long_pos"]) == want == np.sum(s["len"] < 0), thr
        assert np.sum(slot < 0) == s["long_ptr"][-1], thr
    assert sl.LONG_THRESHOLD == 64


# ---- (b) every case reaches what it is named after ----------------------------------
def test_the_case_list_is_the_one_the_gpu_test_runs():
    assert tuple(kc.cases()) == kc.NAMES
    for case in kc.cases().values():
        names = set(case.recipes())
        assert names - {"pivots"} == set(kc.RECIPES), case.name
    assert "pivots" in kc.cases()["pivots_in_785_rows"].recipes()


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_reaches_its_decision_points(name):
    case = kc.cases()[name]
    pts = kc.reached(case)
    assert case.pins and set(case.pins) <= pts, sorted(set(case.pins) - pts)
    assert case.n <= 4000
    # a proper colouring, every colour worn, row 0 alone in its row and last
    B, A = case.ref.parts
    assert np.all(np.diff(case.ref.color_start) > 0)
    assert case.colours[0] == case.ref.nc - 1 and case.rp[1] - case.rp[0] == 1
    assert not np.any(case.ci[~case.on] == 0)
    assert np.any(case.ref.perm != np.arange(case.n))
    # inside a part the columns ascend with the positions: both restatements
    # of (c) add in the same order
    for part in (B, A):
        same_row = np.diff(np.repeat(np.arange(case.n), np.diff(part["ptr"]))) == 0
        assert np.all(np.diff(part["col"])[same_row] > 0), name


def test_every_decision_point_of_the_list_is_pinned():
    pinned = set().union(*(c.pins for c in kc.cases().values()))
    assert set(kc.REQUIRED) <= pinned, sorted(set(kc.REQUIRED) - pinned)


def test_the_layout_arrays_say_so_themselves():
    """the points again, read off the arrays without kc.reached"""
    C = kc.cases()
    lay = C["colour_sizes_1_63_64_65_128_129"].lay
    assert sorted(np.diff(lay["color_start"]).tolist()) == [1, 63, 64, 65, 128, 129]
    case = C["rows_of_64_65_127_128_129_192"]
    for h in ("before", "after"):
        s, lens = case.lay[h]["sliced"], np.diff(case.lay[h]["ptr"])
        assert s["len"].max() == 64
        assert sorted(lens[s["long_pos"]].tolist()) == [65, 127, 128, 129, 192]
        at64, at65 = np.flatnonzero(lens == 64)[0], np.flatnonzero(lens == 65)[0]
        assert at65 == at64 + 1 and s["len"][at65] == -1
    case = C["slice_of_64_long_rows"]
    c0, c1 = case.lay["color_start"][1:3]
    assert c1 - c0 == 64
    for h in ("before", "after"):
        s = case.lay[h]["sliced"]
        i = s["color_slice"][1]
        assert s["color_slice"][2] == i + 1 and s["slice_pos0"][i] == c0
        assert s["slice_ptr"][i + 1] == s["slice_ptr"][i]  # span == 0
        assert np.all(s["len"][c0:c1] == -1)
        assert s["color_long"][2] - s["color_long"][1] == 64
    case = C["factor_rows_of_255_256_257_600"]
    tot = (np.diff(case.lay["before"]["ptr"]) + 1
           + np.diff(case.lay["after"]["ptr"]))
    c0, c1 = case.lay["color_start"][1:3]
    assert tot[c0:c1].tolist() == [255, 256, 257, 600]
    case = C["pivots_in_785_rows"]
    assert case.n == 256 * 3 + 17


# ---- (c) the restatements agree ----------------------------------------------------------
def _sweep_inputs(case, rec):
    l, u, d = case.parts_values(rec.va)
    with np.errstate(all="ignore"):
        dinv = 1.0 / case.diag_of(rec.va)
    return (l, u, d), dinv


@pytest.mark.parametrize("name", kc.NAMES)
def test_restatements_agree(name):
    case = kc.cases()[name]
    for rname, rec in case.recipes().items():
        if not rec.sweep:
            continue
        fac, dinv = _sweep_inputs(case, rec)
        want = case.apply(fac, rec.r)
        with np.errstate(all="ignore"):
            by_column = Sweeps((case.rp, case.ci, rec.va), case.n, case.colours,
                               False).apply(dinv, rec.r)
        assert sv.same_bits(by_column, want), (name, rname, "Sweeps")
        lay = sl.with_values(case.lay, fac[0], fac[1])
        for z0 in (rec.z0, np.full(case.n, np.inf)):
            got = sl.sweep(lay, dinv, rec.r, z0)
            assert sv.same_bits(got, want), (name, rname, "sliced")
        if rname == "benign":
            assert np.all(np.isfinite(want)), name
        if rname == "poison":
            assert np.isinf(want[0]) and not np.all(np.isfinite(want[1:]))
            assert np.any(np.isfinite(want)), name
        if rname == "negzero":
            nb = np.diff(case.ref.parts[0]["ptr"])[case.ref.pos]
            zero = (want == 0.0) & np.signbit(want)
            assert np.any(zero & (nb == 0)), name
        if rname == "subnormal":
            assert np.any(sv.subnormal(dinv)) and np.any(sv.subnormal(rec.va))
            assert np.any(sv.subnormal(want)), name


def test_factor_recipes_are_what_they_say():
    for name, case in kc.cases().items():
        rec = case.recipes()["special"]
        off = rec.va[~case.on]
        assert np.any(sv.subnormal(off)) and np.any(np.isinf(off)), name
        assert np.any((off == 0) & np.signbit(off)), name
        rec = case.recipes()["benign"]
        fac = case.ref.factor(rec.va, case.diag_of(rec.va))
        assert kc.pivot_counts(fac[2]) == (0, 0), name
        assert all(np.all(np.isfinite(f)) for f in fac), name
    # the factor is not the matrix where fill lands
    case = kc.cases()["fill_dropped_everywhere_and_a_row_without_before"]
    rec = case.recipes()["benign"]
    fac = case.ref.factor(rec.va, case.diag_of(rec.va))
    plain = case.parts_values(rec.va)
    assert all(np.any(f != p) for f, p in zip(fac, plain))


# ---- (d) the overflow recipe tells summation orders apart -----------------------------
@pytest.mark.parametrize("name", ["rows_of_64_65_127_128_129_192",
                                  "slice_of_64_long_rows",
                                  "factor_rows_of_255_256_257_600"])
def test_overflow_recipe_distinguishes_orders(name):
    case = kc.cases()[name]
    nc = case.ref.nc
    for rname, h, colour in (("overflow_before", "before", 1),
                             ("overflow_after", "after", nc - 2)):
        rec = case.recipes()[rname]
        fac, dinv = _sweep_inputs(case, rec)
        want = case.apply(fac, rec.r)
        lay = sl.with_values(case.lay, fac[0], fac[1])
        pairwise = sl.sweep(lay, dinv, rec.r, rec.z0, mutant="pairwise")
        s, start = case.lay[h]["sliced"], case.lay["color_start"]
        lp = s["long_pos"]
        rows = case.ref.perm[lp[(lp >= start[colour]) & (lp < start[colour + 1])]]
        assert len(rows) >= 4
        # in the loop's order the sum is Inf; by halving strides it is finite
        assert not np.any(np.isfinite(want[rows])), (name, rname, want[rows])
        assert np.all(np.isfinite(pairwise[rows])), (name, rname, pairwise[rows])
        assert not np.array_equal(np.isfinite(pairwise), np.isfinite(want))


# ---- (e) the pivot recipe ----------------------------------------------------------------
def test_pivot_recipe_counts_and_lanes():
    case = kc.cases()["pivots_in_785_rows"]
    rec = case.recipes()["pivots"]
    l, u, d = case.ref.factor(rec.va, case.diag_of(rec.va))
    assert kc.pivot_counts(d) == rec.pivots == kc.PIVOT_COUNTS == (3, 2)
    at = kc.PIVOT_AT
    assert d[at["zero"]] == 0.0 and d[at["negative"]] < 0 and np.isnan(d[at["nan"]])
    assert d[at["inf"]] == np.inf and d[at["negative_first"]] < 0
    start = case.diag_of(rec.va)[case.ref.perm]
    for key in ("zero", "negative", "nan", "inf"):  # they BECOME so
        assert np.isfinite(start[at[key]]) and start[at[key]] > 0, key
    bad = np.flatnonzero(~np.isfinite(d) | (d <= 0))
    assert sorted(bad.tolist()) == sorted(at.values())
    waves = bad // 64
    assert len(set(waves.tolist())) == len(bad)       # a wave each
    assert len(set((bad // 256).tolist())) == 4       # four workgroups
    assert at["zero"] % 64 == 0 and at["negative"] % 64 == 63
    assert at["negative_first"] % 64 == 63
    last = at["inf"] // 64
    assert last * 64 < case.n < (last + 1) * 64       # lanes beyond n


# ---- a deliberately wrong kernel would fail ------------------------------------------------
@pytest.mark.parametrize("mutant", ["pad", "first", "pairwise"])
def test_mutant_differs_from_the_reference(mutant):
    caught = []
    for name, case in kc.cases().items():
        for rname, rec in case.recipes().items():
            if not rec.sweep:
                continue
            fac, dinv = _sweep_inputs(case, rec)
            want = case.apply(fac, rec.r)
            lay = sl.with_values(case.lay, fac[0], fac[1])
            got = sl.sweep(lay, dinv, rec.r, rec.z0, mutant=mutant)
            if not sv.same_bits(got, want):
                caught.append((name, rname))
    print(mutant, "caught by", caught)
    assert caught, mutant
    recipes = {r for _, r in caught}
    if mutant == "pad":  # 0 * the poisoned z[0]
        assert "poison" in recipes
        # ... and the non-finite SET is what gives it away
        case = kc.cases()[caught[0][0]]
        rec = case.recipes()["poison"]
        fac, dinv = _sweep_inputs(case, rec)
        want = case.apply(fac, rec.r)
        got = sl.sweep(sl.with_values(case.lay, fac[0], fac[1]), dinv, rec.r,
                       rec.z0, mutant="pad")
        assert not np.array_equal(np.isfinite(got), np.isfinite(want))
    if mutant == "first":  # -0.0 + ... against 0.0 + -0.0
        assert "negzero" in recipes
    if mutant == "pairwise":
        assert {"overflow_before", "overflow_after"} <= recipes
