"""Small matrices with colours of the CALLER's choosing, each built to reach
named decision points of mcgs_sweep_kernel (hip/spmv_mcgs.hip) and of
ilu0_factor_kernel / ilu0_finish_kernel (hip/spmv_ilu0.hip), with value
recipes.  No GPU, no library.

A case is (csr, colours); reached() reads the decision points off the layout
arrays of sgs_layout and off the binary searches the factor kernel will make,
so test_sgs_kernel_cases_host.py can hold every case to its name.

Numbering.  Row 0 is isolated and wears the LAST colour: z[0] keeps its
prefill through the forward sweeps of all other colours and no row refers to
it, so a multiplied padding slot (column 0, value 0) shows as 0 * Inf.  The
designed rows follow, colour by colour; a few isolated rows wearing colour 0
close the numbering, so position != row for every designed row.  Inside a
part the columns ascend with their positions: test_gpu_sgs.Sweeps (column
order) and ilu0_cases.Ilu0Ref (position order) add in the same order.

Recipes (values of the whole CSR, r, the prefill of z):
  benign     small integers over 8, strictly diagonally dominant
  poison     benign values; Inf, -Inf, NaN in r; z prefilled with Inf / NaN
  negzero    mixed signs; r = -0.0 except every fifth row
  overflow_before / overflow_after   (sweep) diagonal 1, r = 1; in the
             `before` of the rows of colour 1 / the `after` of the rows of
             the last colour but one, entry k of a long row is +M if
             k % 64 < 32 else -M (an incomplete last chunk: +M, then ones; a
             short row: +M, -M, ...), every other entry 0.0: the z they
             multiply is 1, left to right the sum is Inf, a chunk added by
             halving strides finite -- and 0 * Inf = NaN carries the
             difference into every later colour
  subnormal  diagonals of 2^1023 (dinv subnormal), subnormal entries
  special    (factor) +-0.0 and subnormal entries, an Inf and a NaN entry in
             the last rows that have a `before`
  pivots     (the pivot case) 2 x 2 blocks whose second pivot becomes 0,
             negative, NaN, Inf at chosen lanes"""
import numpy as np

import ilu0_cases as ic
import sgs_layout as sl
import special_values as sv

ISO = 3          # isolated rows wearing colour 0 at the end of the numbering
KSLAB = 256      # kSlab of spmv_ilu0.hip
BIG = float(sv.big(np.float64))


class Blocks:
    """row numbers of the designed rows of every colour"""

    def __init__(self, sizes, iso=ISO):
        self.sizes = sizes
        first = 1 + np.concatenate([[0], np.cumsum(sizes)])
        self.n = int(first[-1]) + iso
        self.colours = np.zeros(self.n, np.int64)
        self.colours[0] = len(sizes) - 1
        for c, s in enumerate(sizes):
            self.colours[first[c]:first[c] + s] = c
        self._first = first

    def rows(self, c, idx=None):
        r = self._first[c] + np.arange(self.sizes[c])
        return r if idx is None else r[np.asarray(idx)]

    def row(self, c, t):
        return int(self._first[c] + t)


class Pairs:
    """directed off-diagonal entries (row, column)"""

    def __init__(self):
        self.a, self.b = [], []

    def add(self, rows, cols, mirror=True):
        rows, cols = np.broadcast_arrays(np.atleast_1d(rows), np.atleast_1d(cols))
        self.a += rows.tolist() + (cols.tolist() if mirror else [])
        self.b += cols.tolist() + (rows.tolist() if mirror else [])

    def csr(self, n):
        rows = np.concatenate([np.array(self.a, np.int64), np.arange(n)])
        cols = np.concatenate([np.array(self.b, np.int64), np.arange(n)])
        key = np.unique(rows * n + cols)
        rows, cols = key // n, key % n
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
        return rp.astype(np.int32), cols.astype(np.int32)


class Recipe:
    def __init__(self, va, r, z0=None, sweep=True, factor=True, pivots=None):
        self.va, self.r, self.sweep, self.factor = va, r, sweep, factor
        self.z0 = np.full(len(r), np.nan) if z0 is None else z0
        self.pivots = pivots  # (not usable, negative) the case states, or None


class Case:
    def __init__(self, name, pins, blocks, pairs, pivot_recipe=None):
        self.name, self.pins = name, tuple(pins)
        self.n, self.colours = blocks.n, blocks.colours
        self.rp, self.ci = pairs.csr(self.n)
        self.rows = ic.row_of(self.rp)
        self.on = self.ci == self.rows  # the diagonal entries, one per row
        self.nnz = len(self.ci)
        self._pivot_recipe = pivot_recipe
        self._recipes = None
        self.ref = ic.Ilu0Ref((self.rp, self.ci, self.benign_values()), self.n,
                              self.colours, False)
        self.lay = sl.layout(self.ref)

    # -- values ---------------------------------------------------------------------
    def _with_diagonal(self, off, extra):
        """`off` on the off-diagonal entries; diagonal = sum |off| of the row + extra"""
        va = np.where(self.on, 0.0, off)
        row_sum = np.bincount(self.rows, weights=np.abs(va), minlength=self.n)
        va[self.on] = row_sum + extra
        return va

    def benign_values(self, signs=False):
        i, j = self.rows.astype(np.int64), self.ci.astype(np.int64)
        off = -(1.0 + (3 * i + 5 * j) % 7) / 8.0
        if signs:
            off = np.where((i + j) % 2 == 0, -off, off)
        return self._with_diagonal(off, 1.0 + (np.arange(self.n) % 4) / 4.0)

    def benign_r(self):
        return ((7 * np.arange(self.n)) % 23 - 11.0) / 4.0

    def diag_of(self, va):
        d = np.zeros(self.n)
        d[self.rows[self.on]] = va[self.on]
        return d

    def parts_values(self, va):
        """(l, u, d) of the plain sweeps: the matrix's own values, d by position"""
        B, A = self.ref.parts
        return va[B["src"]], va[A["src"]], self.diag_of(va)[self.ref.perm]

    def apply(self, fac, r):
        """Ilu0Ref.apply, quietly: the recipes overflow on purpose"""
        with np.errstate(all="ignore"):
            return self.ref.apply(fac, r)

    def row_in(self, colour, with_before=True):
        """a designed row of `colour` (the one in the middle)"""
        nb = np.diff(self.ref.parts[0]["ptr"])[self.ref.pos]
        rows = np.flatnonzero((self.colours == colour) & ((nb > 0) == with_before)
                              & (np.diff(self.rp) > 1))
        return int(rows[len(rows) // 2])

    def recipes(self):
        if self._recipes is not None:
            return self._recipes
        n, nc = self.n, self.ref.nc
        out = {"benign": Recipe(self.benign_values(), self.benign_r())}
        # poison: r[0] = Inf keeps z[0] = Inf through the backward sweeps too
        r = self.benign_r()
        r[0] = np.inf
        r[self.row_in(0, False)] = -np.inf
        r[self.row_in(1 if nc > 2 else nc - 1)] = np.nan
        z0 = np.where(np.arange(n) % 2 == 0, np.inf, np.nan)
        out["poison"] = Recipe(self.benign_values(), r, z0)
        r = np.where(np.arange(n) % 5 == 0, self.benign_r(), -0.0)
        out["negzero"] = Recipe(self.benign_values(signs=True), r)
        # overflow: the rows of ONE colour get +-M in one part, every other
        # entry is 0.0; diagonal 1, r = 1, so the z they multiply is 1 exactly
        pos_colour = self.colours[self.ref.perm]
        for rname, part, colour in (("overflow_before", self.ref.parts[0], 1),
                                    ("overflow_after", self.ref.parts[1], nc - 2)):
            ptr = part["ptr"]
            m = np.repeat(np.diff(ptr), np.diff(ptr))
            k = np.arange(len(part["src"])) - np.repeat(ptr[:-1], np.diff(ptr))
            tail = k >= m // 64 * 64  # an incomplete last chunk: +M, then ones
            v = np.where(tail, np.where(k % 64 == 0, BIG, 1.0),
                         np.where(k % 64 < 32, BIG, -BIG))
            # a short row stays finite: +M, -M, +M, ...
            v = np.where(m > sl.LONG_THRESHOLD, v, np.where(k % 2 == 0, BIG, -BIG))
            mine = np.repeat(pos_colour == colour, np.diff(ptr))
            va = np.where(self.on, 1.0, 0.0)
            va[part["src"][mine]] = v[mine]
            out[rname] = Recipe(va, np.ones(n), factor=False)
        # subnormal: every third diagonal 2^1023, every eleventh entry subnormal
        va = self.benign_values()
        off = np.flatnonzero(~self.on)
        va[off] = va[off] * 2.0 ** -20
        va[off[::11]] = va[off[::11]] * 2.0 ** -1020
        d = self.diag_of(va)
        d[::3] = 2.0 ** 1023
        va[self.on] = d[self.rows[self.on]]
        out["subnormal"] = Recipe(va, self.benign_r())
        # special: zeros of both signs and subnormals among the entries; an Inf
        # and a NaN entry in the `before` of the last two rows that have one
        va = self.benign_values()
        va[off[0::40]] = -0.0
        va[off[10::40]] = 0.0
        va[off[20::40]] = 3.0 * 2.0 ** -1060
        va[off[30::40]] = -(2.0 ** -1070)
        B = self.ref.parts[0]
        has = np.flatnonzero(np.diff(B["ptr"]) > 0)
        va[B["src"][B["ptr"][has[-1]]]] = np.inf
        if len(has) > 1:
            va[B["src"][B["ptr"][has[-2] + 1] - 1]] = np.nan
        out["special"] = Recipe(va, self.benign_r(), sweep=False)
        if self._pivot_recipe:
            out["pivots"] = self._pivot_recipe(self)
        self._recipes = out
        return out


def pivot_counts(d):
    """ilu0_finish_kernel's two counters for the pivots d: (not finite or zero,
    finite and negative)"""
    d = np.asarray(d)
    finite = np.isfinite(d)
    return int(np.sum(~finite | (d == 0.0))), int(np.sum(finite & (d < 0.0)))


# ---- the decision points a case reaches ------------------------------------------------
def searches(ref):
    """Every binary search ilu0_factor_kernel makes, as (pos, tot, nb, kk, na_k,
    lo, found) arrays: row `pos` in step kk looks for the entries of after~(k)
    (na_k of them) in its list from kk + 1 on; lo = where the search ends."""
    B, A = ref.parts
    bptr, bc, aptr, ac = B["ptr"], B["cpos"], A["ptr"], A["cpos"]
    out = []
    for p in range(int(ref.color_start[1]) if ref.nc > 1 else ref.n, ref.n):
        cp = np.concatenate([bc[bptr[p]:bptr[p + 1]], [p], ac[aptr[p]:aptr[p + 1]]])
        nb, tot = int(bptr[p + 1] - bptr[p]), len(cp)
        for kk in range(nb):
            k = cp[kk]
            j = ac[aptr[k]:aptr[k + 1]]
            lo = kk + 1 + np.searchsorted(cp[kk + 1:], j)
            found = cp[np.minimum(lo, tot - 1)] == j
            found &= lo < tot
            out.append((p, tot, nb, kk, len(j), lo, found))
    return out


def reached(case):
    """the names of the decision points the case's layout and searches reach"""
    ref, lay = case.ref, case.lay
    pts = set()
    sizes = np.diff(ref.color_start)
    pts |= {f"colour_of_{s}_rows" for s in sizes.tolist()}
    if np.any(sizes % 64 != 0):
        pts.add("last_slice_cut_by_pos_end")
    for name in ("before", "after"):
        s = lay[name]["sliced"]
        lens = np.diff(lay[name]["ptr"])
        assert np.array_equal(s["len"] < 0, lens > sl.LONG_THRESHOLD)
        pts |= {f"{name}_long_row_of_{m}" for m in lens[s["len"] < 0].tolist()}
        pts |= {f"{name}_short_row_of_{m}" for m in s["len"][s["len"] >= 0].tolist()}
        for i, p0 in enumerate(s["slice_pos0"]):
            c = int(np.searchsorted(ref.color_start, p0, side="right")) - 1
            p1 = min(int(p0) + 64, int(ref.color_start[c + 1]))
            ln, full = s["len"][p0:p1], lens[p0:p1]
            span = int(s["slice_ptr"][i + 1] - s["slice_ptr"][i])
            if p1 - p0 == 64 and np.all(ln < 0):
                assert span == 0
                pts.add(f"{name}_slice_of_long_rows_only")
            if np.any(ln == 64) and np.any(full == 65):
                pts.add(f"{name}_64_next_to_65")
            if np.any((ln >= 0) & (64 * ln < span)):
                pts.add(f"{name}_padding")
    nb_all = np.diff(lay["before"]["ptr"])
    na_all = np.diff(lay["after"]["ptr"])
    tot_all = nb_all + 1 + na_all
    later = np.arange(ref.n) >= (ref.color_start[1] if ref.nc > 1 else ref.n)
    pts |= {f"tot_{t}" for t in tot_all[later].tolist()}
    if np.any(later & (nb_all == 0)):
        pts.add("nb_0_in_a_later_colour")
    if np.any(later & (nb_all == 0) & (na_all > 0)):
        pts.add("nb_0_with_after_in_a_later_colour")
    for p, tot, nb, kk, na_k, lo, found in searches(ref):
        path = "lds" if tot <= KSLAB else "global"
        pts.add(f"finished_row_of_{na_k}")
        if np.any(found & (lo < nb)):
            # step k updates the `before` entry that a later step multiplies with
            pts.add(f"{path}_multiplier_chain")
        if np.any(found & (lo == nb)):
            pts.add(f"{path}_fill_on_the_diagonal")
        if np.any(found & (lo > nb)):
            pts.add(f"{path}_fill_in_after")
        if np.any(~found & (lo == tot)):
            pts.add(f"{path}_drop_beyond_the_last")
        if np.any(~found & (lo == nb)):
            pts.add(f"{path}_drop_on_the_diagonal")
        if np.any(~found & (lo != nb) & (lo < tot)):
            pts.add(f"{path}_drop_in_the_middle")
    if ref.n > 3 * 256 and ref.n % 64 != 0:
        pts.add("finish_ragged_wave_several_workgroups")
    return pts


# ---- the cases --------------------------------------------------------------------------
def _ring(bl, pr, c, d, strides=((1, 0), (3, 1))):
    """designed row t of colour d <-> rows (a t + b) % size of colour c"""
    t = np.arange(bl.sizes[d])
    for a, b in strides:
        pr.add(bl.rows(d), bl.rows(c, (a * t + b) % bl.sizes[c]))


def colour_sizes():
    # with the isolated rows: 63, 1, 64, 65, 128, 129 rows
    bl, pr = Blocks([63 - ISO, 1, 64, 65, 128, 128]), Pairs()
    for c in range(5):
        _ring(bl, pr, c, c + 1)
    for c in range(4):
        _ring(bl, pr, c, c + 2, ((5, 2),))
    return Case("colour_sizes_1_63_64_65_128_129",
                [f"colour_of_{s}_rows" for s in (1, 63, 64, 65, 128, 129)]
                + ["last_slice_cut_by_pos_end", "before_padding", "after_padding"],
                bl, pr)


LONG_LENGTHS = (64, 65, 127, 128, 129, 192)


def long_lengths():
    bl, pr = Blocks([200, len(LONG_LENGTHS) + 3, 200]), Pairs()
    for t, m in enumerate(LONG_LENGTHS):
        pr.add(bl.row(1, t), bl.rows(0, np.arange(m)))
        pr.add(bl.row(1, t), bl.rows(2, np.arange(m)))
    for t in range(len(LONG_LENGTHS), len(LONG_LENGTHS) + 3):
        pr.add(bl.row(1, t), bl.rows(0, [t, 199 - t]))
        pr.add(bl.row(1, t), bl.rows(2, [2 * t, 198]))
    pins = []
    for name in ("before", "after"):
        pins += [f"{name}_short_row_of_64", f"{name}_64_next_to_65"]
        pins += [f"{name}_long_row_of_{m}" for m in LONG_LENGTHS[1:]]
    return Case("rows_of_64_65_127_128_129_192", pins, bl, pr)


def all_long_slice():
    bl, pr = Blocks([70, 64, 70]), Pairs()
    for t in range(64):
        pr.add(bl.row(1, t), bl.rows(0))
        pr.add(bl.row(1, t), bl.rows(2))
    return Case("slice_of_64_long_rows",
                ["before_slice_of_long_rows_only", "after_slice_of_long_rows_only",
                 "colour_of_64_rows", "lds_drop_beyond_the_last",
                 "lds_drop_on_the_diagonal", "lds_fill_on_the_diagonal"], bl, pr)


SLAB = ((127, 127), (128, 127), (128, 128), (300, 299))


def slab_limit():
    bl, pr = Blocks([300, len(SLAB), 299]), Pairs()
    for t, (nb, na) in enumerate(SLAB):
        pr.add(bl.row(1, t), bl.rows(0, np.arange(nb)))
        pr.add(bl.row(1, t), bl.rows(2, np.arange(na)))
    _ring(bl, pr, 0, 2, ((1, 0),))  # fill in the hubs' `after`
    return Case("factor_rows_of_255_256_257_600",
                ["tot_255", "tot_256", "tot_257", "tot_600", "global_fill_in_after",
                 "lds_fill_in_after"], bl, pr)


FINISHED = (0, 1, 63, 64, 65)


def finished_rows():
    bl, pr = Blocks([len(FINISHED), 70, 2]), Pairs()
    i, i2 = bl.row(2, 0), bl.row(2, 1)
    for t, m in enumerate(FINISHED):
        k = bl.row(0, t)
        pr.add(i, k, mirror=m > 0)  # after~(k_0) is empty: a(k_0, i) = 0
        if m > 1:
            pr.add(k, bl.rows(1, np.arange(m - 1)))
    pr.add(i, bl.rows(1, [0, 10, 61, 62, 63, 64, 69]))
    pr.add(i2, bl.rows(1, [5, 62, 63]))
    pr.add(i2, bl.rows(0, [0, 2]), mirror=False)
    return Case("finished_rows_of_0_1_63_64_65",
                [f"finished_row_of_{m}" for m in FINISHED]
                + ["lds_multiplier_chain"], bl, pr)


def global_chain():
    bl, pr = Blocks([10, 150, 2, 150]), Pairs()
    hub, twin = bl.row(2, 0), bl.row(2, 1)
    pr.add(hub, bl.rows(0))
    pr.add(hub, bl.rows(1))
    pr.add(hub, bl.rows(3))
    pr.add(twin, bl.rows(0))
    pr.add(twin, bl.rows(1, np.arange(50)))
    pr.add(twin, bl.rows(3, np.arange(50)))
    j = np.arange(150)
    pr.add(bl.rows(1), bl.rows(0, j % 10))
    pr.add(bl.rows(1), bl.rows(0, j % 7))
    pr.add(bl.rows(1), bl.rows(3))
    return Case("multiplier_chain_in_a_hub_row_of_311",
                ["tot_311", "global_multiplier_chain", "lds_multiplier_chain",
                 "global_fill_in_after", "global_fill_on_the_diagonal",
                 "global_drop_in_the_middle"], bl, pr)


def fill_and_nb0():
    bl, pr = Blocks([4, 4, 4, 4]), Pairs()
    a, b, c, d = (lambda t, col=col: bl.row(col, t) for col in range(4))
    i = c(1)
    pr.add(i, [a(1), b(2), d(1)])
    # after~(a_1): dropped in the middle (b_0, c_2), a later multiplier (b_2),
    # dropped where the search ends on the diagonal (b_3, c_0), the diagonal
    # (i), an entry of after(i) (d_1), dropped beyond the last entry (d_3)
    pr.add(a(1), [b(0), b(2), b(3), c(0), c(2), d(1), d(3)], mirror=False)
    pr.add(b(2), [a(0), d(0)])
    pr.add(b(3), a(3))
    pr.add(b(1), c(3))  # b_1: no `before`, one entry after it
    pr.add(c(0), [a(0), b(0)])
    pr.add(d(2), [a(2), b(3), c(2)])
    return Case("fill_dropped_everywhere_and_a_row_without_before",
                ["lds_drop_beyond_the_last", "lds_drop_in_the_middle",
                 "lds_drop_on_the_diagonal", "lds_fill_on_the_diagonal",
                 "lds_fill_in_after", "lds_multiplier_chain",
                 "nb_0_with_after_in_a_later_colour"], bl, pr)


# -- the pivot case: n = 256 * 3 + 17, pairs (k_t, i_t) of colour 0 and 1 -------------
PIVOT_N = 256 * 3 + 17
PIVOT_PAIRS = 390
# position of i_t = 392 + 1 + t (colour 0: 390 designed + 2 isolated rows; row 0
# leads colour 1); position of k_t = t
PIVOT_AT = dict(zero=448, negative=575, nan=600, inf=780, negative_first=63)
PIVOT_COUNTS = (3, 2)


def _pivot_recipe(case):
    va = np.zeros(case.nnz)
    i, j = case.rows, case.ci
    va[case.on] = np.where(case.colours[i[case.on]] == 0, 2.0, 3.0)
    va[~case.on] = 1.0
    ref = case.ref

    def put(r, c, v):
        e = np.flatnonzero((i == r) & (j == c))
        assert len(e) == 1
        va[e[0]] = v

    def pair(pos):
        row = int(ref.perm[pos])
        return int(row - PIVOT_PAIRS), row  # k_t, i_t

    k, r = pair(PIVOT_AT["zero"])
    put(r, r, 0.5)                      # 0.5 - (1 * 0.5) * 1 = 0
    k, r = pair(PIVOT_AT["negative"])
    put(r, r, 0.25)                     # 0.25 - 0.5 < 0
    k, r = pair(PIVOT_AT["nan"])
    put(r, k, 0.0)
    put(k, r, np.inf)                   # 3 - (0 * 0.5) * Inf = NaN
    k, r = pair(PIVOT_AT["inf"])
    put(k, k, 1.0)
    put(r, k, -BIG)
    put(r, r, BIG)                      # M - (-M * 1) * 1 = Inf
    row = int(ref.perm[PIVOT_AT["negative_first"]])
    put(row, row, -2.0)                 # colour 0: the pivot is the diagonal
    return Recipe(va, case.benign_r(), sweep=False, pivots=PIVOT_COUNTS)


def pivots():
    bl, pr = Blocks([PIVOT_PAIRS, PIVOT_PAIRS + 2], iso=2), Pairs()
    assert bl.n == PIVOT_N
    pr.add(bl.rows(1, np.arange(PIVOT_PAIRS)), bl.rows(0))
    return Case("pivots_in_785_rows",
                ["finish_ragged_wave_several_workgroups", "nb_0_in_a_later_colour",
                 "finished_row_of_1"], bl, pr, _pivot_recipe)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in (
            colour_sizes(), long_lengths(), all_long_slice(), slab_limit(),
            finished_rows(), global_chain(), fill_and_nb0(), pivots())}
    return _CASES


NAMES = ("colour_sizes_1_63_64_65_128_129", "rows_of_64_65_127_128_129_192",
         "slice_of_64_long_rows", "factor_rows_of_255_256_257_600",
         "finished_rows_of_0_1_63_64_65", "multiplier_chain_in_a_hub_row_of_311",
         "fill_dropped_everywhere_and_a_row_without_before", "pivots_in_785_rows")
RECIPES = ("benign", "poison", "negzero", "overflow_before", "overflow_after",
           "subnormal", "special")
# the decision points of the issue's list, each pinned by a case above
REQUIRED = (
    [f"colour_of_{s}_rows" for s in (1, 63, 64, 65, 128, 129)]
    + [f"{p}_{w}" for p in ("before", "after") for w in (
        "short_row_of_64", "long_row_of_65", "64_next_to_65",
        "slice_of_long_rows_only", "long_row_of_127", "long_row_of_128",
        "long_row_of_129", "long_row_of_192", "padding")]
    + ["last_slice_cut_by_pos_end", "tot_255", "tot_256", "tot_257", "tot_600"]
    + [f"finished_row_of_{m}" for m in FINISHED]
    + ["nb_0_with_after_in_a_later_colour", "lds_drop_beyond_the_last",
       "lds_drop_on_the_diagonal", "lds_drop_in_the_middle",
       "lds_fill_on_the_diagonal", "global_multiplier_chain",
       "finish_ragged_wave_several_workgroups"])
