"""Reference loops, a bit comparison and data recipes for the special-value
tests (test_special_values_host.py, test_gpu_special_values.py): Inf, NaN,
signed zeros, overflowing partial sums and subnormals in x, y0 and the values.

ref_spmv / ref_spmv_sym restate csr_kernels.cpp:41-51 and :26-40 in numpy on
the arithmetic type `dtype`, with the library's one defined difference: at
beta == 0 the result is alpha * sum and y0 is never read (include/spmv_hip.h).
"""
import numpy as np

AB_S1 = ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0))
AB_S3 = ((1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (-1.0, 1.0))
AB_S4 = ((1.0, 0.0), (2.0, 1.0))
AB_S5 = ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0))


def _row_sums(rp, ci, va, x, start, dtype):
    """start[i] + va[j] * x[ci[j]] for j = rp[i] ... rp[i + 1] - 1, left to
    right, one rounding per product and one per addition; vectorised over the
    rows that still have an entry at position p."""
    rp = np.asarray(rp, np.int64)
    va, x = np.asarray(va, dtype), np.asarray(x, dtype)
    acc = np.array(start, dtype)
    lens = np.diff(rp)
    rows = np.flatnonzero(lens > 0)
    p = 0
    with np.errstate(all="ignore"):
        while len(rows):
            j = rp[rows] + p
            prod = va[j] * x[np.asarray(ci)[j]]
            acc[rows] = acc[rows] + prod
            p += 1
            rows = rows[lens[rows] > p]
    return acc


def ref_spmv(rp, ci, va, x, alpha, beta, y0, dtype):
    """y = alpha * A x + beta * y0, general storage (csr_kernels.cpp:41-51)."""
    dtype = np.dtype(dtype).type
    n = len(rp) - 1
    acc = _row_sums(rp, ci, va, x, np.zeros(n, dtype), dtype)
    with np.errstate(all="ignore"):
        out = dtype(alpha) * acc
        if beta != 0:
            out = out + dtype(beta) * np.asarray(y0, dtype)
    return out


def ref_spmv_sym(lrp, lci, lva, diag, x, alpha, beta, y0, dtype):
    """Symmetric storage (strictly lower CSR + diagonal, csr_kernels.cpp:26-40):
    the row sum starts from diag[i] * x[i]; out[col] += alpha * val * x[i] is
    added in row order (col < i: after out[col] got its own row's result)."""
    dtype = np.dtype(dtype).type
    n = len(diag)
    x, diag = np.asarray(x, dtype), np.asarray(diag, dtype)
    nnz = 0 if lva is None else len(lva)
    with np.errstate(all="ignore"):
        acc = diag * x
        if nnz:
            acc = _row_sums(lrp, lci, lva, x, acc, dtype)
        out = dtype(alpha) * acc
        if beta != 0:
            out = out + dtype(beta) * np.asarray(y0, dtype)
        if nnz:
            lva = np.asarray(lva, dtype)
            rows = np.repeat(np.arange(n), np.diff(np.asarray(lrp, np.int64)))
            add = dtype(alpha) * lva * x[rows]
            cols = np.asarray(lci, np.int64)
            order = np.argsort(cols, kind="stable")  # per column: row order
            cs = cols[order]
            first = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
            cnt = np.diff(np.r_[first, len(cs)])
            k = 0
            while len(first):
                idx = order[first + k]
                out[cols[idx]] = out[cols[idx]] + add[idx]
                k += 1
                keep = cnt > k
                first, cnt = first[keep], cnt[keep]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want):
    """NaN where and only where `want` is NaN (NaNs as a class: sign and payload
    of a generated NaN differ between processors); everywhere else the raw bits
    are equal, so -0.0 != +0.0 and +Inf != -Inf."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(bits(got)[~nan], bits(want)[~nan])


def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1,
                                             np.where(a == -np.inf, 2, 0)))


def flush(a):
    """subnormals -> zero of the same sign"""
    a = np.array(a)
    tiny = np.finfo(a.dtype).tiny
    sub = (np.abs(a) < tiny) & (a != 0)
    a[sub] = np.copysign(a.dtype.type(0), a[sub])
    return a


def subnormal(a):
    a = np.asarray(a)
    return (a != 0) & (np.abs(a) < np.finfo(a.dtype).tiny)


class Data:
    """One recipe applied to one pattern: values (and the diagonal of symmetric
    storage), x, y0 and the (alpha, beta) pairs to run."""

    def __init__(self, name, va, x, y0, ab, diag=None, **extra):
        self.name, self.va, self.x, self.y0, self.ab = name, va, x, y0, ab
        self.diag = diag
        self.__dict__.update(extra)
        for a in (va, x, y0, diag):
            if a is not None:
                a.setflags(write=False)


def _values(rng, nnz, dtype, group):
    """uniform(-1, 1) per entry -- or per group (constant diagonals: `group`
    gives every entry the index of its diagonal)"""
    if group is None:
        return rng.uniform(-1, 1, nnz).astype(dtype)
    return rng.uniform(-1, 1, int(group.max()) + 1 if nnz else 0).astype(dtype)


def _expand(v, group):
    return v if group is None else v[group]


POISON = (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)


def poison_columns(rng, ncols):
    """0, 255, 256, ncols - 1 and two drawn ones -- as many as exist"""
    cols = [c for c in (0, 255, 256, ncols - 1) if 0 <= c < ncols]
    cols = list(dict.fromkeys(cols))
    rest = np.setdiff1d(np.arange(ncols), cols)
    cols += [int(c) for c in rng.choice(rest, min(2, len(rest)), replace=False)]
    return np.array(cols, np.int64)


def s1(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """S1, poisoned x: uniform values and x, six columns NaN / +-Inf."""
    rng = np.random.default_rng([seed, 1])
    va = _expand(_values(rng, len(ci), dtype, group), group)
    x = rng.uniform(-1, 1, ncols).astype(dtype)
    y0 = rng.uniform(-1, 1, N).astype(dtype)
    diag = rng.uniform(-1, 1, N).astype(dtype) if sym else None
    cols = poison_columns(rng, ncols)
    x[cols] = np.array(POISON[:len(cols)], dtype)
    return Data("S1", va, x, y0, AB_S1, diag, poisoned=cols)


def s2(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """S2, stored zeros under Inf: S1 with the stored entries of the +-Inf
    columns set to +0.0 / -0.0 by halves (the reference multiplies them: NaN).
    With `group` (constant diagonals): one whole diagonal 0.0, another -0.0."""
    d = s1(rp, ci, N, ncols, dtype, seed, sym, group)
    va = d.va.copy()
    ci = np.asarray(ci)
    if group is None:
        hit = np.flatnonzero(np.isin(ci, d.poisoned[np.isinf(d.x[d.poisoned])]))
        va[hit[0::2]] = 0.0
        va[hit[1::2]] = -0.0
    else:
        va[group == 0] = 0.0
        va[group == 1] = -0.0
    return Data("S2", va, d.x.copy(), d.y0.copy(), AB_S1,
                None if d.diag is None else d.diag.copy(), poisoned=d.poisoned)


def s3(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """S3, signed zeros: x in {+0.0, -0.0}, a tenth of the values +-0.0, y0 in
    {+0.0, -0.0, 1.0}; symmetric storage: diagonals with -0.0 in them."""
    rng = np.random.default_rng([seed, 3])
    v = _values(rng, len(ci), dtype, group)
    z = rng.random(len(v)) < 0.1
    if group is not None and len(v) > 1:
        z[1] = True
    v[z] = rng.choice(np.array([0.0, -0.0], dtype), int(z.sum()))
    va = _expand(v, group)
    x = rng.choice(np.array([0.0, -0.0], dtype), ncols)
    y0 = rng.choice(np.array([0.0, -0.0, 1.0], dtype), N)
    diag = None
    if sym:
        diag = rng.uniform(-1, 1, N).astype(dtype)
        diag[rng.random(N) < 0.3] = -0.0
    return Data("S3", va, x, y0, AB_S3, diag)


def big(dtype):
    return np.dtype(dtype).type(1.5e308 if np.dtype(dtype) == np.float64 else 3e38)


def s4(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """S4, overflow order: x = 1, values +-M; a third of the rows read
    [+M, +M, -M, -M, ...] (left to right: +Inf), a third [+M, -M, +M, -M, ...]
    (0 or M), the rest a seeded order.  With `group`: the first pattern by
    diagonal."""
    rng = np.random.default_rng([seed, 4])
    M = big(dtype)
    rp = np.asarray(rp, np.int64)
    if group is None:
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        pos = np.arange(len(ci)) - rp[rows]
        sign = np.where(rows % 3 == 0, np.where(pos % 4 < 2, 1.0, -1.0),
                        np.where(rows % 3 == 1, np.where(pos % 2 == 0, 1.0, -1.0),
                                 rng.choice((-1.0, 1.0), len(ci))))
    else:
        sign = np.where(group % 4 < 2, 1.0, -1.0)
    va = (sign * M).astype(dtype)
    x = np.ones(ncols, dtype)
    y0 = rng.uniform(-1, 1, N).astype(dtype)
    diag = (rng.choice((-1.0, 1.0), N) * M).astype(dtype) if sym else None
    return Data("S4", va, x, y0, AB_S4, diag)


def s5(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """S5, subnormals: values and x uniform(-1, 1) * 2**-537 (fp32: 2**-70), so
    that the products are subnormal."""
    rng = np.random.default_rng([seed, 5])
    dt = np.dtype(dtype).type
    scale = dt(2.0 ** -537 if np.dtype(dtype) == np.float64 else 2.0 ** -70)
    va = _expand(_values(rng, len(ci), dtype, group), group) * scale
    x = rng.uniform(-1, 1, ncols).astype(dtype) * scale
    y0 = rng.uniform(-1, 1, N).astype(dtype) * dt(
        2.0 ** -1070 if np.dtype(dtype) == np.float64 else 2.0 ** -140)
    diag = rng.uniform(-1, 1, N).astype(dtype) * scale if sym else None
    return Data("S5", va, x, y0, AB_S5, diag)


def s5_mixed(rp, ci, N, ncols, seed=0, group=None):
    """S5 for the mixed f32f64 kernels: fp32 values uniform(-1, 1) * 2**-140
    (fp32 subnormals) under fp64 x = uniform(-1, 1) * 2**100.  `va` is fp32."""
    rng = np.random.default_rng([seed, 6])
    v = _values(rng, len(ci), np.float64, group) * 2.0 ** -140
    va = _expand(v.astype(np.float32), group)
    x = rng.uniform(-1, 1, ncols) * 2.0 ** 100
    y0 = rng.uniform(-1, 1, N) * 2.0 ** -40
    return Data("S5m", va, x, y0, AB_S5)


AB_G = ((1.0, 0.0), (-0.5, 0.0))


def g0(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """G0, S1 before the poison: finite data, so that x . y is finite (the
    tolerance branch of the fused dot's check)."""
    d = s1(rp, ci, N, ncols, dtype, seed, sym, group)
    x = d.x.copy()
    x[d.poisoned] = np.random.default_rng([seed, 7]).uniform(
        -1, 1, len(d.poisoned)).astype(dtype)
    return Data("G0", d.va.copy(), x, d.y0.copy(), AB_G,
                None if d.diag is None else d.diag.copy())


def ghost_columns(rng, N, ncols):
    """N (the first ghost), ncols - 1 and one drawn ghost column"""
    assert ncols >= N + 3
    c = int(rng.integers(N + 1, ncols - 1))
    return np.array([N, ncols - 1, c], np.int64)


def g1(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """G1, the poison in the ghost range only (columns >= N: a remote block
    after a failed exchange): NaN, +Inf, -Inf.  x[:N] is finite, so a NaN
    reaches x[:N] . y through y alone."""
    d = g0(rp, ci, N, ncols, dtype, seed, sym, group)
    x = d.x.copy()
    cols = ghost_columns(np.random.default_rng([seed, 8]), N, ncols)
    x[cols] = np.array(POISON[:3], dtype)
    return Data("G1", d.va.copy(), x, d.y0.copy(), AB_G, poisoned=cols)


def g2(rp, ci, N, ncols, dtype=np.float64, seed=0, sym=False, group=None):
    """G2, +Inf in three ghost columns under positive values, x[:N] positive:
    the rows that read them are +Inf and x[:N] . y is the infinity of alpha's
    sign, not NaN."""
    d = g0(rp, ci, N, ncols, dtype, seed, sym, group)
    x = d.x.copy()
    x[:N] = np.abs(x[:N]) + np.dtype(dtype).type(0.125)
    cols = ghost_columns(np.random.default_rng([seed, 8]), N, ncols)
    x[cols] = np.inf
    va = d.va.copy()
    hit = np.isin(np.asarray(ci), cols)
    va[hit] = np.abs(va[hit]) + np.dtype(dtype).type(0.125)
    return Data("G2", va, x, d.y0.copy(), AB_G, poisoned=cols)


def want_dot(d, N, y_ref):
    """x[:N] . y_ref in float64 (what the fused dot's partials add up to)"""
    with np.errstate(all="ignore"):
        return float(np.sum(d.x[:N].astype(np.float64) * y_ref.astype(np.float64)))


RECIPES = dict(S1=s1, S2=s2, S3=s3, S4=s4, S5=s5, G0=g0, G1=g1, G2=g2)


def reversed_rows(rp, ci, va):
    """the same rows with their entries in reversed order"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    pos = np.arange(len(ci)) - rp[rows]
    src = rp[rows + 1] - 1 - pos
    return np.asarray(ci)[src], np.asarray(va)[src]


# ---------------------------------------------------------------------------
# The patterns of test_gpu_special_values.py (the smallest case the form tests
# use per plan form); test_special_values_host.py holds every recipe to its
# target on each of them.
# ---------------------------------------------------------------------------
class Pattern:
    def __init__(self, rp, ci, N, ncols, sym=False, group=None, mirror=None,
                 recipes=("S1", "S2", "S3", "S4", "S5"), seed=0):
        self.rp = np.ascontiguousarray(rp, np.int32)
        self.ci = np.ascontiguousarray(ci, np.int32)
        self.N, self.ncols, self.sym, self.group = int(N), int(ncols), sym, group
        self.mirror, self.recipes, self.seed = mirror, recipes, seed
        self._data = {}

    def data(self, recipe, dtype=np.float64):
        """the recipe's data on this pattern (made once, read-only)"""
        key = (recipe, np.dtype(dtype).name)
        if key not in self._data:
            if recipe == "S5m":
                d = s5_mixed(self.rp, self.ci, self.N, self.ncols, self.seed,
                             self.group)
            else:
                d = RECIPES[recipe](self.rp, self.ci, self.N, self.ncols, dtype,
                                    self.seed, self.sym, self.group)
            if self.mirror is not None:  # values symmetric bit for bit
                va = d.va.copy()
                va[self.mirror[0]] = va[self.mirror[1]]
                va.setflags(write=False)
                d.va = va
            self._data[key] = d
        return self._data[key]

    def ref(self, d, alpha, beta, dtype=None):
        dtype = d.x.dtype if dtype is None else dtype
        if self.sym:
            return ref_spmv_sym(self.rp, self.ci, d.va, d.diag, d.x, alpha, beta,
                                d.y0, dtype)
        return ref_spmv(self.rp, self.ci, d.va, d.x, alpha, beta, d.y0, dtype)


def offset_groups(rp, ci):
    """per entry: the index of its diagonal among the pattern's offsets"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return np.unique(np.asarray(ci, np.int64) - rows, return_inverse=True)[1]


def mirror_map(rp, ci, N):
    """(upper entries, their lower mirrors) of a structurally symmetric CSR"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(N), np.diff(rp))
    cols = np.asarray(ci, np.int64)
    key = rows * N + cols
    order = np.argsort(key)
    pos = order[np.searchsorted(key[order], cols * N + rows)]
    up = np.flatnonzero(cols > rows)
    return up, pos[up]


def lower_pattern(rp, ci):
    rp = np.asarray(rp, np.int64)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    lo = np.asarray(ci) < rows
    lrp = np.zeros(n + 1, np.int64)
    np.add.at(lrp, rows[lo] + 1, 1)
    return np.cumsum(lrp), np.asarray(ci)[lo]


def sym_box_pattern(rng, N, P, L):
    """the 27 offsets a P + b L + c of a box stencil, structurally symmetric"""
    offs = sorted({s * (a * P + b * L + c) for s in (-1, 1) for a in (0, 1)
                   for b in (-1, 0, 1) for c in (-1, 0, 1)
                   if a * P + b * L + c >= 0})
    from gpu_helpers import stencil_csr
    rp, ci, _ = stencil_csr(rng, N, offs)
    return rp, ci


_PATTERNS = None


def patterns():
    global _PATTERNS
    if _PATTERNS is not None:
        return _PATTERNS
    from gpu_helpers import banded_mixed, stencil_csr
    from spmv_amd import poisson
    from util import random_csr
    rng = np.random.default_rng(0x5BEC1A1)
    P = {}
    rp, ci, _ = random_csr(rng, 513, 300, 8, long_rows=1, long_len=3000)
    P["ragged"] = Pattern(rp, ci, 513, 300)
    # ... square (the fused dot reads x[i] of every row), and the shape of a
    # remote block: columns beyond the rows (the ghost range), rows without
    # entries
    rp, ci, _ = random_csr(rng, 513, 513, 8, long_rows=1, long_len=3000)
    P["ragged_sq"] = Pattern(rp, ci, 513, 513)
    rp, ci, _ = random_csr(rng, 600, 900, 6, empty_frac=0.3)
    P["remote"] = Pattern(rp, ci, 600, 900)
    for n in (9, 16):
        rp, ci, _ = poisson.poisson3d_csr(n)
        P[f"poisson{n}"] = Pattern(rp, ci, n ** 3, n ** 3)
        # (constants that are symmetric: the tile kernel of 3-D lattices)
        P[f"poisson{n}_const"] = Pattern(rp, ci, n ** 3, n ** 3,
                                         group=offset_groups(rp, ci),
                                         mirror=mirror_map(rp, ci, n ** 3),
                                         seed=3)
        P[f"poisson{n}_symvals"] = Pattern(rp, ci, n ** 3, n ** 3,
                                           mirror=mirror_map(rp, ci, n ** 3))
        P[f"poisson{n}_lower"] = Pattern(*lower_pattern(rp, ci), n ** 3, n ** 3,
                                         sym=True)
    rp, ci, _ = stencil_csr(rng, 9001, [-700, -33, -2, -1, 0, 1, 40, 900], drop=0.33)
    P["eight"] = Pattern(rp, ci, 9001, 9001)
    rp, ci, _ = banded_mixed(rng, 5000)
    P["banded"] = Pattern(rp, ci, 5000, 5000)
    rp, ci, _ = random_csr(rng, 1500, 1500, 9, long_rows=2, long_len=700)
    P["sj_ragged"] = Pattern(rp, ci, 1500, 1500)
    rp, ci, _ = poisson.fem_like_csr(6000, jitter=64, layer=400)
    P["fem"] = Pattern(rp, ci, 6000, 6000)
    P["fem_lower"] = Pattern(*lower_pattern(rp, ci), 6000, 6000, sym=True)
    rp, ci, _ = poisson.fem_like_csr(9000, jitter=64, layer=500, tail_permille=20,
                                     tail_min=100, tail_max=900, tail_stride=4)
    P["fem_tail"] = Pattern(rp, ci, 9000, 9000)
    rp, ci, _ = poisson.fem_like_csr(7000, jitter=64, layer=400, tail_permille=5,
                                     tail_min=150, tail_max=600, tail_stride=3)
    P["fem_tail_lower"] = Pattern(*lower_pattern(rp, ci), 7000, 7000, sym=True)
    rp, ci, _ = poisson.stencil27_csr(7)
    P["stencil27"] = Pattern(rp, ci, 343, 343)
    P["stencil27_const"] = Pattern(rp, ci, 343, 343, group=offset_groups(rp, ci))
    P["stencil27_symvals"] = Pattern(rp, ci, 343, 343,
                                     mirror=mirror_map(rp, ci, 343))
    rp, ci, _ = stencil_csr(rng, 2000, list(range(-16, 16)), drop=0.1)
    P["thirty_two"] = Pattern(rp, ci, 2000, 2000)
    rp, ci = sym_box_pattern(rng, 9216, 1024, 32)
    P["box27"] = Pattern(rp, ci, 9216, 9216, mirror=mirror_map(rp, ci, 9216))
    rp, ci, _ = stencil_csr(rng, 5000, [-700, -30, -2, -1])
    P["four_lower"] = Pattern(rp, ci, 5000, 5000, sym=True)
    _PATTERNS = P
    return P
