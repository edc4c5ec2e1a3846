"""Hand-built coarsening steps in the layout of spmv_hip_amg_host, and the five
kernels of hip/spmv_amg.hip restated in numpy, one rounding per operation, on
amg_cases.seq_sum and amg_cases.values_of.  Nothing here touches a GPU:
test_amg_kernel_cases_host.py holds this module to its claims,
test_gpu_amg_kernels.py launches the kernels on it.

plan_create checks indices only, not that `src` describes a Galerkin product, so
the lists here are synthetic: whatever shape reaches a path of a kernel.

A step is a dict: fine_rows, coarse_rows, num_values, num_diagonal, coarse_nnz
and the arrays agg, member_ptr, member, src_ptr, src, xrow_ptr, xrow_src (None
where the layout allows NULL).  coarse_rows == 0 describes no step.

Grid shapes the cases are sized for (common.h, blas1_stream.h): galerkin and
restrict launch min(ceil(items / 256), grid_cap) workgroups of 256 lanes with
grid_cap = 8 * CUs; diag caps its grid at 256 workgroups (65 536 rows per
round); prolong and post0 give a workgroup units of 1 024 double2 elements and
wrap beyond grid_cap * 1 024 of them."""
import numpy as np

import amg_cases as ac

BLOCK = 256                 # kBlock
DIAG_ROUND = 256 * BLOCK    # rows of one round of amg_diag
UNIT = 4 * BLOCK            # kUnit: double2 elements per workgroup and trip
LONG = 2500                 # "at least 2 000" sources / members
NZ = np.float64(-0.0)


def grid_cap(num_cus):
    return 8 * num_cus


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _i64(a):
    return np.ascontiguousarray(a, np.int64)


def _idx(rows):
    return np.array(list(rows), np.int64)


def _ptr(lens):
    return _i64(np.concatenate([[0], np.cumsum(lens)]))


def make_step(agg=None, src_lens=None, src=None, num_values=0, num_diagonal=0,
              fine_rows=None, xrow_ptr=None, xrow_src=None):
    """agg None: no step (coarse_rows = 0).  The member lists are the rows of
    every aggregate ascending (a stable sort of agg)."""
    if agg is None:
        n, nc = int(fine_rows), 0
        agg_a = mp = mem = sp = sr = None
        nnz = 0
    else:
        agg_a = _i32(agg)
        n = len(agg_a)
        nc = int(agg_a.max()) + 1
        mem = _i32(np.argsort(agg_a, kind="stable"))
        mp = _i32(np.concatenate([[0], np.cumsum(np.bincount(agg_a,
                                                             minlength=nc))]))
        lens = np.zeros(0, np.int64) if src_lens is None else src_lens
        sp, nnz = _ptr(lens), len(lens)
        sr = _i32(src) if src is not None and len(src) else None
    return dict(fine_rows=n, coarse_rows=nc, num_values=int(num_values),
                num_diagonal=int(num_diagonal), coarse_nnz=int(nnz), agg=agg_a,
                member_ptr=mp, member=mem, src_ptr=sp, src=sr,
                xrow_ptr=None if xrow_ptr is None else _i64(xrow_ptr),
                xrow_src=None if xrow_src is None else _i32(xrow_src))


def _src_in_range(step, q):
    q = np.asarray(q, np.int64)
    return bool(np.all(np.where(q >= 0, q < step["num_values"],
                                ~q < step["num_diagonal"])))


def is_sound(s):
    """amg_is_sound of spmv_amg.hip, rule by rule"""
    n, nc = s["fine_rows"], s["coarse_rows"]
    if (n < 0 or nc < 0 or nc > n or s["num_values"] < 0
            or s["num_diagonal"] < 0 or s["coarse_nnz"] < 0):
        return False
    if s["num_diagonal"] not in (0, n):
        return False
    if nc == 0:
        if s["coarse_nnz"] != 0:
            return False
    else:
        agg, mp, mem, sp = s["agg"], s["member_ptr"], s["member"], s["src_ptr"]
        if agg is None or mp is None or mem is None or sp is None:
            return False
        if len(agg) != n or len(mem) != n or len(mp) != nc + 1:
            return False
        if np.any(agg < 0) or np.any(agg >= nc):
            return False
        if mp[0] != 0 or mp[nc] != n or np.any(np.diff(mp) <= 0):
            return False
        if np.any(mem < 0) or np.any(mem >= n):
            return False
        owner = np.repeat(np.arange(nc), np.diff(mp))
        if np.any(agg[mem] != owner):
            return False
        inside = np.ones(n, bool)
        inside[mp[:-1]] = False  # not the first member of a list
        if np.any(np.diff(mem.astype(np.int64))[inside[1:]] <= 0):
            return False
        if len(sp) != s["coarse_nnz"] + 1 or sp[0] != 0:
            return False
        if np.any(np.diff(sp) <= 0):
            return False
        count = int(sp[-1])
        if count > 0 and (s["src"] is None or len(s["src"]) != count):
            return False
        if count > 0 and not _src_in_range(s, s["src"]):
            return False
    if s["xrow_ptr"] is not None:
        xp = s["xrow_ptr"]
        if len(xp) != n + 1 or xp[0] != 0 or np.any(np.diff(xp) < 0):
            return False
        count = int(xp[n]) if n > 0 else 0
        if count > 0 and (s["xrow_src"] is None or len(s["xrow_src"]) != count):
            return False
        if count > 0 and not _src_in_range(s, s["xrow_src"]):
            return False
    return True


# ---------------------------------------------------------------------------
# the kernels, restated
# ---------------------------------------------------------------------------
def galerkin_ref(step, values, diagonal=None):
    """coarse_values[E] = v_0 + v_1 + ... from the first source"""
    with np.errstate(all="ignore"):
        return ac.seq_sum(step["src_ptr"],
                          ac.values_of(step["src"], values, diagonal))


def diag_ref(n, values, rowptr=None, colind=None, ncols_local=None,
             xrow_ptr=None, xrow_src=None, diagonal=None):
    """-> (d, dinv, bad, gmax, g).  The general form (rowptr, colind, ncols_local)
    or the xrow form (xrow_ptr, xrow_src, diagonal).  bad: the number of d that
    are not finite or not > 0; gmax: the maximum of g from 0.0, NaNs skipped."""
    with np.errstate(all="ignore"):
        if xrow_ptr is not None:
            d = np.array(diagonal[:n], np.float64)
            a = np.abs(ac.values_of(xrow_src[:xrow_ptr[n]], values, diagonal))
            asum = ac.seq_sum(xrow_ptr, a)
        else:
            rowptr = np.asarray(rowptr, np.int64)
            colind = np.asarray(colind[:rowptr[n]], np.int64)
            rows = np.repeat(np.arange(n), np.diff(rowptr))
            keep = colind < ncols_local
            r, c, v = rows[keep], colind[keep], np.asarray(values)[:rowptr[n]][keep]
            on = c == r
            d = ac.seq_sum(_ptr(np.bincount(r[on], minlength=n)), v[on],
                           from_zero=True)
            asum = ac.seq_sum(_ptr(np.bincount(r, minlength=n)), np.abs(v))
        dinv = 1.0 / d
        g = asum * dinv
        bad = int(np.sum(~np.isfinite(d) | ~(d > 0.0)))
        return d, dinv, bad, ac.nanless_max(g), g


def restrict_ref(step, r, w):
    """rc[I] = (t_0 + t_1) + ..., t_m = r[i_m] - w[i_m], members ascending"""
    with np.errstate(all="ignore"):
        return ac.seq_sum(step["member_ptr"], (r - w)[step["member"]])


def prolong_ref(step, scale, e, z):
    with np.errstate(all="ignore"):
        return z + np.float64(scale) * e[step["agg"]]


def post0_ref(b0, w, r, dinv, z):
    """-> (d, z_new): d = b0 * (dinv * (r - w)); z_new = z + d"""
    with np.errstate(all="ignore"):
        d = np.float64(b0) * (dinv * (r - w))
        return d, z + d


# ---------------------------------------------------------------------------
# galerkin
# ---------------------------------------------------------------------------
class Galerkin:
    def __init__(self, name, step, values, diagonal, **claims):
        self.name, self.step, self.values, self.diagonal = (name, step, values,
                                                            diagonal)
        self.claims = claims


def _galerkin_random(name, lens, nv, nd, seed, **claims):
    """lists of the given lengths over nv values and nd diagonal entries (nd
    fine rows in one aggregate), sources drawn at random from both arrays"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    total = int(lens.sum())
    q = rng.integers(0, nv, total)
    if nd:
        from_diag = rng.random(total) < 0.3
        q = np.where(from_diag, ~rng.integers(0, nd, total), q)
    step = make_step(np.zeros(max(nd, 1), np.int32), lens, q, nv, nd)
    values = rng.uniform(-1.0, 1.0, nv)
    diagonal = rng.uniform(1.0, 2.0, nd) if nd else None
    return Galerkin(name, step, values, diagonal, **claims)


def galerkin_special():
    """lists written out: signed zeros, Inf - Inf, a NaN in the middle,
    overflow; values[q] and diagonal[~q] mixed"""
    inf, nan = np.inf, np.nan
    values = np.array([NZ, 0.0, inf, -inf, 1.0, nan, 2.0, 1e308, 0.5])
    diagonal = np.array([NZ, 3.0, -inf])
    lists = [[0],                 # a lone -0.0 stays -0.0
             [1, 0],              # +0.0 + -0.0 = +0.0
             [0, 0],              # -0.0 + -0.0 = -0.0
             [~0],                # a lone -0.0 of the diagonal array
             [0, ~0],             # -0.0 + -0.0 across the arrays
             [2, 3],              # Inf + -Inf = NaN
             [2, ~2],             # the same across the arrays
             [4, 5, 6],           # a NaN in the middle
             [4, 8, 5, 6, 4],
             [7, 7],              # overflow to +Inf
             [7, 7, 3],           # ... and then NaN
             [4, ~1, 8]]          # finite, mixed
    step = make_step(np.zeros(3, np.int32), [len(x) for x in lists],
                     np.concatenate(lists), len(values), 3)
    return Galerkin("special", step, values, diagonal, negative_zero=(0, 2, 3, 4),
                    nan=(5, 6, 7, 8, 10))


def galerkin_cases():
    out = [_galerkin_random("lengths", [1, 2, 3, 64, 65, LONG], 700, 7, 1,
                            long_list=5),
           galerkin_special()]
    for nnz in (1, 255, 256, 257):
        rng = np.random.default_rng(nnz)
        out.append(_galerkin_random(f"entries{nnz}", rng.integers(1, 4, nnz), 300,
                                    5 if nnz % 2 else 0, nnz + 10))
    return out


def galerkin_wrap(num_cus):
    """more coarse entries than one pass of the grid holds, lists of <= 4"""
    nnz = grid_cap(num_cus) * BLOCK + 300
    rng = np.random.default_rng(5)
    return _galerkin_random("wrap", rng.integers(1, 5, nnz), 4096, 9, 6)


# ---------------------------------------------------------------------------
# diag
# ---------------------------------------------------------------------------
BAD_KINDS = ("pzero", "nzero", "negative", "nan", "pinf", "ninf", "empty",
             "ghost_only", "dup_cancel")
BAD_DIAGONAL = {"pzero": 0.0, "nzero": NZ, "negative": -2.0, "nan": np.nan,
                "pinf": np.inf, "ninf": -np.inf}
# variant "max_last" keeps to the kinds whose g is negative or NaN, so that the
# maximum is a finite number (d = 0 has g = +Inf)
TAME_KINDS = ("negative", "nan", "pinf", "ninf")
DIAG_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, DIAG_ROUND + 257)


class Diag:
    """One amg_diag case.  form "general": rowptr, colind, values, cols (>
    n: ghost columns), ncols_local = n.  form "xrow": step (no coarse level,
    xrow lists), values (the stored lower entries), diagonal.  claims: bad (the
    count by construction), gnan (rows whose g is NaN while d is good),
    max_row."""

    def __init__(self, name, form, n, **kw):
        self.name, self.form, self.n = name, form, n
        self.__dict__.update(kw)

    def ref(self):
        if self.form == "general":
            return diag_ref(self.n, self.values, self.rowptr, self.colind, self.n)
        return diag_ref(self.n, self.values, xrow_ptr=self.step["xrow_ptr"],
                        xrow_src=self.step["xrow_src"], diagonal=self.diagonal)


def bad_rows(n, variant):
    """{row: kind index}.  variant "bad": rows 0, 63, 64, n - 1, the whole
    wavefront 128..191, and in a second round its first row, 63 rows on and the
    wavefront from 64 rows on.  variant "max_last": the last row stays good (it
    holds the maximum) and so does row 64 (its g is NaN)."""
    if variant == "bad":
        rows = [0, 63, 64, n - 1] + list(range(128, 192))
        rows += [DIAG_ROUND, DIAG_ROUND + 63] + list(range(DIAG_ROUND + 64,
                                                           DIAG_ROUND + 128))
    else:
        rows = [0, 63, 130, DIAG_ROUND + 1]
    last = n - 1 if variant == "max_last" else -1
    rows = sorted({r for r in rows if 0 <= r < n and r != last})
    return {r: k for k, r in enumerate(rows)}


def gnan_rows(n, variant, bad):
    """rows with a good d and a NaN off the diagonal: lane 0 of a wavefront, a
    lane in the middle, one beside the end and one of a second round"""
    rows = [2, 64, 70, n - 2, DIAG_ROUND + 64, DIAG_ROUND + 70] \
        if variant == "max_last" else [1, 65, 200, DIAG_ROUND + 130]
    return sorted({r for r in rows if 0 <= r < n - 1 and r not in bad})


def diag_general(n, variant):
    """Rows (i - 1, i, i + 1) with a positive diagonal, every fifth row with a
    large entry in a ghost column (it must be dropped: kept, it would move the
    maximum), every seventh with diagonal duplicates 1, 2 (fine); the bad rows
    of `bad_rows`, kinds in turn; gnan rows; variant "max_last": the last row
    holds the maximum."""
    rng = np.random.default_rng(n + len(variant))
    bad = bad_rows(n, variant)
    gnan = gnan_rows(n, variant, bad)
    i = np.arange(n)
    rows = [i[1:], i, i[:-1]]
    cols = [i[1:] - 1, i, i[:-1] + 1]
    vals = [rng.uniform(-1, 1, max(n - 1, 0)), rng.uniform(2, 4, n),
            rng.uniform(-1, 1, max(n - 1, 0))]
    seq = [np.zeros(max(n - 1, 0)), np.ones(n), np.full(max(n - 1, 0), 4)]
    gh = i[i % 5 == 0]
    rows.append(gh), cols.append(n + gh % 3), vals.append(np.full(len(gh), 100.0))
    seq.append(np.full(len(gh), 2))
    dup = i[i % 7 == 3]  # the diagonal becomes 1 + 2: entry 1.0 here, 2.0 later
    vals[1][dup] = 1.0
    rows.append(dup), cols.append(dup), vals.append(np.full(len(dup), 2.0))
    seq.append(np.full(len(dup), 3))
    rows, cols, vals, seq = (np.concatenate(a) for a in (rows, cols, vals, seq))
    special = np.zeros(n + 1, bool)
    special[_idx(bad)] = True
    keep = ~special[rows]
    rows, cols, vals, seq = rows[keep], cols[keep], vals[keep], seq[keep]
    extra = []  # (row, col, value) in storage order
    kinds = {}
    for r, k in bad.items():
        pool = BAD_KINDS if variant == "bad" else TAME_KINDS
        kind = pool[k % len(pool)]
        kinds[r] = kind
        left = [(r, r - 1, 0.25)] if r > 0 else []
        right = [(r, r + 1, -0.5)] if r + 1 < n else []
        if kind in BAD_DIAGONAL:
            extra += left + [(r, r, BAD_DIAGONAL[kind])] + right
        elif kind == "ghost_only":
            extra += [(r, n, 5.0), (r, n + 2, -1.0)]
        elif kind == "dup_cancel":
            extra += left + [(r, r, 3.0)] + right + [(r, r, -3.0)]
    if extra:
        er, ec, ev = (np.array(a) for a in zip(*extra))
        rows = np.concatenate([rows, er.astype(np.int64)])
        cols = np.concatenate([cols, ec.astype(np.int64)])
        vals = np.concatenate([vals, ev.astype(np.float64)])
        seq = np.concatenate([seq, 10.0 + np.arange(len(er))])
    order = np.lexsort((seq, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    for r in gnan:  # an entry off the diagonal (the row has a right neighbour)
        e = np.flatnonzero((rows == r) & (cols == r + 1))[0]
        vals[e] = np.nan
    max_row = None
    if variant == "max_last" and n > 0:
        max_row = n - 1
        if n > 1:  # g of this row alone is beyond 2^9
            e = np.flatnonzero((rows == max_row) & (cols == max_row - 1))[0]
            vals[e] = 4096.0
    rowptr = _i32(_ptr(np.bincount(rows, minlength=n)))
    return Diag(f"general-{variant}-{n}", "general", n, rowptr=rowptr,
                colind=_i32(cols), values=np.ascontiguousarray(vals, np.float64),
                cols=n + 3, diagonal=None, bad=len(bad), kinds=kinds, gnan=gnan,
                max_row=max_row)


def diag_xrow(n, variant):
    """Symmetric storage of the tridiagonal matrix: values[i - 1] is the stored
    entry (i, i - 1); the expanded row i is (values[i - 1], diagonal[i],
    values[i]).  The bad rows take the diagonal values of BAD_DIAGONAL in turn;
    every eleventh good row has an empty list (g = 0.0, d stays good)."""
    rng = np.random.default_rng(2 * n + len(variant))
    bad = bad_rows(n, variant)
    # (a NaN at (n - 1, n - 2) would reach the row that holds the maximum)
    gnan = [r for r in gnan_rows(n, variant, bad)
            if not (variant == "max_last" and r == n - 2)]
    values = rng.uniform(-1, 1, max(n - 1, 0))
    diagonal = rng.uniform(2, 4, n)
    kinds = {}
    names = tuple(BAD_DIAGONAL) if variant == "bad" else TAME_KINDS
    for r, k in bad.items():
        kinds[r] = names[k % len(names)]
        diagonal[r] = BAD_DIAGONAL[kinds[r]]
    for r in gnan:
        values[r] = np.nan  # the entry (r + 1, r): in the rows r and r + 1
    i = np.arange(n)
    ent_r = np.concatenate([i[1:], i, i[:-1]])
    ent_s = np.concatenate([i[1:] - 1, ~i, i[:-1]])
    part = np.concatenate([np.zeros(max(n - 1, 0)), np.ones(n),
                           np.full(max(n - 1, 0), 2)])
    empty = (i % 11 == 5) & (i < n - 1)
    empty[_idx(bad)] = False
    empty[_idx(r for g in gnan for r in (g, g + 1) if r < n)] = False
    keep = ~empty[ent_r]
    ent_r, ent_s, part = ent_r[keep], ent_s[keep], part[keep]
    order = np.lexsort((part, ent_r))
    xrow_ptr = _ptr(np.bincount(ent_r, minlength=n))
    max_row = None
    if variant == "max_last" and n > 0:
        max_row = n - 1
        diagonal[max_row] = 2.0 ** -10
    step = make_step(None, fine_rows=n, num_values=len(values), num_diagonal=n,
                     xrow_ptr=xrow_ptr, xrow_src=ent_s[order])
    # a NaN at (r + 1, r) makes g NaN in row r + 1 too, where d is good
    gnan_all = sorted({r for g in gnan for r in (g, g + 1)
                       if r < n and r not in bad})
    return Diag(f"xrow-{variant}-{n}", "xrow", n, step=step, values=values,
                diagonal=diagonal, bad=len(bad), kinds=kinds, gnan=gnan_all,
                max_row=max_row, empty=np.flatnonzero(empty))


_DIAG = {}


def diag_cases():
    """every size in both forms and both variants, built once"""
    if not _DIAG:
        for n in DIAG_SIZES:
            for variant in ("bad", "max_last"):
                for make in (diag_general, diag_xrow):
                    c = make(n, variant)
                    _DIAG[c.name] = c
    return list(_DIAG.values())


# ---------------------------------------------------------------------------
# restrict
# ---------------------------------------------------------------------------
class Restrict:
    def __init__(self, name, step, r, w, **claims):
        self.name, self.step, self.r, self.w, self.claims = name, step, r, w, claims


def _agg_of_sizes(sizes, seed):
    """aggregates of the given sizes, their rows scattered over the range"""
    rng = np.random.default_rng(seed)
    agg = np.repeat(np.arange(len(sizes)), sizes)
    return agg[rng.permutation(len(agg))]


def _restrict_random(name, sizes, seed, **claims):
    agg = _agg_of_sizes(np.asarray(sizes, np.int64), seed)
    rng = np.random.default_rng(seed + 1)
    n = len(agg)
    return Restrict(name, make_step(agg), rng.uniform(-1, 1, n),
                    rng.uniform(-1, 1, n), **claims)


def restrict_special():
    """aggregate 0: r == w on all 3 members (+0.0); 1: a lone -0.0 - +0.0 =
    -0.0; 2: a lone Inf - Inf; 3: (1 - Inf) + 2; 4: -0.0 + -0.0; 5: finite"""
    inf = np.inf
    agg = np.array([0, 1, 0, 2, 3, 0, 3, 4, 5, 4, 5])
    r = np.array([1.5, NZ, -2.0, inf, 1.0, 0.3, 2.0, NZ, 0.7, NZ, 0.1])
    w = np.array([1.5, 0.0, -2.0, inf, inf, 0.3, 0.0, 0.0, 0.2, 0.0, 0.9])
    return Restrict("special", make_step(agg), r, w, positive_zero=(0,),
                    negative_zero=(1, 4), nan=(2,))


def restrict_cases():
    out = [_restrict_random("sizes", [1, 2, 3, LONG, 1, 2], 3, long_list=3),
           restrict_special()]
    for nc in (1, 256, 257):
        rng = np.random.default_rng(nc)
        out.append(_restrict_random(f"aggregates{nc}", rng.integers(1, 4, nc),
                                    nc + 20))
    return out


def restrict_wrap(num_cus):
    nc = grid_cap(num_cus) * BLOCK + 300
    rng = np.random.default_rng(8)
    return _restrict_random("wrap", rng.integers(1, 3, nc), 9)


# ---------------------------------------------------------------------------
# prolong and post0
# ---------------------------------------------------------------------------
STREAM_SIZES = (1, 2, 3, 2 * UNIT - 1, 2 * UNIT, 2 * UNIT + 1, 4 * UNIT + 1)
SCALES = (1.0, -0.0, 0.5, 1.6, np.inf)


def stream_wrap(num_cus):
    return 2 * grid_cap(num_cus) * UNIT + 2 * UNIT + 3


def sprinkle(v, seed):
    """-0.0, NaN, +Inf, -Inf and +0.0 at a few places of v (the first, the last
    and ones between, as the length allows), the rest kept"""
    v = np.array(v, np.float64)
    n = len(v)
    rng = np.random.default_rng(seed)
    spots = {0, n - 1} | set(rng.integers(0, n, 6).tolist())
    for k, p in enumerate(sorted(spots)):
        v[p] = (NZ, np.nan, np.inf, 0.0, -np.inf)[(k + seed) % 5]
    return v


def prolong_case(n, seed=0):
    """-> (step, e, z): n fine rows scattered over max(1, n // 3) aggregates;
    special values among e and z"""
    rng = np.random.default_rng(100 + n + seed)
    nc = max(1, n // 3)
    agg = np.concatenate([np.arange(nc), rng.integers(0, nc, n - nc)])
    agg = agg[rng.permutation(n)]
    e = sprinkle(rng.uniform(-1, 1, nc), seed + 1)
    z = sprinkle(rng.uniform(-1, 1, n), seed + 2)
    if n >= 3:  # a -0.0 that must survive z + scale * e for scale = -0.0
        z[1] = NZ
    return make_step(agg), e, z


def post0_case(n, seed=0):
    """-> (w, r, dinv, z) with special values in every one of them"""
    rng = np.random.default_rng(200 + n + seed)
    w, r, z = (sprinkle(rng.uniform(-1, 1, n), seed + k) for k in (3, 4, 5))
    dinv = sprinkle(rng.uniform(0.2, 1, n), seed + 6)
    return w, r, dinv, z
