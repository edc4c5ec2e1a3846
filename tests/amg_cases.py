"""The aggregation multigrid preconditioner of host/cg.h (AmgPreconditioner)
restated in numpy: expanded rows, aggregates, the Galerkin operator with its
source lists, the row-sum bound and the V-cycle.  Every numpy operation is one
rounding per element; every sum that has an order is taken left to right
(seq_sum).  Shared by test_amg_host.py and test_gpu_amg.py.

Input form: the rows of a rank as a CSR triple with local column numbers;
columns >= n are ghosts and are dropped.  symmetric: the triple is the stored
strictly lower block (anything else is dropped) and `diagonal` the diagonal
array."""
import numpy as np

import gmres_cases as gc

DEFAULTS = dict(theta=0.25, max_levels=10, min_coarse_rows=200, smooth_degree=2,
                coarse_degree=8, eig_ratio=4.0, coarse_scale=1.0)


def seq_sum(ptr, vals, from_zero=False):
    """per group g the sum of vals[ptr[g]:ptr[g + 1]] left to right, starting
    from the first element (or from 0.0)"""
    ptr = np.asarray(ptr, np.int64)
    lens = np.diff(ptr)
    out = np.zeros(len(lens))
    k0 = 0
    if not from_zero:
        has = lens > 0
        out[has] = vals[ptr[:-1][has]]
        k0 = 1
    for k in range(k0, int(lens.max(initial=0))):
        g = np.nonzero(lens > k)[0]
        out[g] = out[g] + vals[ptr[g] + k]
    return out


def nanless_max(g):
    """the maximum from 0.0 in which a NaN never replaces a number (amg_diag's
    `if (g > max) max = g`); -> float"""
    g = np.asarray(g, np.float64)
    return float(g[~np.isnan(g)].max(initial=0.0))


def spmv_ltr(csr, x):
    """row sums left to right from 0.0, product rounded first"""
    rp, ci, va = csr
    return seq_sum(rp, va * x[ci], from_zero=True)


def vector_lanes(csr):
    """Lanes per row of the sub-wavefront SpMV kernel, or 0 where the plan of a
    general block keeps the sequential order: spmv_hip_csr_plan_create's rule
    for a block of fewer than sj_min_nnz = 2^20 entries."""
    rp = csr[0]
    n, nnz = len(rp) - 1, int(rp[-1])
    avg = nnz / n if n else 0.0
    if avg <= 64.0 or nnz >= 1 << 20 or nnz * 4 < n:
        return 0
    lpr = 4
    while lpr < 64 and lpr < avg / 2:
        lpr *= 2
    return lpr


def spmv_vector(csr, x, lpr):
    """the sub-wavefront kernel's order: lane l adds the products l, l + lpr,
    ... of the row left to right from 0.0, then the lanes are added pairwise,
    lane l += lane l + off for off = lpr / 2, ..., 1"""
    rp, ci, va = csr
    prod = va * x[ci]
    out = np.zeros(len(rp) - 1)
    for i in range(len(out)):
        p = prod[rp[i]:rp[i + 1]]
        lanes = np.zeros(lpr)
        for k in range(0, len(p), lpr):
            seg = p[k:k + lpr]
            lanes[:len(seg)] = lanes[:len(seg)] + seg
        off = lpr // 2
        while off:
            lanes[:off] = lanes[:off] + lanes[off:2 * off]
            off //= 2
        out[i] = lanes[0]
    return out


def expand(rp, ci, n, symmetric):
    """-> (ptr, col, src): the expanded rows; src >= 0 indexes the values, < 0
    is ~(row of the diagonal array)"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp[:n + 1]))
    ci = np.asarray(ci[:rp[n]], np.int64)
    e = np.arange(len(ci))
    if not symmetric:
        keep = ci < n
        r, c, s = rows[keep], ci[keep], e[keep]
        part = np.zeros(len(r), np.int64)
        seq = s
    else:
        keep = ci < rows
        lr, lc, ls = rows[keep], ci[keep], e[keep]
        i = np.arange(n)
        # lower (storage order), the diagonal, the mirror images by their row
        r = np.concatenate([lr, i, lc])
        c = np.concatenate([lc, i, lr])
        s = np.concatenate([ls, ~i, ls])
        part = np.concatenate([np.zeros(len(lr)), np.ones(n), np.full(len(lr), 2)])
        seq = np.concatenate([ls, i, ls])  # (row-major storage order: by row)
    order = np.lexsort((seq, part, r))
    r, c, s = r[order], c[order], s[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return ptr.astype(np.int64), c.astype(np.int32), s.astype(np.int32)


def values_of(src, va, diagonal):
    src = np.asarray(src, np.int64)
    out = np.empty(len(src))
    pos = src >= 0
    out[pos] = np.asarray(va)[src[pos]]
    if np.any(~pos):
        out[~pos] = np.asarray(diagonal)[~src[~pos]]
    return out


def aggregate(ptr, col, val, n, theta):
    """-> (agg, n_agg): the three passes of host/amg_build.h"""
    strong = []
    for i in range(n):
        c, a = col[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
        off = c != i
        m = np.abs(a[off]).max(initial=0.0)
        bar = theta * m
        seen, out = set(), []
        for j, v in zip(c.tolist(), a.tolist()):
            if j != i and v != 0.0 and abs(v) >= bar and j not in seen:
                seen.add(j)
                out.append(j)
        strong.append(out)
    agg = [-1] * n
    n_agg = 0
    for i in range(n):
        if agg[i] < 0 and all(agg[j] < 0 for j in strong[i]):
            for j in [i] + strong[i]:
                agg[j] = n_agg
            n_agg += 1
    snapshot = list(agg)
    for i in range(n):
        if snapshot[i] < 0:
            for j in strong[i]:
                if snapshot[j] >= 0:
                    agg[i] = snapshot[j]
                    break
    for i in range(n):
        if agg[i] < 0:
            agg[i] = n_agg
            for j in strong[i]:
                if agg[j] < 0:
                    agg[j] = n_agg
            n_agg += 1
    return np.array(agg, np.int32), n_agg


def coarsen(ptr, col, src, val, n, theta):
    """One step -> dict(n_agg, agg, member_ptr, member, rowptr, colind,
    src_ptr, src) or None when nothing merges.  The sources of a coarse entry
    are ordered by member row, then by the expanded row's order: the order of
    the expanded entries themselves."""
    agg, n_agg = aggregate(ptr, col, val, n, theta)
    member = np.argsort(agg, kind="stable").astype(np.int32)
    member_ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=n_agg))])
    rows = np.repeat(np.arange(n), np.diff(ptr))
    big_i, big_j = agg[rows].astype(np.int64), agg[col].astype(np.int64)
    order = np.lexsort((np.arange(len(col)), big_j, big_i))
    key = (big_i * max(n_agg, 1) + big_j)[order]
    first = np.concatenate([[True], key[1:] != key[:-1]]) if len(key) else \
        np.zeros(0, bool)
    start = np.nonzero(first)[0]
    src_ptr = np.concatenate([start, [len(key)]]).astype(np.int64)
    c_rows = big_i[order][start]
    return dict(n_agg=n_agg, agg=agg, member_ptr=member_ptr.astype(np.int32),
                member=member,
                rowptr=np.concatenate([[0], np.cumsum(np.bincount(
                    c_rows, minlength=n_agg))]).astype(np.int32),
                colind=big_j[order][start].astype(np.int32), src_ptr=src_ptr,
                src=src[order].astype(np.int32))


class AmgRef:
    """The hierarchy and the cycle.  spmv0(x_padded) -> the product of level 0
    (default: spmv_ltr on the rows as given, x padded with zeros to ncols);
    spmv_of(csr) -> the product of a coarse level (default: spmv_ltr)."""

    def __init__(self, csr, n, symmetric=False, diagonal=None, spmv0=None,
                 spmv_of=None, ncols=None, frozen=None, **options):
        """frozen: an AmgRef of the same pattern whose aggregates, coarse
        patterns and source lists are kept (what refresh() does)"""
        unknown = set(options) - set(DEFAULTS)
        assert not unknown, unknown
        self.opt = o = dict(DEFAULTS, **options)
        self.n = n
        rp, ci, va = csr
        ncols = n if ncols is None else ncols
        if spmv0 is None:
            assert not symmetric

            def spmv0(x):
                return spmv_ltr((rp, ci, va), x)
        self._pad = ncols - n
        spmv_of = spmv_of or (lambda c: (lambda x: spmv_ltr(c, x)))
        self.levels = []
        cur, sym, diag, spmv = (rp, ci, va), symmetric, diagonal, \
            (lambda x: spmv0(np.concatenate([x, np.zeros(self._pad)])))
        while True:
            rows = len(cur[0]) - 1
            ptr, col, src = expand(cur[0], cur[1], rows, sym)
            val = values_of(src, cur[2], diag)
            L = dict(n=rows, csr=cur, spmv=spmv, nnz=len(cur[1]))
            if sym:
                L["d"] = np.array(diag, np.float64)
            else:
                row_of = np.repeat(np.arange(rows), np.diff(ptr))
                on = col == row_of
                dptr = np.concatenate([[0], np.cumsum(np.bincount(
                    row_of[on], minlength=rows))])
                L["d"] = seq_sum(dptr, val[on], from_zero=True)
            if not (np.all(np.isfinite(L["d"])) and np.all(L["d"] > 0)):
                raise ValueError("diagonal is not positive")
            L["dinv"] = 1.0 / L["d"]
            g = seq_sum(ptr, np.abs(val)) * L["dinv"]
            L["lmax"] = nanless_max(g)
            if not (np.isfinite(L["lmax"]) and L["lmax"] > 0):
                raise ValueError("the row-sum bound is not finite")
            L["lmin"] = L["lmax"] / o["eig_ratio"]
            self.levels.append(L)
            if frozen is not None:
                step = frozen.levels[len(self.levels) - 1].get("step")
                if step is None:
                    break
            else:
                if not (rows > o["min_coarse_rows"]
                        and len(self.levels) < o["max_levels"]):
                    break
                step = coarsen(ptr, col, src, val, rows, o["theta"])
                if step["n_agg"] == rows:
                    break
            L["step"] = step
            c_val = seq_sum(step["src_ptr"], values_of(step["src"], cur[2], diag))
            cur = (step["rowptr"], step["colind"], c_val)
            sym, diag, spmv = False, None, spmv_of(cur)

    def _cheb(self, L, r, degree, z=None):
        """the `degree`-step Chebyshev iteration: from z = 0, or continued"""
        a, b = gc.chebyshev_coefficients(degree, L["lmin"], L["lmax"])
        dinv = L["dinv"]
        if z is None:
            d = b[0] * (dinv * r)
            z = d.copy()
        else:
            d = b[0] * (dinv * (r - L["spmv"](z)))
            z = z + d
        for j in range(1, degree):
            w = L["spmv"](z)
            d = a[j] * d + b[j] * (dinv * (r - w))
            z = z + d
        return z

    def cycle(self, level, r):
        L, o = self.levels[level], self.opt
        if level == len(self.levels) - 1:
            return self._cheb(L, r, o["coarse_degree"])
        st = L["step"]
        z = self._cheb(L, r, o["smooth_degree"])
        t = r - L["spmv"](z)
        rc = seq_sum(st["member_ptr"], t[st["member"]])
        e = self.cycle(level + 1, rc)
        z = z + o["coarse_scale"] * e[st["agg"]]
        return self._cheb(L, r, o["smooth_degree"], z)

    def apply(self, r):
        return self.cycle(0, np.asarray(r, np.float64))

    def dense_p(self, level):
        st = self.levels[level]["step"]
        P = np.zeros((self.levels[level]["n"], st["n_agg"]))
        P[np.arange(P.shape[0]), st["agg"]] = 1.0
        return P


def lower_split(csr):
    """a general symmetric matrix -> ((rp, ci, va) strictly lower, diagonal)"""
    rp, ci, va = csr
    n = len(rp) - 1
    rows = gc.row_of(rp)
    low = ci < rows
    lrp = np.concatenate([[0], np.cumsum(np.bincount(rows[low], minlength=n))])
    return (lrp.astype(np.int32), ci[low], va[low]), gc.diag_of(csr)


def dense(csr, n):
    rp, ci, va = csr
    A = np.zeros((n, n))
    rows = gc.row_of(rp)
    keep = ci < n
    np.add.at(A, (rows[keep], ci[keep]), va[keep])
    return A
