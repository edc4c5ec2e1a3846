"""The multicolour ILU(0) of host/cg.h (spmv::Ilu0Preconditioner) restated in
numpy, and the arrow matrix.  No GPU, no library: the colours come from the
caller (the object's colors(), or the greedy colouring).

Everything is fp64 and every product, difference and quotient one rounding.
The restatement works in POSITION space: pos = the colour-major position of a
row (stable sort of the colours), the parts are CSR over positions with the
entries ascending by the position of their column, and the factor loop is the
definition's, row after row; only the innermost loop -- the entries of the
finished row k, which hit DISTINCT entries of row i -- is one numpy operation."""
import numpy as np


def arrow(n):
    """Rows 0 .. n-2 are coupled to row n-1 only; nonsymmetric, strictly
    diagonally dominant.  The greedy colouring gives two colours (rows 0 .. n-2,
    then row n-1) and the elimination of the last row creates no fill, so
    (D~ + L~) D~^-1 (D~ + U~) = A in exact arithmetic."""
    i = np.arange(n - 1)
    x = i.astype(np.float64)
    up = -(0.5 + 0.4 * np.sin(x))        # (i, n-1)
    low = -(0.3 + 0.25 * np.cos(2 * x))  # (n-1, i)
    diag = np.concatenate([2.0 + 0.5 * np.sin(3 * x), [low.__abs__().sum() + 3.0]])
    rows = np.concatenate([i, np.full(n - 1, n - 1), np.arange(n)])
    cols = np.concatenate([np.full(n - 1, n - 1), i, np.arange(n)])
    vals = np.concatenate([up, low, diag])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32), vals[order])


def row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


class Ilu0Ref:
    """Symbolic part: perm, pos, color_start and the two parts of the local
    diagonal block (columns < n) of a CSR as the storage holds them --
    symmetric: the stored lower entries and their mirror images, both with the
    index of the stored entry as their source."""

    def __init__(self, csr, n, colours, symmetric):
        rp, ci, va = csr
        rows = row_of(rp)[:len(ci)]
        src = np.arange(len(ci))
        if symmetric:
            low = ci < rows
            rows, cols, src = (np.concatenate([rows[low], ci[low]]),
                               np.concatenate([ci[low], rows[low]]),
                               np.concatenate([src[low], src[low]]))
        else:
            keep = (ci < n) & (ci != rows)
            rows, cols, src = rows[keep], ci[keep], src[keep]
        self.n = n
        self.colours = colours = np.asarray(colours, np.int64)[:n]
        self.nc = int(colours.max()) + 1 if n else 0
        self.perm = np.argsort(colours, kind="stable")
        self.pos = np.zeros(n, np.int64)
        self.pos[self.perm] = np.arange(n)
        self.color_start = np.concatenate(
            [[0], np.cumsum(np.bincount(colours, minlength=self.nc))]).astype(np.int64)
        rows, cols = rows.astype(np.int64), cols.astype(np.int64)
        prow, pcol = self.pos[rows], self.pos[cols]
        order = np.lexsort((pcol, prow))
        prow, pcol, src, cols = prow[order], pcol[order], src[order], cols[order]
        if np.any((prow[1:] == prow[:-1]) & (pcol[1:] == pcol[:-1])):
            raise ValueError("duplicate column in a row of the block")
        assert not np.any(colours[self.perm[prow]] == colours[cols])
        self.parts = []
        for sel in (colours[cols] < colours[self.perm[prow]],
                    colours[cols] > colours[self.perm[prow]]):
            r = prow[sel]
            ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
            self.parts.append(dict(ptr=ptr.astype(np.int64), cpos=pcol[sel],
                                   col=cols[sel], src=src[sel]))
        self.values = np.asarray(va, np.float64)
        if symmetric:  # the diagonal has an array of its own in that storage
            on = ci == row_of(rp)[:len(ci)]
            self.diag = np.zeros(n)
            np.add.at(self.diag, ci[on], va[on])
        else:
            self.diag = np.zeros(n)
            all_rows = row_of(rp)[:len(ci)]
            for e in np.flatnonzero(ci == all_rows):  # storage order
                self.diag[ci[e]] = self.diag[ci[e]] + va[e]

    # -- the factor ---------------------------------------------------------------
    def factor(self, values=None, diag=None):
        """-> (l, u, d): l~ and u~ in part order, d~ by position"""
        values = self.values if values is None else np.asarray(values)
        diag = self.diag if diag is None else np.asarray(diag)
        B, A = self.parts
        bptr, bc, aptr, ac = B["ptr"], B["cpos"], A["ptr"], A["cpos"]
        bw, aw = values[B["src"]].copy(), values[A["src"]].copy()
        wd = diag[self.perm].copy()
        with np.errstate(all="ignore"):
            wdinv = 1.0 / wd
            for p in range(int(self.color_start[1]) if self.nc > 1 else self.n,
                           self.n):
                b0, b1, a0, a1 = bptr[p], bptr[p + 1], aptr[p], aptr[p + 1]
                nb = b1 - b0
                cp = np.concatenate([bc[b0:b1], [p], ac[a0:a1]])
                w = np.concatenate([bw[b0:b1], [wd[p]], aw[a0:a1]])
                for kk in range(nb):  # ascending pos(k): w[kk] is final
                    k = cp[kk]
                    m = w[kk] * wdinv[k]
                    j = ac[aptr[k]:aptr[k + 1]]
                    u = aw[aptr[k]:aptr[k + 1]]
                    at = np.minimum(np.searchsorted(cp, j), len(cp) - 1)
                    hit = cp[at] == j
                    w[at[hit]] = w[at[hit]] - m * u[hit]
                bw[b0:b1], wd[p], aw[a0:a1] = w[:nb], w[nb], w[nb + 1:]
                wdinv[p] = 1.0 / wd[p]
        return bw, aw, wd

    # -- the two sweeps -------------------------------------------------------------
    def _sum(self, part, vals, c, zp):
        c0, c1 = int(self.color_start[c]), int(self.color_start[c + 1])
        P = np.arange(c0, c1)
        ptr, cpos = self.parts[part]["ptr"], self.parts[part]["cpos"]
        lens = ptr[P + 1] - ptr[P]
        s = np.zeros(c1 - c0)
        for k in range(int(lens.max()) if len(lens) else 0):
            sel = lens > k
            e = ptr[P[sel]] + k
            s[sel] = s[sel] + vals[e] * zp[cpos[e]]
        return P, s

    def apply(self, fac, r):
        """z = M^-1 r with fac = (l, u, d): sgs_apply's sweeps, the sums in
        position order"""
        l, u, d = fac
        with np.errstate(all="ignore"):
            dinv = 1.0 / d
        rp = np.asarray(r)[self.perm]
        zp = np.full(self.n, np.nan)
        for c in range(self.nc):
            P, s = self._sum(0, l, c, zp)
            zp[P] = (rp[P] - s) * dinv[P]
        for c in range(self.nc - 2, -1, -1):
            P, t = self._sum(1, u, c, zp)
            zp[P] = zp[P] - dinv[P] * t
        z = np.zeros(self.n)
        z[self.perm] = zp
        return z

    # -- dense, in the caller's numbering (small n only) -------------------------------
    def dense_m(self, fac):
        """(D~ + L~) D~^-1 (D~ + U~) as a dense matrix"""
        l, u, d = fac
        n = self.n
        L, U = np.zeros((n, n)), np.zeros((n, n))
        for M, part, vals in ((L, self.parts[0], l), (U, self.parts[1], u)):
            prow = np.repeat(np.arange(n), np.diff(part["ptr"]))
            M[prow, part["cpos"]] = vals
        D = np.diag(d)
        Mp = (D + L) @ np.diag(1.0 / d) @ (D + U)
        out = np.zeros((n, n))
        out[np.ix_(self.perm, self.perm)] = Mp
        return out


def greedy_colours(csr, n, symmetric=False):
    """sgs_color restated: colour(i) = the smallest colour no neighbour j < i in
    B + B^T wears"""
    rp, ci, _ = csr
    rows = row_of(rp)[:len(ci)]
    keep = (ci < n) & (ci != rows) & ((ci < rows) if symmetric else True)
    a, b = rows[keep], ci[keep]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    start = np.searchsorted(hi, np.arange(n + 1))
    colour = np.full(n, -1, np.int64)
    for i in range(n):
        worn = set(colour[lo[start[i]:start[i + 1]]].tolist())
        c = 0
        while c in worn:
            c += 1
        colour[i] = c
    return colour
