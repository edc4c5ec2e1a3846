"""Cases for spmv::AmgPreconditioner on data that is not a benign matrix and a
benign right-hand side: systems scaled by powers of two, poisoned right-hand
sides, and matrices whose row-sum bound is not finite.  Nothing here touches a
GPU: test_amg_edges_host.py holds this module to its claims on the restatement
(amg_cases.AmgRef through test_gpu_amg.restate), test_gpu_amg_edges.py runs the
device on it.

a. SCALED.  The strength test |a| >= theta * max, the Galerkin sums, dinv = 1 / d
   and g = asum * dinv are covariant under A -> 2^s A as long as nothing
   overflows or turns subnormal: same aggregates, coarse values 2^s times,
   lmax the same bits, and amg_apply(2^s A, 2^t r) = 2^(t - s) amg_apply(A, r).
   PAIRS are solver_edges.SCALES and LARGE; the host test records every operand
   of both runs (`recorded`) and finds them finite and normal.
b. POISONS: one NaN, +Inf, -Inf or 1e300 in r at the first, a middle or the
   last row.
c. BAD BOUNDS: Poisson 11^3 with one diagonal entry 1e-310 (dinv = Inf), or with
   two symmetric pairs of 1e308 in one row (the sum of the row overflows).  Both
   pass the test d > 0 and give lmax = Inf: "the row-sum bound is not finite".
   NAN_FAR: a NaN pair far from the diagonal whose rows land in different
   aggregates on every level: g is NaN in a few rows, the maximum skips them,
   lmax stays finite and the object is accepted -- documented, not endorsed."""
import numpy as np

import gmres_cases as gc
import solver_edges as se
import test_gpu_amg as ta
import test_gpu_pcg as tp
from special_values import subnormal

MATRICES = ("poisson11", "ragged3001", "convdiff8")
OPTIONS = {"min_coarse_rows": 20}
LARGE = (300, 350)  # 2t, 2t - s and t - s stay far inside +-1022
PAIRS = se.SCALES + (LARGE,)
KMAX, RTOL = 60, 1e-8
POISON_KMAX = 8


def csr_of(name):
    rp, ci, va = ta._make_csr(name)
    return (np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32),
            np.ascontiguousarray(va, np.float64))


def storages(name):
    return (False, True) if name in ta.SYMMETRIC else (False,)


def clean_rhs(csr):
    return se.scaled_rhs(csr)


def recorded(ref):
    """Wraps the products of every level of an AmgRef: -> the list that receives
    every operand and result from now on (the vectors between them are sums
    and products of these with dinv and the coefficients)."""
    record = []
    for L in ref.levels:
        record += [L["d"], L["dinv"], L["csr"][2], np.array([L["lmax"], L["lmin"]])]

        def spmv(x, inner=L["spmv"]):
            y = inner(x)
            record.append(np.array(x))
            record.append(np.array(y))
            return y
        L["spmv"] = spmv
    return record


def all_normal(record):
    return all(np.all(np.isfinite(a)) and not np.any(subnormal(a)) for a in record)


POISON_VALUES = (np.nan, np.inf, -np.inf, 1e300)


def poisons(n, few=False):
    """[(value, row)]: every value at the first, a middle and the last row;
    few: every value once, the rows in turn"""
    rows = (0, n // 2, n - 1)
    if few:
        return [(v, rows[k % 3]) for k, v in enumerate(POISON_VALUES)]
    return [(v, r) for v in POISON_VALUES for r in rows]


def poisoned(r, value, row):
    out = np.array(r, np.float64)
    out[row] = value
    return out


# ---- c. bounds that are not finite ----------------------------------------------------
def _entry(csr, i, j):
    rp, ci, _ = csr
    e = np.flatnonzero(ci[rp[i]:rp[i + 1]] == j)
    assert len(e) == 1, (i, j)
    return int(rp[i] + e[0])


def tiny_diagonal(csr, row=17):
    """d = 1e-310 > 0: subnormal, dinv = Inf"""
    va = csr[2].copy()
    va[_entry(csr, row, row)] = 1e-310
    return csr[0], csr[1], va


def huge_pairs(csr, row=665):
    """(row, row +- 1) and their mirror images set to 1e308: every entry is
    finite, |row| overflows.  (Row 665 of Poisson 11^3 is interior.)"""
    va = csr[2].copy()
    for j in (row - 1, row + 1):
        va[_entry(csr, row, j)] = 1e308
        va[_entry(csr, j, row)] = 1e308
    return csr[0], csr[1], va


def nan_far(csr, ref, stride=121):
    """-> (csr with a NaN at (i, i + stride) and its mirror image, i): the
    first i whose frozen hierarchy accepts it (the two rows in different
    aggregates on every level, so that no coarse diagonal turns NaN)"""
    n = len(csr[0]) - 1
    for i in range(n // 2, n - stride):
        va = csr[2].copy()
        va[_entry(csr, i, i + stride)] = np.nan
        va[_entry(csr, i + stride, i)] = np.nan
        bad = (csr[0], csr[1], va)
        try:
            with np.errstate(all="ignore"):
                ta.restate(bad, n, False, frozen=ref, **OPTIONS)
        except ValueError:
            continue
        return bad, i
    raise AssertionError("no such pair")


def row_of(csr):
    return gc.row_of(csr[0])


def diag_of(csr):
    return tp._diag_of(csr)
