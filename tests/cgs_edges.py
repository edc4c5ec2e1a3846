"""Cases and references for whole cg_shifted solves on inputs that are not a
benign SPD system: every exit on exact block matrices, the floor of scaling,
non-finite and overflowing data and shifts, and systems scaled by powers of two
or negated.  Nothing here touches a GPU: test_cgs_edges_host.py holds this
module to its claims on the reference alone, test_gpu_cgs_edges.py runs
host.cg_shifted on it.  The companion of solver_edges.py and minres_edges.py.

The reference is cgs_cases.cgs_ref, imported, under np.errstate(all="ignore").
Its comparisons were read against cg.h and blas1_cgshift.hip, in the kernels'
order:
  start     hist_s[0] is written, then `rr == 0` (status 0, k = 0)
  update_r  `not (pq > 0)` (true on a NaN): r is left alone; a = rr / pq is
            guarded by it
  step      `not (pq > 0)` FIRST (status 1 at the k reached, X the last
            iterate), then `k >= kmax`; bn = rrn / rr (rr != 0 by the start
            test or the `rrn == 0` stop of the step before); per shift rhon_s
            (its divisor is not guarded: a zero gives Inf, see huge_shift),
            hist_s[k + 1], then `h / hist0 < rtol` (false on a NaN: the shift
            goes on); at the end `no shift left or rrn == 0 or k + 1 == kmax`
            (status 0).  The host launches no step beyond kmax, so a curvature
            breakdown that would be found in step kmax + 1 is NOT found: with
            kmax = the k of a status-1 row the outcome is that row with status
            0.
cgs_ref works in numpy scalars: nothing raises; cgs_cases.py is unchanged.

a. EXACT cases: one small integer block repeated NB times, with and without
   the tail row (entry 1, b = 0), rr[0] = 1024, hist_s[0] = 32; rtol = 0 and
   kmax = 40, and again kmax = k.  S3 = (0, 2, 6), S8 = (0, 2, 6, ..., 254):
   2 + sigma a power of two.  As measured on the reference:

     name       block            b       NB    N         shifts  k  its   status
     two_i      [[2,0],[0,2]]    (1,1)   512   1024(+1)  S3      1  1     0
     two_i_ns1  as two_i                                 (0)     1  1     0
     two_i_ns8  as two_i                                 S8      1  1     0
                rrn == 0 at k = 1, x_s = b / (2 + sigma_s) exactly
     curv1      [[0,1],[1,0]]    (0,1)   1024  2048      S3      0  0     1
                not (pq > 0) in the first iteration, X = 0
     curv2      [[0,0,1],[0,1,1],[1,1,0]] (1,-1,0) 512 1536 S3   1  1     1
                p.q == 0 in the SECOND iteration: k = 1 (solver_edges counts
                the iteration, 2), X the iterate of k = 1.  a = 2 and rhon_s =
                1, 1/5, 1/13: the last two round once, and reach only the
                history and X (elementwise), which no sum reads
     negative   [[-2,0],[0,-2]]  (1,1)   512   1024      S3      0  0     1
     early      [[1,1],[1,2]]    (0,1)   1024  2048  (0, 2^41-2) 2  2, 1  0
                rtol = 2^-30: the large shift stops at step 1 (zeta = 2^-40)
                with x = 2^-41 b, sigma = 0 goes on and ends by rrn == 0 at k
                = 2 with A x = b (`search_early`, a Fraction search)
     zero       [[2,0],[0,2]]    (0,0)   512   1024      S3      0  0     0
   With kmax = k a status-1 row returns status 0 (see step above).
b. FLOOR: FLOOR_CASES under scale_csr(s) with the shifts times 2^s.  No square
   of an entry of A is ever formed (pq and a carry 2^s and 2^-s once): every s
   of FLOOR_S repeats the unscaled row, X times 2^-s.
c. POISONED data on poisson11 in both storages, shifts (0, 1, 4), kmax 12, rtol
   1e-10, and huge_shift: shifts (0, 1e300) on clean data.  POISON_OUTCOME:
     b_nan, b_inf, a_nan   pq is NaN: k = 0, status 1, X = 0
     b_huge  rr = pq = Inf, a = NaN: pq is NaN in the second step: k = 1,
             status 1, X all NaN
     b_tiny  rr underflows to 0: k = 0, status 0, X = 0 although b != 0
     huge_shift  sigma * a = 1e299 is finite, rhon = zeta = 1e-299 and a * rhon
             = 1e-300: the shift stops at step 1 with x = b / sigma and a
             history of 1e-298, and the column of sigma = 0 has the bits of
             the solve with that shift alone
   WEAK: huge_shift in both storages (twelve clean steps that round): 2 of 12.
d. SCALED systems (2^s A, 2^t b, shifts 2^s): every x_s times 2^(t-s), every
   history times 2^t, the same counts.  PAIRS drops (-400, -300) of
   minres_edges.PAIRS: p.q = 2^(2t + s) p.Ap = 2^-1000 times a quantity that
   shrinks to 1e-16 of its start is subnormal on the reference itself.
   (A, -b) gives -X and the same history; (-A, b) is status 1 at k = 0."""
import numpy as np

import cgs_cases as cc
import minres_edges as me
import oracle
import solver_edges as se
from cgs_cases import cgs_ref  # noqa: F401  (the reference, not a copy)
from minres_edges import rank1_nan, tiled  # noqa: F401
from solver_edges import (DOT, POISONS, SCALES, _recording,  # noqa: F401
                          block_system, clean_rhs, dot_chunked, dot_reversed,
                          poisoned, same_bits, scale_csr, scaled_rhs)

ORDERS = (DOT, dot_reversed, dot_chunked)
KMAX = 40


class Result:
    """solver_edges.Result's sibling for ns solutions"""

    def __init__(self, X, k, its, hist, status=0):
        self.x = np.asarray(X, np.float64)
        self.k, self.status = int(k), int(status)
        self.its = [int(i) for i in its]
        self.hist = np.asarray(hist, np.float64)

    def same(self, other):
        return (self.k == other.k and self.status == other.status
                and self.its == other.its and same_bits(self.hist, other.hist)
                and same_bits(self.x, other.x))


def pattern(r):
    return (r.k, r.status, r.its, r.hist.shape, np.isnan(r.hist).tolist(),
            np.isinf(r.hist).tolist(), np.isnan(r.x).tolist(),
            np.isinf(r.x).tolist())


def reference(csr, b, shifts, kmax, rtol, dot=DOT, record=None, ref=None,
              symmetric=False):
    spmv = me.spmv_of(csr, symmetric)
    if record is not None:
        spmv, dot = _recording(spmv, dot, record)
    X, k, its, hist, status = (ref or cc.cgs_ref)(
        spmv, dot, np.asarray(b, np.float64), tuple(shifts), kmax, rtol)
    return Result(X, k, its, hist, status)


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
def tailed_system(block, rhs, nb, tail):
    """minres_edges.tailed_system for any NB with an even len(block) * NB"""
    (rp, ci, va), b = block_system(block, rhs, nb)
    assert len(b) == len(block) * nb + 1
    if not tail:
        rp, ci, va, b = rp[:-1], ci[:-1], va[:-1], b[:-1]
    return tuple(np.ascontiguousarray(a) for a in (rp, ci, va)), \
        np.ascontiguousarray(b)


def simulate(A, b, sigma, kmax=3):
    """cg_shifted on one block in Fraction arithmetic with the shifts (0,
    sigma), sigma's shift frozen after step 1 -> (k, "conv") when r == 0 after
    k steps; None when a, bn or rhon of step 1 is not dyadic"""
    from fractions import Fraction as F
    n = len(b)
    if any(A[i][j] != A[j][i] for i in range(n) for j in range(i)):
        return None
    r = [F(v) for v in b]
    p = r[:]
    rr = se._dot(r, r)
    if rr == 0:
        return None
    for k in range(1, kmax + 1):
        q = se._mv(A, p)
        pq = se._dot(p, q)
        if pq <= 0:
            return None
        a = rr / pq
        if not se._dyadic(a) or (k == 1 and not se._dyadic(1 / (1 + sigma * a))):
            return None
        r = [x - a * y for x, y in zip(r, q)]
        rrn = se._dot(r, r)
        if rrn == 0:
            return (k, "conv")
        bn = rrn / rr
        if not se._dyadic(bn):
            return None
        p = [x + bn * y for x, y in zip(r, p)]
        rr = rrn
    return None


EARLY_SIGMA = 2.0 ** 41 - 2.0


def search_early():
    """the first 2x2 block and right-hand side over solver_edges.ORDER5 that CG
    solves exactly in TWO steps with dyadic scalars and 1 + EARLY_SIGMA * a_1
    a power of two"""
    import itertools
    from fractions import Fraction as F
    for ent in itertools.product(se.ORDER5, repeat=4):
        A = (ent[:2], ent[2:])
        for b in itertools.product(se.ORDER5, repeat=2):
            if simulate(A, b, F(EARLY_SIGMA)) == (2, "conv"):
                return A, b
    return None


TWO_I = (((2, 0), (0, 2)), (1, 1))
S3, S1 = (0.0, 2.0, 6.0), (0.0,)
S8 = (0.0, 2.0, 6.0, 14.0, 30.0, 62.0, 126.0, 254.0)
EARLY = (((1, 1), (1, 2)), (0, 1))  # search_early()


class Exact:
    def __init__(self, name, system, nb, shifts, k, its, status, hist, x,
                 rtol=0.0, solved=False):
        self.id = self.name = name
        self.block, self.rhs = system
        self.nb, self.shifts, self.rtol = nb, shifts, rtol
        self.k, self.its, self.status = k, list(its), status
        self.solved = solved  # (A + sigma_s I) x_s == b for every s with its_s == k
        self.hist_rows, self.xblocks = hist, x
        self._sys = {}

    def system(self, tail):
        if tail not in self._sys:
            self._sys[tail] = tailed_system(self.block, self.rhs, self.nb, tail)
        return self._sys[tail]

    def kmaxes(self):
        return (KMAX, self.k)

    def want(self, tail, kmax=KMAX):
        """the table row; at kmax = k a status-1 row has status 0 (the step
        that would find p.q <= 0 is never launched)"""
        hist = np.full((len(self.shifts), kmax + 1), -1.0)
        for s, row in enumerate(self.hist_rows):
            hist[s, :len(row)] = row
        X = np.stack([tiled(xb, self.nb, tail) for xb in self.xblocks])
        status = self.status if kmax > self.k else 0
        return Result(X, self.k, self.its, hist, status)


def exact_cases():
    E = Exact
    z2, z3 = (0.0, 0.0), (0.0, 0.0, 0.0)
    inv = lambda sh: [(1 / (2 + s),) * 2 for s in sh]  # noqa: E731
    neg = (((-2, 0), (0, -2)), (1, 1))
    return [
        # name, (block, b), NB, shifts, k, iterations, status, history, x
        E("two_i", TWO_I, 512, S3, 1, [1] * 3, 0, [[32, 0]] * 3, inv(S3),
          solved=True),
        E("two_i_ns1", TWO_I, 512, S1, 1, [1], 0, [[32, 0]], inv(S1),
          solved=True),
        E("two_i_ns8", TWO_I, 512, S8, 1, [1] * 8, 0, [[32, 0]] * 8, inv(S8),
          solved=True),
        E("curv1", se.CURV1, 1024, S3, 0, [0] * 3, 1, [[32]] * 3, [z2] * 3),
        # p.q == 0 in the SECOND iteration: k = 1, X the iterate of k = 1; a = 2,
        # rhon_s = 1 / (1 + 2 sigma_s) = 1, 1/5, 1/13 round, but reach only the
        # history and X (elementwise), which no sum reads
        E("curv2", se.CURV2, 512, S3, 1, [1] * 3, 1,
          [[32, 32 * r] for r in _R], [(2 * r, -2 * r, 0.0) for r in _R]),
        E("negative", neg, 512, S3, 0, [0] * 3, 1, [[32]] * 3, [z2] * 3),
        # sigma = 2^41 - 2 stops at step 1 (rhon = zeta = 2^-40 < rtol) with x =
        # 2^-41 b; sigma = 0 goes on and ends at k = 2 by rrn == 0
        E("early", EARLY, 1024, (0.0, EARLY_SIGMA), 2, [2, 1], 0,
          [[32, 16, 0], [32, 2.0 ** -36]], [(-1.0, 1.0), (0.0, 2.0 ** -41)],
          rtol=2.0 ** -30, solved=True),
        E("zero", (TWO_I[0], (0, 0)), 512, S3, 0, [0] * 3, 0, [[0]] * 3,
          [z2] * 3),
    ]


_R = (1.0, 1.0 / 5.0, 1.0 / 13.0)  # rhon_s of curv2, one rounding each

TWO_RANKS = ("curv2", "early")

# ---------------------------------------------------------------------------
# b. the floor of scaling
# ---------------------------------------------------------------------------
FLOOR_S = (520, -520, 540, -540)
FLOOR_CASES = ("two_i", "curv2")


def floor_case(case, s, tail):
    """-> (csr, b, shifts, want): every s repeats the row, X times 2^-s"""
    csr, b = case.system(tail)
    w = case.want(tail)
    return (scale_csr(csr, s), b, tuple(np.ldexp(case.shifts, s)),
            Result(np.ldexp(w.x, -s), w.k, w.its, w.hist, w.status))


# ---------------------------------------------------------------------------
# c. poisoned data
# ---------------------------------------------------------------------------
POISON_SHAPE = "poisson11"
STORAGES = (False, True)  # symmetric
POISON_SHIFTS, HUGE_SHIFTS = (0.0, 1.0, 4.0), (0.0, 1e300)
POISON_KMAX, POISON_RTOL = 12, 1e-10
KINDS = POISONS + ("huge_shift",)
# kind -> (k, status, hist[0] class, X is NaN everywhere (else 0; None: finite))
POISON_OUTCOME = {
    "b_nan": (0, 1, "nan", False),
    "b_inf": (0, 1, "inf", False),
    "a_nan": (0, 1, "finite", False),
    "b_huge": (1, 1, "inf", True),
    "b_tiny": (0, 0, 0.0, False),
    "huge_shift": (POISON_KMAX, 0, "finite", None),
}
WEAK = {(sym, "huge_shift") for sym in STORAGES}


def csr_of(shape=POISON_SHAPE):
    return me.csr_of(shape)


def poisoned_case(kind):
    """-> (csr, b, shifts)"""
    csr = csr_of()
    if kind == "huge_shift":
        return csr, clean_rhs(len(csr[0]) - 1), HUGE_SHIFTS
    (rp, ci, va), b = poisoned(csr, kind)
    if kind == "a_nan":  # at (i, j) AND (j, i): either storage reads one
        at = int(np.flatnonzero(np.isnan(va))[0])
        i, j = int(np.searchsorted(rp, at, side="right")) - 1, int(ci[at])
        va[rp[j] + int(np.flatnonzero(ci[rp[j]:rp[j + 1]] == i)[0])] = np.nan
    return (rp, ci, va), b, POISON_SHIFTS


def poisoned_reference(sym, kind, dot=DOT, ref=None):
    csr, b, shifts = poisoned_case(kind)
    return reference(csr, b, shifts, POISON_KMAX, POISON_RTOL, dot=dot, ref=ref,
                     symmetric=sym)


# ---------------------------------------------------------------------------
# d. scaled and negated systems
# ---------------------------------------------------------------------------
PAIRS = SCALES + ((300, 0),)
SCALED_KMAX, SCALED_RTOL = 60, se.SCALED_RTOL


def shifted_spmv(csr, sigma, x):
    """(A + sigma I) x by oracle.csr_spmv on the shifted matrix"""
    return oracle.csr_spmv(*cc.shifted(csr, sigma), x)
