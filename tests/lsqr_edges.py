"""Cases and references for whole lsqr solves on inputs that are not a benign
system: every exit on exact block matrices, the floor of scaling, non-finite
and overflowing data, and systems scaled by powers of two or negated.  Nothing
here touches a GPU: test_lsqr_edges_host.py holds this module to its claims on
the reference alone, test_gpu_lsqr_edges.py runs host.lsqr on it.  The
companion of solver_edges.py and minres_edges.py, whose poisons, scales, block
systems and dot products are imported.

The reference is lsqr_cases.lsqr_ref, imported, under np.errstate(all="ignore")
(`reference`), on oracle.csr_spmv of the matrix and of its stable transpose.
Its comparisons were read against cg.h and blas1_lsqr.hip, in the kernels'
order:
  update_v   `beta != 0` guards ib = 1 / beta (a NaN goes on and divides)
  start      `beta == 0` (status 0) comes first, then hist_ar[0] is written,
             then `alpha == 0` (status 2); ia = 1 / alpha and ib = 1 / beta
             follow both tests
  step       alpha_n = beta != 0 ? sqrt(vv) : 0; every scalar, k and both
             histories are written; then `beta == 0 or alpha_n == 0` (status
             2), `res / hist_r[0] < rtol`, `ares / (sqrt(anorm2) * res) < ltol`
             (status 1), `k + 1 == kmax`, in that order: a breakdown or the
             ltol stop that coincides with kmax keeps its status.  ia = 1 /
             alpha_n, ib = 1 / beta and t2 = theta / rho follow the zero test.
All four comparisons against a tolerance or zero are false on a NaN: a NaN never
stops a solve.  rhobar / rhobar1, damp / rhobar1 (rhobar1 = 0 only where rhobar
= damp = 0), rhobar1 / rho, beta / rho, phi / rho and res / hist_r[0] are NOT
guarded by a zero test of their own: the restatement divides through
lsqr_cases._div, IEEE's quotient, and takes its square roots through numpy, so
nothing raises.  lsqr_cases.py is unchanged.

a. EXACT cases: one small integer block (m x n) repeated NB times, with and
   without one tail row and column (entry 1, b = 0), NB a power of two such
   that beta = sqrt(b.b) = 32 and alpha = sqrt(vt.vt) is a power of two: ib and
   ia are exact, every element a small dyadic number, every sum one of equal
   dyadic terms.  sqrt(2) enters through rho = sqrt(rhobar1^2 + beta^2) in
   three rows; it reaches cs, sn, the histories and x (elementwise), which no
   sum reads.  At rtol = 0, kmax = 40 and again with kmax = the step of the
   exit; ltol = 0 but for the row `ltol`.  As measured on the reference:

     name       block              b          damp NB    rows x cols  k status
     alpha0     [[0,0],[0,1]]      (1,0)      0    1024  2048 x 2048  0  2
                A^T b = 0: hist_r (32), hist_ar (0), x = 0
     tall0      [[1],[1]]          (1,-1)     0     512  1024 x  512  0  2
     two_i      [[2,0],[0,2]]      (1,1)      0     512  1024 x 1024  1  2
                beta == 0 after one step: hist_r (32, 0), x = b / 2, A x = b
     tall4      [[1],[1],[1],[1]]  (1,1,1,1)  0     256  1024 x  256  1  2
                consistent: beta == 0, x = 1, A x = b.  (The 2 x 1 block of
                ones has alpha = sqrt(2) for every b in its range and any NB;
                an m x 1 block of ones has alpha^2 = m, and 4 is the first
                square.)
     tall_an0   [[1],[1]]          (1,0)      0    1024  2048 x 1024  1  2
                inconsistent: beta = 1 != 0 and alpha_n == 0 after one step;
                x = 1/2, the least-squares solution; hist_r (32, 32 / sqrt 2)
     wide4      [[1,1,1,1]]        (1)        0    1024  1024 x 4096  1  2
                the minimum-norm solution x = 1/4, A x = b.  ([[1,1]] has
                alpha = sqrt(2).)
     damped     [[2,0],[0,2]]      (1,1)      2     512  1024 x 1024  1  2
                x = 1/4 = A^T b / (A^T A + damp^2)
     ltol       [[0,1],[1,1]]      (1,0)      0    1024  2048 x 2048  1  1
                ltol = 1: beta = alpha_n = 1, no breakdown, the least-squares
                test stops the first step
     zero       [[2,0],[0,2]]      (0,0)      0     512  1024 x 1024  0  0
   With kmax = the step of the exit the outcome is the same row: the exit's
   status wins over the kmax stop (k = 0 rows: kmax = 0 is the start alone).

b. FLOOR: two_i and tall_an0 under scale_csr(s), t = 0, and the row `damped`
   with damp * 2^s.  vt is the UN-normalised vector 2^s (A^T b) / 32, so it is
   vt.vt = 2^(2s + 2) that leaves the range first.  FLOOR holds what the
   reference does, see there: NaN to kmax at s = 520 and 540, the unscaled row
   at -520, status 2 at k = 0 on a regular system at -540.

c. POISONED data: solver_edges.poisoned on convdiff11_2 (square, nonsymmetric,
   integer entries) and tall, kmax 12, rtol = ltol = 1e-10, and two poisons of
   damp on a clean system (`damp_rhs`: +-1 on 1024 rows, so that beta = 32 and
   hist_ar[0] is exact on the integer matrix).  POISON_OUTCOME, as measured:
     b_nan      k = 12, status 0, both histories all NaN, x all NaN
     b_inf      k = 12, status 0, hist_r (Inf, NaN, ...), x all NaN
     a_nan      k = 12, status 0, hist_r (finite, NaN, ...), x all NaN
     b_huge     k = 0, status 2: beta = Inf, ib = 0, vt = 0, alpha == 0;
                hist_r (Inf), hist_ar (NaN = 0 * Inf), x = 0
     b_tiny     k = 0, status 0, hist_r (0), x = 0 although b != 0
     damp_huge  damp = 1e200: damp * damp = Inf, rhobar1 = rho = Inf, cs1 = sn1
                = sn = 0 and cs = Inf / Inf: phibar = 0 and hist_r[1] = 0 pass
                the rtol test while phi is a NaN: k = 1, status 0, hist_r
                (finite, 0), hist_ar (finite, NaN), x all NaN -- a wrong answer
                that looks converged (cg.h says so)
     damp_tiny  damp = 1e-200: damp * damp and psi * psi underflow to 0 and
                rhobar1 = |rhobar|: the solve of damp = 0, bit for bit
   WEAK (held to `pattern`): damp_tiny on both shapes (twelve clean steps on
   data that rounds) and damp_huge on tall (hist_ar[0] rounds): 3 of 14.

d. SCALED systems (2^s A, 2^t b, damp * 2^s), PAIRS = solver_edges.SCALES,
   (300, 0) and (-400, -300), kmax 60, rtol = solver_edges.SCALED_RTOL, ltol =
   1e-10: x scales by 2^(t-s), hist_r by 2^t, hist_ar by 2^(s+t); k and status
   stay.  SCALED lists the solves; (tall, rand) ends by the ltol test.
   Negation: (A, -b) and (-A, b) both give -x and the same histories, bit for
   bit on the reference (ut or vt change sign, every norm is even)."""
import numpy as np

import lsqr_cases as lc
import solver_edges as se
from lsqr_cases import lsqr_ref  # noqa: F401  (the reference, not a copy)
from minres_edges import pattern as _pattern
from minres_edges import rank1_nan, tiled  # noqa: F401
from solver_edges import (DOT, POISONS, SCALES, _recording,  # noqa: F401
                          clean_rhs, dot_chunked, dot_reversed, poisoned,
                          same_bits, scale_csr)

ORDERS = (DOT, dot_reversed, dot_chunked)
KMAX = 40  # of every exact and floor case


class Result(se.Result):
    """solver_edges.Result with the second history"""

    def __init__(self, x, k, hist, hist_ar, status=0):
        super().__init__(x, k, hist, status)
        self.hist_ar = np.asarray(hist_ar, dtype=np.float64)

    def same(self, other):
        return super().same(other) and same_bits(self.hist_ar, other.hist_ar)


def pattern(r):
    return _pattern(r) + (np.isnan(r.hist_ar).tolist(),
                          np.isinf(r.hist_ar).tolist())


def reference(csr, ncols, b, kmax, rtol, ltol=0.0, damp=0.0, dot=DOT,
              record=None, ref=None):
    """lsqr_ref -> Result; record: a list that receives every operand and
    result of the products with A and of the dot products"""
    T = lc.stable_transpose(csr, ncols)
    spmv = se.spmv_of(csr)
    if record is not None:
        spmv, dot = _recording(spmv, dot, record)
    x, k, hr, har, status = (ref or lc.lsqr_ref)(
        spmv, se.spmv_of(T), dot, np.asarray(b, np.float64), kmax, rtol, ltol,
        damp)
    return Result(x, k, hr, har, status)


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
def rect_system(block, rhs, nb, tail):
    """tailed_system's rectangular sibling -> (csr, ncols, b): `nb` copies of
    the m x n block on the diagonal (zero entries are not stored); tail: one
    more row AND column, entry 1, b = 0"""
    m, n = len(block), len(block[0])
    rows, cols, vals = [], [], []
    for i in range(m):
        for j in range(n):
            if block[i][j] != 0:
                rows.append(i), cols.append(j), vals.append(float(block[i][j]))
    rows = (m * np.arange(nb)[:, None] + np.array(rows, int)[None, :]).reshape(-1)
    cols = (n * np.arange(nb)[:, None] + np.array(cols, int)[None, :]).reshape(-1)
    vals = np.tile(np.array(vals, float), nb)
    b = np.tile(np.array(rhs, dtype=np.float64), nb)
    M, N = m * nb, n * nb
    if tail:
        rows, cols = np.append(rows, M), np.append(cols, N)
        vals, b = np.append(vals, 1.0), np.append(b, 0.0)
        M, N = M + 1, N + 1
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))])
    return ((rp.astype(np.int32), cols[order].astype(np.int32), vals[order]),
            N, b)


class Exact:
    def __init__(self, name, block, rhs, nb, k, status, hist_r, hist_ar, x,
                 damp=0.0, ltol=0.0, solved=False):
        self.id = self.name = name
        self.block, self.rhs, self.nb = block, rhs, nb
        self.k, self.status, self.damp, self.ltol = k, status, damp, ltol
        self.hist = np.array(hist_r, np.float64)
        self.hist_ar = np.array(hist_ar, np.float64)
        self.xblock = np.array(x, np.float64)
        self.solved = solved  # A x == b, bit for bit
        self._sys = {}

    def system(self, tail):
        if tail not in self._sys:
            self._sys[tail] = rect_system(self.block, self.rhs, self.nb, tail)
        return self._sys[tail]

    def want(self, tail):
        return Result(tiled(self.xblock, self.nb, tail), self.k, self.hist,
                      self.hist_ar, self.status)

    def kmaxes(self):
        return (KMAX, self.k)


def exact_cases():
    E = Exact
    i2 = ((2, 0), (0, 2))
    return _filled([
        E("alpha0", ((0, 0), (0, 1)), (1, 0), 1024, 0, 2, [32], [0], (0, 0)),
        E("tall0", ((1,), (1,)), (1, -1), 512, 0, 2, [32], [0], (0,)),
        E("two_i", i2, (1, 1), 512, 1, 2, [32, 0], [64, 0], (.5, .5),
          solved=True),
        E("tall4", ((1,),) * 4, (1,) * 4, 256, 1, 2, [32, 0], [64, 0], (1,),
          solved=True),
        E("tall_an0", ((1,), (1,)), (1, 0), 1024, 1, 2, None, None, (.5,)),
        E("wide4", ((1, 1, 1, 1),), (1,), 1024, 1, 2, [32, 0], [64, 0],
          (.25,) * 4, solved=True),
        E("damped", i2, (1, 1), 512, 1, 2, None, None, None, damp=2.0),
        E("ltol", ((0, 1), (1, 1)), (1, 0), 1024, 1, 1, None, None, None,
          ltol=1.0),
        E("zero", i2, (0, 0), 512, 0, 0, [0], [0], (0, 0)),
    ])


# the rows that sqrt(2) or damp reaches: (hist_r, hist_ar, x per block) as the
# reference gives them, the same in every summation order (the host test)
_MEASURED = {
    "tall_an0": (["0x1.0000000000000p+5", "0x1.6a09e667f3bccp+4"],
                 ["0x1.0000000000000p+5", "0x0.0p+0"],
                 ["0x1.fffffffffffffp-2"]),
    "damped": (["0x1.0000000000000p+5", "0x1.6a09e667f3bccp+4"],
               ["0x1.0000000000000p+6", "0x0.0p+0"],
               ["0x1.fffffffffffffp-3", "0x1.fffffffffffffp-3"]),
    "ltol": (["0x1.0000000000000p+5", "0x1.6a09e667f3bccp+4"],
             ["0x1.0000000000000p+5", "0x1.ffffffffffffep+3"],
             ["0x0.0p+0", "0x1.fffffffffffffp-2"]),
}


def _filled(cases):
    for c in cases:
        if c.name in _MEASURED:
            hr, har, x = _MEASURED[c.name]
            c.hist = np.array([float.fromhex(v) for v in hr])
            c.hist_ar = np.array([float.fromhex(v) for v in har])
            c.xblock = np.array([float.fromhex(v) for v in x])
    return cases


# with the tail row; square, so that rows and columns share one map; the halo
# of `ltol` is not empty
TWO_RANKS = ("ltol", "two_i")

# ---------------------------------------------------------------------------
# b. the floor of scaling
# ---------------------------------------------------------------------------
FLOOR_S = (520, -520, 540, -540)
FLOOR_CASES = ("two_i", "tall_an0", "damped")
# s -> what every one of the three rows does there, as measured:
#   "nan"     vt = 2^s (A^T b) / 32 is finite but vt.vt overflows: alpha = Inf,
#             hist_ar[0] = Inf, ia = 0, and Inf * 0 makes every later scalar a
#             NaN: k = kmax = 40, status 0, x NaN (the tail row too)
#   "scaled"  vt.vt = 2^-1038 or 2^-1040 is subnormal but exact: the unscaled
#             row, x times 2^-s, hist_ar times 2^s
#   "alpha0"  vt.vt underflows to 0: alpha == 0, k = 0 and status 2 ("A^T b =
#             0") on a regular system, hist_r (32), hist_ar (0), x = 0
FLOOR = {520: "nan", 540: "nan", -520: "scaled", -540: "alpha0"}


def floor_case(case, s, tail):
    """-> (csr, ncols, b, damp, want) of one exact case under scale_csr(s)"""
    csr, ncols, b = case.system(tail)
    n, what = len(case.xblock), FLOOR[s]
    if what == "nan":
        nan = [np.nan] * KMAX
        want = Result(np.full(n * case.nb + int(tail), np.nan), KMAX,
                      [32.0] + nan, [np.inf] + nan, 0)
    elif what == "scaled":
        want = Result(tiled(np.ldexp(case.xblock, -s), case.nb, tail), case.k,
                      case.hist, np.ldexp(case.hist_ar, s), case.status)
    else:
        want = Result(tiled(np.zeros(n), case.nb, tail), 0, [32.0], [0.0], 2)
    return (scale_csr(csr, s), ncols, b, float(np.ldexp(case.damp, s)), want)


# ---------------------------------------------------------------------------
# c. poisoned data
# ---------------------------------------------------------------------------
POISON_SHAPES = ("convdiff11_2", "tall")
POISON_KMAX, POISON_RTOL, POISON_LTOL = 12, 1e-10, 1e-10
DAMP_POISONS = {"damp_huge": 1e200, "damp_tiny": 1e-200}
KINDS = POISONS + tuple(DAMP_POISONS)
# kind -> (k, status, hist_r[0] ("nan", "inf", "finite", 0.0), x is NaN
# everywhere (else +0.0 everywhere; None: a finite solve))
POISON_OUTCOME = {
    "b_nan": (POISON_KMAX, 0, "nan", True),
    "b_inf": (POISON_KMAX, 0, "inf", True),
    "a_nan": (POISON_KMAX, 0, "finite", True),
    "b_huge": (0, 2, "inf", False),
    "b_tiny": (0, 0, 0.0, False),
    "damp_huge": (1, 0, "finite", True),
    "damp_tiny": (POISON_KMAX, 0, "finite", None),
}
WEAK = {("convdiff11_2", "damp_tiny"), ("tall", "damp_tiny"),
        ("tall", "damp_huge")}


def csr_of(shape):
    return lc.csr_by_name(shape)


def damp_rhs(M):
    """+-1 on 1024 rows (every row of a shorter vector but the last ones, so
    that b.b is a power of four), 0 elsewhere"""
    n = 1024 if M >= 1024 else 256
    rng = np.random.default_rng(M + 9)
    b = np.zeros(M)
    b[rng.permutation(M)[:n]] = rng.choice([-1.0, 1.0], n)
    return b


def poisoned_case(shape, kind):
    """-> (csr, ncols, b, damp)"""
    csr, ncols = csr_of(shape)
    if kind in DAMP_POISONS:
        return csr, ncols, damp_rhs(len(csr[0]) - 1), DAMP_POISONS[kind]
    pc, b = poisoned(csr, kind)
    return pc, ncols, b, 0.0


def poisoned_reference(shape, kind, dot=DOT, ref=None):
    csr, ncols, b, damp = poisoned_case(shape, kind)
    return reference(csr, ncols, b, POISON_KMAX, POISON_RTOL, POISON_LTOL, damp,
                     dot=dot, ref=ref)


# ---------------------------------------------------------------------------
# d. scaled and negated systems
# ---------------------------------------------------------------------------
PAIRS = SCALES + ((300, 0), (-400, -300))
SCALED_KMAX, SCALED_RTOL, SCALED_LTOL = 60, se.SCALED_RTOL, 1e-10
# (shape, right-hand side of lsqr_cases.rhs, damp)
SCALED = (("convdiff11_2", "ones", 0.0), ("tall", "rand", 0.0),
          ("tall", "rand", 0.5), ("wide", "rand", 0.0))


def scaled_rhs(shape, kind):
    csr, _ = csr_of(shape)
    return lc.rhs(shape, kind, se.spmv_of(csr))
