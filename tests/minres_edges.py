"""Cases and references for whole minres solves on inputs that are not a benign
system: every exit on exact block matrices, the floor of scaling, non-finite
and overflowing data, and systems scaled by powers of two or negated.  Nothing
here touches a GPU: test_minres_edges_host.py holds this module to its claims
on the reference alone, test_gpu_minres_edges.py runs host.minres on it.  The
companion of solver_edges.py and gmres_edges.py, whose poisons, scales, block
systems and dot products are imported.

The reference is minres_cases.minres_ref, imported, under np.errstate(all=
"ignore") (`reference`).  Its comparisons were read against cg.h and
blas1_minres.hip, in the kernels' order: `ry < 0` (start and step; false on a
NaN, and it comes BEFORE the square root, so math.sqrt never sees a negative
number; sqrt of NaN, of Inf and of -0.0 return without raising), `beta1 == 0`,
`gamma == 0`, then -- after x, k and hist[k] are written -- `beta == 0` and the
stop `hist[k] / hist[0] < rtol` (false on a NaN: a NaN never stops a solve).
The scalar part works in Python floats, where x / 0.0 raises; the divisors and
the zero test that guards each:
    1 / beta1, hist[k] / hist[0]     beta1 == 0 (start)
    alfa / beta, beta / oldb,        beta == 0 of the step before (status 1: the
    1 / beta                         loop has ended); at k = 0 beta is beta1
    gbar / gamma, beta / gamma,      gamma == 0 (status 3)
    1 / gamma
An overflow gives Inf and Inf / Inf a NaN without an exception.  Nothing had to
be rewritten: minres_cases.py is unchanged.  test_minres_edges_host.py feeds
the recurrence negative, NaN, infinite and -0.0 `ry` directly.

a. EXACT cases: one small integer block repeated NB times (NB even; with and
   without one tail row, entry 1 and b = 0, so N is even and odd), NB chosen
   so that b.M^-1 b is a power of four: beta1 and 1 / beta1 are powers of two
   and every dot product is a sum of equal dyadic terms, exact in any order.
   EXACT_DINV = 0.5 everywhere halves b.M^-1 b, so NB doubles (sing3: halves, to
   keep N <= 4097, and beta1 = 16); x is unchanged, the history is that of the
   M^-1-norm.  At rtol = 0, kmax = 40 and again with kmax = the step of the
   exit, as measured on the reference:

     name     block                 b        dinv      NB    N     k status
     two_i    [[2,0],[0,2]]         (1,1)    -         512  1024(+1)  1  1
              hist (32, 0), x = (0.5, 0.5)
     perm     [[0,1],[1,0]]         (1,0)    -        1024  2048  2  1
              alfa == 0 twice; hist (32, 32, 0), x = (0, 1)
     indef    [[1,0],[0,-1]]        (1,1)    -         512  1024  2  1
              indefinite; hist (32, 32, 0), x = (1, -1)
     sing3    [[0,1,0],[1,0,1],     (1,0,0)  -        1024  3072  2  3
               [0,1,0]]             singular, b outside the range: the third
              step finds beta == 0 and gbar == 0, gamma == 0; hist (32, 32,
              H_R2), x = (0, X_R2, 0) kept from the two steps taken
     two_i-d  as two_i              dinv 0.5          1024  2048  1  1   (32, 0)
     perm-d   as perm               dinv 0.5          2048  4096  2  1   (32, 32, 0)
     indef-d  as indef              dinv 0.5          1024  2048  2  1   (32, 32, 0)
     sing3-d  as sing3              dinv 0.5           512  1536  2  3   (16, 16, H_R2 / 2)
     neg0     [[2,0],[0,2]]         (1,1)    (1,-2)    512  1024  0  2
              ry < 0 in start: hist (0) (hist[0] is never written), x = 0
     neg1     [[0,0,1],[0,1,1],     (0,1,0)  (-1,1,1) 1024  3072  1  2
               [1,1,0]]             ry < 0 after ONE step (search_negative, a
              brute-force search in Fraction arithmetic over the symmetric
              blocks, first hit with a first step that moves x): hist (32,
              H_R2), x = (0, X_R2, 0), the iterate of k = 1
   H_R2 = 0x1.6a09e667f3bccp+4 (32 / sqrt 2 rounded through gamma = sqrt(2048))
   and X_R2 = 0.5 - 2^-53: sqrt(2) reaches only hist, w and x, which no sum
   reads, so these rows too have the same bits in every order.  With kmax = the
   step of the exit (k for status 1, k + 1 for status 2 and 3, 0 for neg0) the
   outcome is the same row: the breakdown wins over the kmax stop.

b. FLOOR: two_i and perm (and their -d rows with dinv = 0.5 * 2^-s) under
   scale_csr(s), t = 0.  As measured on the reference, without a preconditioner:
     s = +520, +540  two_i  gbar^2 = 2^1042 overflows, gamma = Inf, beta == 0:
                            cs = sn = phi = 0: k = 1, status 1, hist (32, 0)
                            and x = 0 -- a wrong answer that looks converged
                     perm   ry overflows, beta = Inf: sn = Inf / Inf, NaN history to
                            kmax = 40, status 0, x NaN (the tail row too)
     s = -520        both   gbar^2 = 2^-1038 or beta^2 = 2^-1040 (from products
                            of 2^-1050) are subnormal but exact: the unscaled
                            row, x times 2^520
     s = -540        both   gbar^2 + beta^2 underflows to 0: gamma == 0, k = 0,
                            status 3, hist (32), x = 0
   With the scaled dinv every s gives the unscaled row, the history times
   2^(-s/2) and x times 2^-s.  Every sum has equal terms: the device is held to
   these bits.

c. POISONED data: solver_edges.poisoned on shift11 and saddle500 (its integer
   right-hand side, clean_rhs), kmax 12, rtol 1e-10, without a preconditioner
   and with dinv_by_name (of the clean matrix).  POISON_OUTCOME, as measured:
     b_nan   k = 12, status 0, hist all NaN, x all NaN
     b_inf   k = 12, status 0, hist (Inf, NaN, ...), x all NaN
     a_nan   k = 12, status 0, hist (finite, NaN, ...), x all NaN
     b_huge  k = 0, status 3, hist (Inf), x = 0: v = b * (1 / Inf) = 0
     b_tiny  k = 0, status 0, hist (0), x = 0 although b != 0: the start stops
             on beta1 == 0 (cg.h says so)
   The three summation orders agree bit for bit on all of them but a_nan with
   Jacobi (WEAK), whose finite hist[0] = sqrt(sum dinv b^2) moves with the
   order: that one is compared on k, status and the NaN / Inf pattern of hist
   and x (`pattern`).

d. SCALED systems (2^s A, 2^t b), PAIRS = solver_edges.SCALES, (300, 0) and
   (-400, -300), kmax 60, rtol = solver_edges.SCALED_RTOL, on shift11 (general
   and symmetric storage; none, Jacobi), saddle500 (none, Jacobi) and poisson11
   (none, Jacobi, SGS, ILU(0), AMG); Jacobi is dinv_by_name * 2^-s, the others
   are built from the scaled matrix.  x scales by 2^(t-s); the history by 2^t
   without a preconditioner and by 2^(t - s/2) with one (`hist_exponent`; every
   s is even).  Inside a preconditioned solve v carries 2^(-s/2), Av and r2
   2^(s/2); alfa, beta (from k = 1), gamma, cs and sn do not scale.  Without
   one r2 and beta carry 2^s from k = 1 (2^-800 in ry at s = -400).  At ODD_S =
   101 with Jacobi sqrt(ry) picks up a sqrt(2) and NO power of two carries one
   history into the other.  shift11 and saddle500 run all 60 steps (6e-5 and
   1e-4 of hist[0]), poisson11 converges in 42, 42, 22, 22 and 11.
   Negation: (A, -b) gives -x and the same history.  (-A, b) with the positive
   dinv left alone gives -x and the same history too, bit for bit on the
   reference (alfa, gbar and every second Lanczos vector change sign, which is
   exact): included for none and Jacobi; SGS, ILU(0) and AMG refuse a negative
   diagonal.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

import gmres_cases as gc
import ilu0_cases as ic
import minres_cases as mc
import oracle
import solver_edges as se
from minres_cases import minres_ref  # noqa: F401  (the reference, not a copy)
from solver_edges import (DOT, POISONS, SCALES, Result, _recording,  # noqa: F401
                          block_system, clean_rhs, dot_chunked, dot_reversed,
                          poisoned, same_bits, scale_csr, scaled_rhs)

ORDERS = (DOT, dot_reversed, dot_chunked)
KMAX = 40  # of every exact and floor case


def reference(csr, b, kmax, rtol, minv=None, dot=DOT, record=None, spmv=None):
    """minres_ref -> Result; record: a list that receives every operand and
    result of the SpMVs and dot products (solver_edges._recording); spmv:
    another product than oracle.csr_spmv on `csr` (symmetric storage)"""
    spmv = spmv or se.spmv_of(csr)
    if record is not None:
        spmv, dot = _recording(spmv, dot, record)
    with np.errstate(all="ignore"):
        x, k, hist, status = mc.minres_ref(spmv, dot, minv,
                                           np.asarray(b, np.float64), kmax, rtol)
    return Result(x, k, hist, status)


def jacobi(dinv):
    return lambda q: dinv * q


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
TWO_I = (((2, 0), (0, 2)), (1, 1))
PERM = (((0, 1), (1, 0)), (1, 0))
INDEF = (((1, 0), (0, -1)), (1, 1))
SING3 = (((0, 1, 0), (1, 0, 1), (0, 1, 0)), (1, 0, 0))


def tiled(block_vec, nb, tail, tail_value=0.0):
    v = np.tile(np.array(block_vec, dtype=np.float64), nb)
    return np.append(v, tail_value) if tail else v


def tailed_system(block, rhs, nb, tail):
    """-> (csr, b): `nb` copies of the block on the diagonal (zero entries are
    not stored); tail: one more row, entry 1, b = 0.  Every NB here is even, so
    solver_edges.block_system always adds the tail row: without it, that row is
    cut off again."""
    assert nb % 2 == 0
    (rp, ci, va), b = block_system(block, rhs, nb)
    if not tail:
        rp, ci, va, b = rp[:-1], ci[:-1], va[:-1], b[:-1]
    assert len(b) == len(block) * nb + int(tail) and rp[-1] == len(ci)
    return (np.ascontiguousarray(rp), np.ascontiguousarray(ci),
            np.ascontiguousarray(va)), np.ascontiguousarray(b)


class Exact:
    """One row of the table: the block, its right-hand side, dinv per block (or
    None), the number of blocks and what the reference must return at rtol = 0,
    kmax = KMAX."""

    def __init__(self, name, system, dinv, nb, k, status, hist, x):
        self.id = self.name = name
        self.block, self.rhs = system
        self.dinv_block, self.nb = dinv, nb
        self.k, self.status = k, status
        self.hist = np.array(hist, np.float64)
        self.xblock = np.array(x, np.float64)
        self._sys = {}

    def system(self, tail):
        if tail not in self._sys:
            self._sys[tail] = tailed_system(self.block, self.rhs, self.nb, tail)
        return self._sys[tail]

    def dinv(self, tail):
        """the tail row's entry is 1 (its b is 0: it adds nothing to any sum)"""
        if self.dinv_block is None:
            return None
        return tiled(self.dinv_block, self.nb, tail, 1.0)

    def minv(self, tail):
        d = self.dinv(tail)
        return None if d is None else jacobi(d)

    def want(self, tail):
        return Result(tiled(self.xblock, self.nb, tail), self.k, self.hist,
                      self.status)

    def kmaxes(self):
        """KMAX, and the step of the exit: the kmax stop and the exit coincide
        (status 2 and 3 leave in the step AFTER the k completed ones)"""
        at = self.k if self.status in (0, 1) or self.k == 0 else self.k + 1
        return (KMAX, at)


# the exact search for the second status-2 case -----------------------------------
def _pow2(q):
    """q = 2^e: q and 1 / q are floats, and multiplying by either is exact"""
    a, b = q.numerator, q.denominator
    return a > 0 and a & (a - 1) == 0 and b & (b - 1) == 0


def _sqrt(q):
    a, b = q.numerator, q.denominator
    ra, rb = math.isqrt(a), math.isqrt(b)
    return Fraction(ra, rb) if ra * ra == a and rb * rb == b else None


def simulate_lanczos(A, b, dinv, nb, kmax=4):
    """The Lanczos part of minres (all that ry depends on: alfa, beta, r1, r2,
    v) on `nb` copies of one symmetric block in Fraction arithmetic -> k >= 1
    when ry < 0 first AFTER k completed steps; None when that does not happen,
    A is not symmetric, or a beta on the way is not a power of two (v = y * (1 /
    beta), alfa / beta and beta / oldb would round)."""
    n = len(b)
    if any(A[i][j] != A[j][i] for i in range(n) for j in range(i)):
        return None
    r1 = r2 = [Fraction(v) for v in b]
    y = [d * v for d, v in zip(dinv, r2)]
    ry = nb * se._dot(r2, y)
    if ry <= 0:
        return None
    beta, oldb = _sqrt(ry), None
    for k in range(kmax):
        if beta is None or not _pow2(beta):
            return None
        v = [q / beta for q in y]
        Av = se._mv(A, v)
        alfa = nb * se._dot(v, Av)
        if k == 0 and alfa == 0:  # cs = 0, phi = 0: the first step leaves x at 0
            return None
        t = [p - (alfa / beta) * q for p, q in zip(Av, r2)]
        if k > 0:
            t = [p - (beta / oldb) * q for p, q in zip(t, r1)]
        r1, r2 = r2, t
        y = [d * v for d, v in zip(dinv, r2)]
        ry = nb * se._dot(r2, y)
        if ry < 0:
            return k if k >= 1 else None
        if ry == 0:
            return None
        oldb, beta = beta, _sqrt(ry)
    return None


SEARCH_NB = {2: (1024, 512), 3: (1024, 512)}  # N <= 4097; both parities of log2


def search_negative(n):
    """The first symmetric n x n block, right-hand side, dinv in {1, -1}^n (not
    all positive) and NB of SEARCH_NB, in the order of itertools.product over
    solver_edges.ORDER5 (n = 2) or ORDER3 (n = 3), with ry < 0 first at k >= 1
    -> (A, b, dinv, nb, k) or None"""
    vals = se.ORDER5 if n == 2 else se.ORDER3
    for ent in itertools.product(vals, repeat=n * n):
        A = tuple(ent[i * n:(i + 1) * n] for i in range(n))
        for b in itertools.product(vals, repeat=n):
            for dinv in itertools.product((1, -1), repeat=n):
                for nb in SEARCH_NB[n]:
                    k = simulate_lanczos(A, b, dinv, nb)
                    if k is not None:
                        return A, b, dinv, nb, k
    return None


NEG1 = (((0, 0, 1), (0, 1, 1), (1, 1, 0)), (0, 1, 0))  # search_negative(3)
NEG1_DINV, NEG1_NB = (-1, 1, 1), 1024
EXACT_DINV = 0.5
# sqrt(2) enters two rows through gamma = sqrt(32^2 + 32^2): hist[2] and x are
# then roundings of 32 / sqrt(2) and 0.5, the same in every order because no sum
# ever sees them (x and w are elementwise; the next v is y / 32)
H_R2 = float.fromhex("0x1.6a09e667f3bccp+4")  # 32 / sqrt(2), one ulp below
X_R2 = float.fromhex("0x1.ffffffffffffep-2")  # 0.5 - 2^-53


def exact_cases():
    E, h, d2, d3 = Exact, EXACT_DINV, (EXACT_DINV,) * 2, (EXACT_DINV,) * 3
    return [
        # name, (block, b), dinv per block, NB, k, status, history, x per block
        E("two_i", TWO_I, None, 512, 1, 1, [32, 0], (h, h)),
        E("perm", PERM, None, 1024, 2, 1, [32, 32, 0], (0, 1)),
        E("indef", INDEF, None, 512, 2, 1, [32, 32, 0], (1, -1)),
        E("sing3", SING3, None, 1024, 2, 3, [32, 32, H_R2], (0, X_R2, 0)),
        # dinv = 0.5: b.M^-1 b = b.b / 2, NB doubled (sing3: halved, N <= 4097)
        E("two_i-d", TWO_I, d2, 1024, 1, 1, [32, 0], (h, h)),
        E("perm-d", PERM, d2, 2048, 2, 1, [32, 32, 0], (0, 1)),
        E("indef-d", INDEF, d2, 1024, 2, 1, [32, 32, 0], (1, -1)),
        E("sing3-d", SING3, d3, 512, 2, 3, [16, 16, H_R2 / 2], (0, X_R2, 0)),
        # status 2: b.M^-1 b = 512 * (1 - 2) at the start, hist[0] is not written
        E("neg0", TWO_I, (1, -2), 512, 0, 2, [0], (0, 0)),
        # status 2 after one step (search_negative)
        E("neg1", NEG1, NEG1_DINV, NEG1_NB, 1, 2, [32, H_R2], (0, X_R2, 0)),
    ]


TWO_RANKS = ("perm", "sing3")  # with the tail row

# ---------------------------------------------------------------------------
# b. the floor of scaling, on exact cases
# ---------------------------------------------------------------------------
FLOOR_S = (520, -520, 540, -540)
FLOOR_CASES = ("two_i", "perm")  # and their -d rows, dinv = 0.5 * 2^-s
# (name, s) -> (k, status, history, x per block); an "-d" row that is not listed
# is its unscaled row with the history times 2^(-s/2) and x times 2^-s
_NAN_RUN = (KMAX, 0, [32.0] + [np.nan] * KMAX, (np.nan, np.nan))
FLOOR = {
    # gbar^2 = alfa^2 overflows, gamma = Inf.  beta == 0: cs = sn = phi = 0, the
    # step is "converged" (status 1, hist[1] = 0) with x left at 0 -- WRONG, and
    # nothing says so; beta != 0 is also Inf: sn = Inf / Inf = NaN to kmax
    ("two_i", 520): (1, 1, [32, 0], (0, 0)),
    ("two_i", 540): (1, 1, [32, 0], (0, 0)),
    ("perm", 520): _NAN_RUN,
    ("perm", 540): _NAN_RUN,
    # 2^-1038 and 2^-1050 are subnormal but exact: the unscaled outcome
    ("two_i", -520): (1, 1, [32, 0], (2.0 ** 519, 2.0 ** 519)),
    ("perm", -520): (2, 1, [32, 32, 0], (0, 2.0 ** 520)),
    # gbar^2 + beta^2 underflows to 0: gamma == 0, status 3 before any step
    ("two_i", -540): (0, 3, [32], (0, 0)),
    ("perm", -540): (0, 3, [32], (0, 0)),
}


def floor_case(case, s, tail):
    """-> (csr, b, dinv or None, want) of one exact case under scale_csr(s)"""
    csr, b = case.system(tail)
    d = case.dinv(tail)
    if d is None:
        k, status, hist, xb = FLOOR[(case.name, s)]
    else:
        d = np.ldexp(d, -s)
        k, status = case.k, case.status
        hist, xb = np.ldexp(case.hist, -s // 2), np.ldexp(case.xblock, -s)
    x_tail = np.nan if np.any(np.isnan(xb)) else 0.0  # NaN * 0: the tail row too
    return (scale_csr(csr, s), b, d,
            Result(tiled(xb, case.nb, tail, x_tail), k, hist, status))


# ---------------------------------------------------------------------------
# c. poisoned data
# ---------------------------------------------------------------------------
POISON_SHAPES = ("shift11", "saddle500")
POISON_KMAX, POISON_RTOL = 12, 1e-10
PRE_POISON = ("none", "jacobi")
# kind -> (k is kmax, status, hist[0] ("nan", "inf", "finite", 0.0), x is NaN
# everywhere (else +0.0 everywhere)); hist[1:] is NaN wherever it exists
POISON_OUTCOME = {
    "b_nan": (True, 0, "nan", True),
    "b_inf": (True, 0, "inf", True),
    "a_nan": (True, 0, "finite", True),
    # beta1 = Inf, v = b * 0 = 0, alfa = 0, r2 = 0 - (0 / Inf) * b = 0: beta = 0
    # and gbar = 0, gamma == 0 in the first step
    "b_huge": (False, 3, "inf", False),
    "b_tiny": (False, 0, 0.0, False),  # b.b underflows to 0: the start stops
}
# held to the reference's bits on the device; the rest (a_nan with Jacobi, where
# hist[0] = sqrt(sum dinv b^2) moves with the order) to (k, status, the pattern)
WEAK = {(shape, "a_nan", "jacobi") for shape in POISON_SHAPES}

_CSR = {}


def csr_of(shape):
    if shape not in _CSR:
        _CSR[shape] = mc.csr_by_name(shape)
    return _CSR[shape]


def pattern(r):
    """what a weak comparison looks at"""
    return (r.k, r.status, len(r.hist), np.isnan(r.hist).tolist(),
            np.isinf(r.hist).tolist(), np.isnan(r.x).tolist(),
            np.isinf(r.x).tolist())


def rank1_nan(N):
    """b_nan for two ranks: the NaN in the second slab only"""
    b = clean_rhs(N)
    cut = int(oracle.owner_ranges(2, N)[1])
    b[(cut + N) // 2] = np.nan
    return b


# ---------------------------------------------------------------------------
# d. scaled and negated systems
# ---------------------------------------------------------------------------
PAIRS = SCALES + ((300, 0), (-400, -300))
ODD_S = 101
SCALED_KMAX, SCALED_RTOL = 60, se.SCALED_RTOL
# shape -> the preconditioners; shift11 also in symmetric storage
SCALED = {"shift11": ("none", "jacobi"), "saddle500": ("none", "jacobi"),
          "poisson11": ("none", "jacobi", "sgs", "ilu0", "amg")}
SYMMETRIC = ("shift11",)
NEGATED_A = ("none", "jacobi")  # SGS, ILU(0) and AMG refuse a negative diagonal


def hist_exponent(pre, s, t):
    return t if pre == "none" else t - s // 2


def spmv_of(csr, symmetric=False):
    if not symmetric:
        return se.spmv_of(csr)
    lrp, lci, lva, diag = mc.lower_csr(csr)
    return lambda v: oracle.csr_spmv_sym(lrp, lci, lva, diag,
                                         np.ascontiguousarray(v))


def minv_of(pre, shape, s=0):
    """the reference's M^-1 for 2^s * csr_of(shape): Jacobi is dinv_by_name
    times 2^-s (and is NOT negated with A: M stays positive definite); SGS,
    ILU(0) and AMG are built from the scaled matrix"""
    csr = csr_of(shape)
    A = scale_csr(csr, s)
    N = len(csr[0]) - 1
    if pre == "none":
        return None
    if pre == "jacobi":
        return jacobi(np.ldexp(mc.dinv_by_name(shape), -s))
    if pre == "sgs":
        return gc.SgsRef(A)
    if pre == "ilu0":
        ref = ic.Ilu0Ref(A, N, ic.greedy_colours(A, N), False)
        fac = ref.factor()
        return lambda r: ref.apply(fac, r)
    if pre == "amg":
        import test_gpu_amg as ta
        return ta.restate(A, N, False).apply
    raise ValueError(pre)
