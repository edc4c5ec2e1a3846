"""Cases and references for whole gmres solves on inputs that are not a benign
system: breakdowns and stagnation on exact matrices, non-finite and overflowing
data, and systems scaled by powers of two or negated.  Nothing here touches a
GPU: test_gmres_edges_host.py holds this module to its claims on the reference
alone, test_gpu_gmres_edges.py runs host.gmres on it.  The companion of
solver_edges.py, whose poisons, scales and dot products are imported.

The reference is gmres_cases.gmres_ref, imported, under np.errstate(all=
"ignore") with a dot product that returns np.float64 (`reference`).  Its
comparisons were read against cg.h and blas1_gmres.hip: the stop test is `res /
hist[0] < rtol` (false on NaN: a NaN never stops a solve), the pivot, breakdown
and r.r tests are `== 0`, the rotation's branches are taken in the kernel's
order (`b == 0`, then `|b| > |a|`, which is false on a NaN).  None had to be
rewritten.  The scalar part works in Python floats, where x / 0.0 raises: the
divisors are b (after `b == 0` and `|b| > |a|`), a (the else branch: a == 0
there needs b NaN and a zero, which no case produces), sqrt(1 + tau^2) >= 1,
beta and hn (both after their `== 0` tests), hist[0] (after rr0 == 0) and R_ii
(a kept column has R_ii != 0).  That no case reaches a zero divisor is shown by
running them: every reference of the host test completes, and a zero divisor
would have raised.

a. EXACT cases: one small 0/1 block (TWO_I: 2 I) repeated NB times, one nonzero
   of b per block (TWO_I: two) and NB chosen so that b.b = 1024: beta = 32 and
   1 / beta are powers of two, every basis vector is a column of the identity
   over the blocks divided by 32, every rotation is (0, 1) or (1, 0), and every
   dot product is a sum of equal dyadic terms, exact in any order.  `EXACT`
   lists (k, status, history, x per block) at rtol = 0, kmax = 40; which exit
   of which kernel a row reaches:

     perm   restart 30   hn == 0 at j = 1 (givens, status 1)
            restart 2    the same on the LAST step of a cycle (no scale kernel)
            restart 1    stagnation: every cycle keeps jn = 1 column with y == 0,
                         x stays +0.0, r.r is never 0, the solve ends on kmax
     nil    restart 30   R_00 == 0 (givens, status 2) with jn == 0: solve_y,
                         combine and add have nothing to do
     shift3 restart 30   R_22 == 0 (status 2) with jn == 2: x is formed from the
                         two columns kept (y == 0, -0.0: x == +0.0)
            restart 3    the same on the last step of a cycle
            restart 2    stagnation with jn = 2
     cyc3   restart 30   hn == 0 at j = 2 (status 1), x from three columns
            restart 3    the same on the last step of a cycle
            restart 2    stagnation with jn = 2
     two_i  restart 30   hn == 0 at j = 0 with x = b / 2 (test_gpu_gmres.py has
                         A = I only)

   Every case also runs with one tail row (entry 1, b = 0: N odd) and with the
   right preconditioner dinv = 0.5 (h and R halve, y doubles, x and the history
   are unchanged: the same table).

   r.r == 0 in a LATER cycle with a positive history (the stop of the start
   kernel outside the first cycle).  A right-hand side scaled by 2^-490 on the
   blocks above does not give one: a rotation with dyadic c and s is (0, +-1) or
   (+-1, 0), so on an exact case a step leaves the residual as it is or
   removes it, and a residual that is removed is an exact 0 with hist[k] == 0.
   A case that is not exact in this sense exists where every sum has at most
   two nonzero terms, so that it is still the same in any order: UNDER, the
   2 x 2 matrix [[1, 2^-40], [0, 1]] with b = 2^-505 (1, 1) at restart 1.  One
   step leaves a residual of about 2^-546 per element: hist[1] is positive and
   normal, every r_i * r_i underflows to +0, r.r == 0 and the second cycle
   stops in the start kernel with k = 1, status 0.

b. POISONED data: solver_edges.poisoned on convdiff11 and banded4097, kmax 12,
   rtol 1e-10, restarts 5 and 30, without a preconditioner and with Jacobi's
   dinv (of the clean matrix).  What the reference does is in POISON_OUTCOME.

c. SCALED systems (2^s A, 2^t b) with solver_edges.SCALES, and the negated (-A,
   b) and (A, -b), for no preconditioner, Jacobi's dinv (times 2^-s, negated
   with A), SGS, ILU(0) and Chebyshev of degree 3 (dinv left alone, lmin and
   lmax times 2^s).  The basis vectors are normalised, so they do not scale at
   all; beta, g, the history and y scale by 2^t, h and R by 2^s without a
   preconditioner, x by 2^(t - s).  kmax = 60 and rtol = SCALED_RTOL, at which
   every unscaled combination converges in 5 to 49 steps on the reference
   (convdiff11 at restart 5 without a preconditioner: 49, nine restarts; it
   does not reach 1e-8 in 60).  None of the four pairs had to shrink.

   ILU(0) under scaling: the stored factor is (l~, u~, d~) of (D~ + L~) D~^-1
   (D~ + U~), whose entries all scale with A; the multipliers of the
   elimination, l~_ik * (1 / d~_k), do not.  `ilu0_multipliers` forms them.
"""
import math

import numpy as np

import gmres_cases as gc
import ilu0_cases as ic
import oracle
import solver_edges as se
from solver_edges import (DOT, POISONS, SCALES, Result, clean_rhs,  # noqa: F401
                          dot_chunked, dot_reversed, poisoned, same_bits,
                          scale_csr, scaled_rhs)

ORDERS = (DOT, dot_reversed, dot_chunked)
KMAX = 40  # of every exact case


def reference(csr, b, m, kmax, rtol, minv=None, dot=DOT, record=None):
    """gmres_ref -> Result; record: a list that receives every operand and
    result of the SpMVs and dot products (solver_edges._recording)"""
    spmv = se.spmv_of(csr)
    if record is not None:
        spmv, dot = se._recording(spmv, dot, record)
    with np.errstate(all="ignore"):
        x, k, hist, status = gc.gmres_ref(spmv, dot, minv,
                                          np.asarray(b, np.float64), m, kmax,
                                          rtol)
    return Result(x, k, hist, status)


def jacobi(dinv):
    return lambda q: dinv * q


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
PERM = (((0, 1), (1, 0)), (1, 0))
NIL = (((0, 1), (0, 0)), (1, 0))
SHIFT3 = (((0, 0, 0), (1, 0, 0), (0, 1, 0)), (1, 0, 0))
CYC3 = (((0, 0, 1), (1, 0, 0), (0, 1, 0)), (1, 0, 0))
TWO_I = (((2, 0), (0, 2)), (1, 1))


def block_system(block, rhs, nb, tail):
    """-> (csr, b): `nb` copies of the block on the diagonal (zero entries are
    not stored; a row may be empty); tail: one more row, entry 1, b = 0"""
    n = len(block)
    at = [(i, j) for i in range(n) for j in range(n) if block[i][j] != 0]
    base = n * np.arange(nb)[:, None]
    rows = (base + np.array([i for i, _ in at])[None, :]).reshape(-1)
    cols = (base + np.array([j for _, j in at])[None, :]).reshape(-1)
    vals = np.tile(np.array([float(block[i][j]) for i, j in at]), nb)
    b = np.tile(np.array(rhs, dtype=np.float64), nb)
    N = n * nb
    if tail:
        rows, cols = np.append(rows, N), np.append(cols, N)
        vals, b = np.append(vals, 1.0), np.append(b, 0.0)
        N += 1
    return gc.to_csr(N, [rows], [cols], [vals]), b


class Exact:
    """One row of the table: the block, its right-hand side, the number of
    blocks, the restart and what the reference must return at rtol = 0, kmax =
    KMAX."""

    def __init__(self, name, system, nb, restart, k, status, hist, x):
        self.name, self.restart = name, restart
        self.id = f"{name}-m{restart}"
        self.block, self.rhs = system
        self.nb, self.k, self.status = nb, k, status
        self.hist = np.array(hist, np.float64)
        self.xblock = np.array(x, np.float64)
        self._sys = {}

    def system(self, tail):
        if tail not in self._sys:
            self._sys[tail] = block_system(self.block, self.rhs, self.nb, tail)
        return self._sys[tail]

    def x(self, tail):
        x = np.tile(self.xblock, self.nb)
        return np.append(x, 0.0) if tail else x

    def want(self, tail):
        return Result(self.x(tail), self.k, self.hist, self.status)


def exact_cases():
    E, stag = Exact, [32.0] * (KMAX + 1)
    return [
        # name, (block, b), NB, restart, k, status, history, x per block
        E("perm", PERM, 1024, 30, 2, 1, [32, 32, 0], (0, 1)),
        E("perm", PERM, 1024, 2, 2, 1, [32, 32, 0], (0, 1)),
        E("perm", PERM, 1024, 1, KMAX, 0, stag, (0, 0)),
        E("nil", NIL, 1024, 30, 0, 2, [32], (0, 0)),
        E("shift3", SHIFT3, 1024, 30, 2, 2, [32, 32, 32], (0, 0, 0)),
        E("shift3", SHIFT3, 1024, 3, 2, 2, [32, 32, 32], (0, 0, 0)),
        E("shift3", SHIFT3, 1024, 2, KMAX, 0, stag, (0, 0, 0)),
        E("cyc3", CYC3, 1024, 30, 3, 1, [32, 32, 32, 0], (0, 0, 1)),
        E("cyc3", CYC3, 1024, 3, 3, 1, [32, 32, 32, 0], (0, 0, 1)),
        E("cyc3", CYC3, 1024, 2, KMAX, 0, stag, (0, 0, 0)),
        E("two_i", TWO_I, 512, 30, 1, 1, [32, 0], (0.5, 0.5)),
    ]


EXACT_DINV = 0.5  # the right preconditioner of the exact cases: all 0.5
TWO_RANKS = ("perm", "shift3", "cyc3")  # at restart 30, with the tail row


def under_case(tail):
    """UNDER (see the top) -> (csr, b, restart, kmax): r.r == 0 at the start of
    the second cycle"""
    e = 2.0 ** -40
    rows, cols, vals = [0, 0, 1], [0, 1, 1], [1.0, e, 1.0]
    b = [2.0 ** -505, 2.0 ** -505]
    if tail:
        rows, cols, vals, b = rows + [2], cols + [2], vals + [1.0], b + [0.0]
    n = len(b)
    csr = gc.to_csr(n, [np.array(rows)], [np.array(cols)], [np.array(vals)])
    return csr, np.array(b), 1, KMAX


# ---------------------------------------------------------------------------
# b. poisoned data
# ---------------------------------------------------------------------------
SHAPES = ("convdiff11", "banded4097")
RESTARTS = (5, 30)
POISON_KMAX, POISON_RTOL = 12, 1e-10
PRE_POISON = ("none", "jacobi")
# kind -> (k is kmax, status, hist[0] ("nan", "inf", "exact", 0.0), x is NaN)
POISON_OUTCOME = {
    "b_nan": (True, 0, "nan", True),
    "b_inf": (True, 0, "inf", True),
    "a_nan": (True, 0, "exact", True),
    "b_huge": (False, 2, "inf", False),  # 1 / beta == 0: v_0 == 0, R_00 == 0
    "b_tiny": (False, 0, 0.0, False),    # b.b underflows to 0
}

_CSR = {}


def csr_of(shape):
    if shape not in _CSR:
        _CSR[shape] = gc.csr_by_name(shape)
    return _CSR[shape]


def jacobi_dinv(csr):
    return 1.0 / gc.diag_of(csr)


# ---------------------------------------------------------------------------
# c. scaled and negated systems
# ---------------------------------------------------------------------------
PRECONDITIONERS = ("none", "jacobi", "sgs", "ilu0", "cheb")
NEGATED_A = ("none", "jacobi")  # SGS and ILU(0) refuse a negative diagonal
CHEB = se.CHEB                  # (3, LMIN, LMAX) of test_gpu_chebyshev.py
SCALED_KMAX, SCALED_RTOL = 60, 1e-6
ILU_SHAPES = ("poisson11", "convdiff8")
ILU_SCALES = (100, -100)


def minv_of(pre, csr, s=0, sign=1.0):
    """the reference's M^-1 for the matrix sign * 2^s * csr (csr unscaled)"""
    A = scale_csr(csr, s, sign)
    N = len(csr[0]) - 1
    if pre == "none":
        return None
    if pre == "jacobi":
        return jacobi(sign * np.ldexp(jacobi_dinv(csr), -s))
    if pre == "sgs":
        return gc.SgsRef(A)
    if pre == "ilu0":
        ref = ic.Ilu0Ref(A, N, ic.greedy_colours(A, N), False)
        fac = ref.factor()
        return lambda r: ref.apply(fac, r)
    if pre == "cheb":
        degree, lmin, lmax = CHEB
        dinv, spmv = jacobi_dinv(csr), se.spmv_of(A)
        lmin, lmax = math.ldexp(lmin, s), math.ldexp(lmax, s)
        return lambda r: gc.chebyshev_apply(spmv, r, dinv, degree, lmin, lmax)
    raise ValueError(pre)


def ilu0_multipliers(cpos, l, d):
    """l~_ik * (1 / d~_k) for the entries of the `before` part: cpos the
    position of an entry's column, d the pivots by position"""
    return np.asarray(l) * (1.0 / np.asarray(d))[np.asarray(cpos)]
