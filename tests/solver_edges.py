"""Cases and references for whole solves on inputs that are not a benign SPD
system: breakdowns, zero curvature, non-finite data and systems scaled by powers
of two.  Nothing here touches a GPU: test_solver_edges_host.py holds this module
to its claims on the references alone, test_gpu_solver_edges.py runs the
solvers on it.

The references are the restatements of cg.h the solver tests already use,
imported, not copied: oracle.cg (cg, and cg_block column by column with the
zero-column rule), test_gpu_pcg._pcg_ref, test_gpu_chebyshev._pcg_ref with
_apply_ref, the same with test_gpu_sgs.Sweeps, test_gpu_bicgstab._bicgstab_ref.
Their comparisons were read against cg.h and the device code: every stop test
is `a / b < rtol` (false on NaN: a NaN never stops a solve), every breakdown
and zero test `== 0`; none had to be rewritten.  What they needed is a dot
product that returns np.float64, so that a division by an exact zero gives the
Inf or NaN of IEEE and not Python's ZeroDivisionError (DOT below), and
np.errstate(all="ignore"), which `reference` sets.

a. EXACT cases: block-diagonal matrices of one small integer block repeated NB
   times (plus, where that leaves N even, one tail row with the entry 1 and
   b = 0), N odd between 1 000 and 5 000, integer right-hand sides.  Every
   alpha, omega and beta up to the event is dyadic and every element a small
   dyadic number, so every product and sum is exact in any summation order and
   the device must reproduce the reference's bits.  The blocks were found by
   `search_blocks`, a brute-force search in Fraction arithmetic over the
   nonsingular 2x2 blocks with entries in (0, 1, -1, 2, -2) and the nonsingular
   3x3 blocks with entries in (0, 1, -1), in that order, first hit:

     BiCGStab  tt == 0 at k = 1             TT0   [[0,1],[1,0]]  b (1,1); and the
                                                  issue's own A = 2I, b (1,1)
               ts == 0, tt != 0 at k = 1    TS0   [[0,1],[1,1]]  b (0,1)
               rho[1] == 0, omega != 0      RHO0  [[0,0,1],[0,1,0],[1,1,1]]  b (0,1,0)
               ts == 0 at k = 2             TS0_2 [[0,0,1],[0,1,1],[1,0,1]]  b (0,1,-1)
               rv == 0 in iteration 2       BD1_2 the same block, b (1,1,-1)
     CG family p.Ap == 0 at k = 1           CURV1 [[0,1],[1,0]]  b (0,1)
               p.Ap == 0 at k = 2           CURV2 [[0,0,1],[0,1,1],[1,1,0]]  b (1,-1,0)

   cg() and cg_block form alpha from sqrt(rr)^2, so for them rr[j] must be a
   square as well: the search for CURV2 demands rr[j] / rr[0] a rational square,
   and NB is chosen so that NB * rr[0] is a square (CURV1: NB = 25^2, rr[0] =
   625; CURV2: NB = 2 * 15^2, rr[0] = 900).  pcg_sgs takes no part in the
   zero-curvature cases: the blocks need a zero on the diagonal, which its
   constructor refuses (a non-positive diagonal is outside the interface).
   Minus the Poisson matrix is negative definite; CG on (-A, b) is CG on (A, b)
   with alpha and x negated, exactly, so it is a case of c. below.

b. POISONED data on the shapes of test_gpu_pcg.py (the plain matrices): see
   `poisoned`.  The clean right-hand side is made of small integers so that
   rr[0], where it is finite, has the same bits in any order.

c. SCALED systems (2^s A, 2^t b), dinv scaled by 2^-s where a solver takes one
   (Chebyshev also: dinv left alone and lmin, lmax scaled by 2^s), and negated
   ones.  The exponent pairs used are SCALES; the pairs the issue starts from,
   s = +-100 and t = +-200, hold on every reference without shrinking.  The
   host test shows the relation bit for bit and, through `reference(...,
   record=)`, that every operand and result of every SpMV and dot product of
   both runs is finite, nonzero where its partner is, and far from the
   subnormal range.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

import oracle
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from special_values import same_bits, subnormal  # noqa: F401 (re-exported)
from spmv_amd import host
from test_gpu_bicgstab import _bicgstab_ref, _dot_chunked
from test_gpu_sgs import Sweeps

SOLVERS = ("cg", "cg_block", "pcg", "pcg_chebyshev", "pcg_sgs", "bicgstab")
KMAX = 40  # of every poisoned and breakdown solve


def DOT(a, b):
    """oracle.ddot as an np.float64: x / 0 is Inf or NaN, not an exception"""
    return np.float64(oracle.ddot(a, b))


def dot_chunked(a, b):
    with np.errstate(all="ignore"):
        return np.float64(_dot_chunked(a, b))


def dot_reversed(a, b):
    return np.float64(oracle.ddot(np.asarray(a)[::-1], np.asarray(b)[::-1]))


class Result:
    def __init__(self, x, k, hist, status=0):
        self.x, self.k, self.status = np.asarray(x), int(k), int(status)
        self.hist = np.asarray(hist, dtype=np.float64)

    def same(self, other):
        return (self.k == other.k and self.status == other.status
                and same_bits(self.hist, other.hist)
                and same_bits(self.x, other.x))


def spmv_of(csr):
    return lambda v: oracle.csr_spmv(*csr, v)


def colours_of(csr):
    return host.sgs_color(csr[0], csr[1], len(csr[0]) - 1)[0]


def _recording(spmv, dot, record):
    """spmv and dot that append what goes in and what comes out to `record`:
    every vector a restatement multiplies or reduces (r, p, z, A p, v, s, t, ...)
    and every reduced scalar (rr, rz, p.Ap, rho, rv, ts, tt)"""
    def spmv2(v):
        y = spmv(v)
        record.append(np.array(v))
        record.append(np.array(y))
        return y

    def dot2(a, b):
        d = dot(a, b)
        record.append(np.array(a))
        record.append(np.array(b))
        record.append(np.array([d]))
        return d
    return spmv2, dot2


def reference(solver, csr, b, kmax, rtol, dinv=None, cheb=None, dot=DOT,
              ref=None, record=None):
    """-> Result.  dinv: pcg (required), pcg_chebyshev and bicgstab (or None);
    cheb = (degree, lmin, lmax); ref: another restatement in place of the
    solver's own (the mutants of the host test); record: a list that receives
    every operand and result of the restatement's SpMVs and dot products (not
    for "cg", whose reference is compiled C).  cg_block: see
    `reference_block`."""
    spmv = spmv_of(csr)
    if record is not None:
        assert solver != "cg" or ref is not None
        spmv, dot = _recording(spmv, dot, record)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        if solver == "cg":
            if ref is not None:
                return Result(*ref(spmv, dot, b, kmax, rtol))
            return Result(*oracle.cg(*csr, b, kmax, rtol))
        if solver == "pcg":
            return Result(*(ref or tp._pcg_ref)(spmv, dot, b, dinv, kmax, rtol))
        if solver == "pcg_chebyshev":
            degree, lmin, lmax = cheb

            def M(r):
                return tc._apply_ref(spmv, r, dinv, degree, lmin, lmax)
            return Result(*(ref or tc._pcg_ref)(spmv, dot, b, M, kmax, rtol))
        if solver == "pcg_sgs":
            sweeps = Sweeps(csr, len(b), colours_of(csr), False)
            d = 1.0 / tp._diag_of(csr)
            return Result(*(ref or tc._pcg_ref)(
                spmv, dot, b, lambda r: sweeps.apply(d, r), kmax, rtol))
        if solver == "bicgstab":
            return Result(*(ref or _bicgstab_ref)(spmv, dot, b, dinv, kmax, rtol))
    raise ValueError(solver)


def reference_block(csr, B, kmax, rtol):
    """cg_block: oracle.cg column by column; a column with r0.r0 == 0 stops at
    k = 0 with x = 0 (cg.h).  -> (iterations, history[nrhs, kmax + 1] with -1.0
    beyond a column's k, X)"""
    B = np.asarray(B, dtype=np.float64)
    n, nrhs = B.shape
    its = np.zeros(nrhs, np.int32)
    hist = np.full((nrhs, kmax + 1), -1.0)
    X = np.zeros((n, nrhs))
    for c in range(nrhs):
        b = np.ascontiguousarray(B[:, c])
        if DOT(b, b) == 0.0:
            hist[c, 0] = 0.0
            continue
        r = reference("cg", csr, b, kmax, rtol)
        its[c], X[:, c] = r.k, r.x
        hist[c, :r.k + 1] = r.hist
    return its, hist, X


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
def _dyadic(q):
    return q.denominator & (q.denominator - 1) == 0


def _is_square(q):
    a, b = q.numerator, q.denominator
    return a >= 0 and math.isqrt(a) ** 2 == a and math.isqrt(b) ** 2 == b


def _mv(A, v):
    return [sum(a * x for a, x in zip(row, v)) for row in A]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _det(A):
    if len(A) == 2:
        return A[0][0] * A[1][1] - A[0][1] * A[1][0]
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1])
            - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
            + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))


def simulate_bicgstab(A, b, kmax=4):
    """BiCGStab of cg.h on one block in Fraction arithmetic -> (k, event) with
    the event of iteration k, or None when a scalar on the way is not dyadic:
    "bd1" rv == 0; "tt0" tt == 0; "ts0" ts == 0 != tt; "conv" r == 0;
    "rho0" rho[k] == 0 with omega != 0 and r != 0."""
    r = [Fraction(v) for v in b]
    rhat, p = r[:], r[:]
    rho = _dot(r, r)
    if rho == 0:
        return None
    for k in range(1, kmax + 1):
        v = _mv(A, p)
        rv = _dot(rhat, v)
        if rv == 0:
            return (k, "bd1")
        alpha = rho / rv
        if not _dyadic(alpha):
            return None
        s = [x - alpha * y for x, y in zip(r, v)]
        t = _mv(A, s)
        ts, tt = _dot(t, s), _dot(t, t)
        omega = Fraction(0) if tt == 0 else ts / tt
        if not _dyadic(omega):
            return None
        r = [x - omega * y for x, y in zip(s, t)]
        rr, rho_new = _dot(r, r), _dot(rhat, r)
        if tt == 0:
            return (k, "tt0")
        if ts == 0:
            return (k, "ts0")
        if rr == 0:
            return (k, "conv")
        if rho_new == 0:
            return (k, "rho0")
        beta = (rho_new / rho) * (alpha / omega)
        if not _dyadic(beta):
            return None
        p = [x + beta * (y - omega * z) for x, y, z in zip(r, p, v)]
        rho = rho_new
    return None


def simulate_cg(A, b, kmax=4):
    """CG on one symmetric block in Fraction arithmetic -> (k, "curv") when
    p.Ap == 0 in iteration k, (k, "conv") when r == 0; None when A is not
    symmetric, an alpha or beta on the way is not dyadic, or an rr[j] / rr[0]
    is not a rational square (cg() forms alpha and beta from sqrt(rr)^2)."""
    n = len(b)
    if any(A[i][j] != A[j][i] for i in range(n) for j in range(i)):
        return None
    r = [Fraction(v) for v in b]
    p = r[:]
    rr = rr0 = _dot(r, r)
    if rr == 0:
        return None
    for k in range(1, kmax + 1):
        Ap = _mv(A, p)
        pAp = _dot(p, Ap)
        if pAp == 0:
            return (k, "curv")
        alpha = rr / pAp
        if not _dyadic(alpha):
            return None
        r = [x - alpha * y for x, y in zip(r, Ap)]
        rr_new = _dot(r, r)
        if rr_new == 0:
            return (k, "conv")
        beta = rr_new / rr
        if not (_dyadic(beta) and _is_square(rr_new / rr0)):
            return None
        p = [beta * x + y for x, y in zip(p, r)]
        rr = rr_new
    return None


ORDER5, ORDER3 = (0, 1, -1, 2, -2), (0, 1, -1)


def search_blocks(n, simulate, want):
    """The first nonsingular n x n block and right-hand side, in the order of
    itertools.product over ORDER5 (n = 2) or ORDER3 (n = 3), for every event in
    `want` -> {event: (A, b)}; stops when all are found."""
    vals = ORDER5 if n == 2 else ORDER3
    found = {}
    for ent in itertools.product(vals, repeat=n * n):
        A = tuple(ent[i * n:(i + 1) * n] for i in range(n))
        if _det(A) == 0:
            continue
        for b in itertools.product(vals, repeat=n):
            ev = simulate(A, b)
            if ev in want and ev not in found:
                found[ev] = (A, b)
                if len(found) == len(want):
                    return found
    return found


class Exact:
    """One exact case: the block, its right-hand side, the number of blocks,
    the solvers it is for and what the reference must do on it."""

    def __init__(self, name, block, rhs, nb, solvers, event, k, status=0,
                 rtol=0.0, at=None):
        self.at = k if at is None else at  # the iteration of the event
        self.name, self.block, self.rhs, self.nb = name, block, rhs, nb
        self.solvers, self.event, self.k = solvers, event, k
        self.status, self.rtol = status, rtol
        self.csr, self.b = block_system(block, rhs, nb)
        self.N = len(self.b)


def exact_block(case, nrhs):
    """cg_block on an exact case: the case's right-hand side in every column
    but column 1, which is zero"""
    return np.stack([np.zeros(case.N) if c == 1 else case.b
                     for c in range(nrhs)], axis=1)


def block_system(block, rhs, nb):
    """-> (csr, b): `nb` copies of the block on the diagonal (zero entries are
    not stored), and one tail row (entry 1, b = 0) where that makes N odd"""
    n = len(block)
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in range(n):
            if block[i][j] != 0:
                rows.append(i), cols.append(j), vals.append(float(block[i][j]))
    base = n * np.arange(nb)[:, None]
    rows = (base + np.array(rows)[None, :]).reshape(-1)
    cols = (base + np.array(cols)[None, :]).reshape(-1)
    vals = np.tile(np.array(vals), nb)
    b = np.tile(np.array(rhs, dtype=np.float64), nb)
    N = n * nb
    if N % 2 == 0:
        rows, cols = np.append(rows, N), np.append(cols, N)
        vals, b = np.append(vals, 1.0), np.append(b, 0.0)
        N += 1
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
    return ((rp.astype(np.int32), cols[order].astype(np.int32), vals[order]), b)


TT0 = (((0, 1), (1, 0)), (1, 1))
TWO_I = (((2, 0), (0, 2)), (1, 1))
TS0 = (((0, 1), (1, 1)), (0, 1))
RHO0 = (((0, 0, 1), (0, 1, 0), (1, 1, 1)), (0, 1, 0))
TS0_2 = (((0, 0, 1), (0, 1, 1), (1, 0, 1)), (0, 1, -1))
BD1_2 = (((0, 0, 1), (0, 1, 1), (1, 0, 1)), (1, 1, -1))
CURV1 = (((0, 1), (1, 0)), (0, 1))
CURV2 = (((0, 0, 1), (0, 1, 1), (1, 1, 0)), (1, -1, 0))

CG_FAMILY = ("cg", "cg_block", "pcg", "pcg_chebyshev")
BI = ("bicgstab",)
# Chebyshev on the exact cases: degree 1 on [0.5, 1.5] without a dinv, theta =
# 1 and b_0 = 1 exactly, so z = r and every scalar is the one of pcg
CHEB_EXACT = (1, 0.5, 1.5)
# Chebyshev on the other cases: the bounds of test_gpu_chebyshev.py, degree 3
CHEB = (3, tc.LMIN, tc.LMAX)


def exact_cases():
    E = Exact
    return [
        # name, block, b, NB, solvers, event, k of the stop, status, rtol
        E("2I", *TWO_I, 625, BI, "tt0", 1, 2),
        E("2I_rtol", *TWO_I, 625, BI, "tt0", 1, 0, rtol=1e-10),
        E("tt0", *TT0, 625, BI, "tt0", 1, 2),
        E("ts0", *TS0, 625, BI, "ts0", 1, 2),
        E("rho0", *RHO0, 445, BI, "rho0", 1, 2),
        E("ts0_k2", *TS0_2, 445, BI, "ts0", 2, 2),
        E("bd1_k2", *BD1_2, 445, BI, "bd1", 1, 1, at=2),
        E("curv_k1", *CURV1, 625, CG_FAMILY, "curv", KMAX, at=1),
        E("curv_k2", *CURV2, 450, CG_FAMILY, "curv", KMAX, at=2),
    ]


# ---------------------------------------------------------------------------
# b. poisoned data
# ---------------------------------------------------------------------------
def clean_rhs(N):
    """integers in [-3, 3] \\ {0}: b.b is exact in any order"""
    rng = np.random.default_rng(N + 5)
    return (rng.integers(1, 4, N) * rng.choice([-1, 1], N)).astype(np.float64)


POISONS = ("b_nan", "b_inf", "b_huge", "b_tiny", "a_nan")


def poisoned(csr, kind):
    """-> (csr, b) of one poisoned case on a matrix of test_gpu_pcg.py"""
    rp, ci, va = csr
    N = len(rp) - 1
    b = clean_rhs(N)
    if kind == "b_nan":
        b[N // 3] = np.nan
    elif kind == "b_inf":
        b[2 * N // 3] = np.inf
    elif kind == "b_huge":
        b = np.full(N, 1e200)   # r0.r0 overflows
    elif kind == "b_tiny":
        b = np.full(N, 1e-200)  # r0.r0 underflows to exactly 0, b != 0
    elif kind == "a_nan":
        rows = tp._row_of(rp)
        off = np.flatnonzero(ci != rows)
        va = va.copy()
        va[off[len(off) // 2]] = np.nan
    else:
        raise ValueError(kind)
    return (rp, ci, va), b


def solver_kwargs(solver, csr, exact=False, s=0, cheb_bounds=False):
    """dinv and cheb of `reference` for a solver on a matrix: the Jacobi dinv
    (exact cases: ones) times 2^-s; cheb_bounds: Chebyshev leaves dinv alone and
    scales lmin and lmax by 2^s"""
    N = len(csr[0]) - 1
    kw = {}
    if solver in ("pcg", "pcg_chebyshev", "bicgstab"):
        d = np.ones(N) if exact else 1.0 / tp._diag_of(csr)
        kw["dinv"] = d if cheb_bounds else np.ldexp(d, -s)
    if solver == "pcg_chebyshev":
        degree, lmin, lmax = CHEB_EXACT if exact else CHEB
        if exact:
            kw["dinv"] = None
        if cheb_bounds:
            lmin, lmax = math.ldexp(lmin, s), math.ldexp(lmax, s)
        kw["cheb"] = (degree, lmin, lmax)
    return kw


# ---------------------------------------------------------------------------
# c. scaled systems
# ---------------------------------------------------------------------------
# (s, t): A' = 2^s A, b' = 2^t b.  The issue's starting pairs; none had to shrink.
SCALES = ((100, 200), (-100, -200), (100, -200), (-100, 200))
# (-A, b): x' = -x.  Not pcg_sgs, whose constructor refuses a negative diagonal,
# and not pcg_chebyshev, whose polynomial on [lmin, lmax] does not commute with
# the sign of A (the spectrum of dinv * (-A) is not in the interval)
NEGATED_A = ("cg", "cg_block", "pcg", "bicgstab")
# the pairs that reach below 1e-290 (rr[0] = 2^-980 b.b): (s, t, kmax), at rtol =
# 0 on the integer right-hand side.  s has the sign that keeps p.Ap = 2^(2t + s)
# (cg) and rz = 2^(2t - s) (pcg) above 2^-1022.
FLOOR = {"cg": (100, -490, 2), "pcg": (-100, -490, 2)}
SCALED_SHAPES = ("poisson11", "banded4097")
SCALED_KMAX, SCALED_RTOL = 60, 1e-8


def scaled_rhs(csr):
    N = len(csr[0]) - 1
    return oracle.csr_spmv(*csr, np.random.default_rng(N + 1).uniform(-1, 1, N))


def scale_csr(csr, s, sign=1.0):
    return csr[0], csr[1], sign * np.ldexp(csr[2], s)
