"""Cases and references for whole idrs solves on inputs that are not a benign
system: every exit on exact block matrices, the floor of scaling, non-finite
and overflowing data (b, A and dinv), and systems scaled by powers of two or
negated.  Nothing here touches a GPU: test_idrs_edges_host.py holds this module
to its claims on the reference alone, test_gpu_idrs_edges.py runs host.idrs on
it.  The companion of solver_edges.py and minres_edges.py.

The reference is idrs_cases.idrs_ref, imported, under np.errstate(all="ignore").
Its comparisons were read against cg.h and blas1_idrs.hip, in the kernels'
order:
  step (start)  hist[0] is written, then `rr == 0 or kmax == 0` (status 0; false
                on a NaN); the coefficients c_i = t / M[i][i] follow (M = I)
  biortho       a_i = t / M[i][i] for i < q (pivots that passed the test in
                their own step), the new column of M, then `M[q][q] == 0 or not
                finite` (status 1, nothing of the step is written); be = f_q /
                M[q][q] is guarded by it.  THIS is the first test a NaN or Inf
                in b, A or dinv meets that is true on it: such a solve ends at
                k = 0 with status 1, before any rtol test.  cg.h's "a non-finite
                scalar takes the go-on branch of the rtol test" and the
                existing test (a NaN in b: k = 0, status 1) are both right.
  step          k += 1, hist[k], then `hist[k] / hist[0] < rtol or k == kmax`
                (status 0; the quotient is false on a NaN), then the update of
                f and the next c_i (c_i = t / M[i][i] with M[i][i] of an EARLIER
                cycle or 1: not guarded again)
  omega         `not (tt > 0)` first (status 2; true on a NaN), then om = tr /
                tt, rho = tr / (sqrt(tt) * sqrt(rr)) (rr == 0 is not tested:
                rho is NaN or Inf there), the kappa rule, then `om == 0 or not
                finite` (status 2).  On two_i at s = 1 the FIRST branch is taken
                (t = 0: tt == 0); on skew the SECOND, with tt > 0 and t.r == 0:
                om = 0, rho = 0, and the kappa rule makes om = 0 * kappa / 0 a
                NaN, so it is "not finite", not "zero", that ends the solve.
                Dropping the first test changes nothing (0 / 0 is caught by the
                second); dropping `not finite` from the second does.
idrs_ref divides through idrs_cases._div (IEEE) and never raises;
idrs_cases.py is unchanged.

a. EXACT cases.  The shadow signs depend on the global row, so b is chosen from
   shadow_signs: `chosen(N, n, sign pattern)` marks the first n blocks whose
   rows have the given signs of p_0.  Every f_i and h_i is a sum of +-1 or +-2.
   TABLE, as measured, (name, s, kmax) -> (k, status, hist, (xa, xb)) with x =
   xa * b + xb * swap(b) (swap exchanges the two rows of a block):

     name    block            b                          N     s        k status
     q0      [[2,0],[0,2]]    1 on 512 + and 512 - rows  2048  1,2,4,8  0  1
             p_0 . b == 0: M[0][0] = p_0 . (A b) == 0 at q = 0, hist (32)
     two_i   [[2,0],[0,2]]    ones                       1024  2,4,8    1  1
             be = 1/2, r = 0, x = b / 2, hist (32, 0), then M[1][1] == 0 at
             q = 1; at s = 1 the om step: not (tt > 0), k = 1, status 2
     skew    [[0,2],[-2,0]]   (1,0) on 256 (+,+) blocks  4096  1        1  2
             M[0][0] = -512 < 0, be = -1/2, then om = NaN by the kappa rule;
             s >= 2: the second inner step solves (x = swap(b) / 2, k = 2),
             then s = 2 meets tt == 0 (status 2), s = 4, 8 M[2][2] == 0 (1)
     perm    [[0,1],[1,0]]    (1,0) on 128 (+,+) blocks  2048  1        2  1
             be = 1, then a full om step (om = -1, rho = -1) solves the system
             at k = 2; the next biortho finds M[0][0] == 0; s >= 2 as skew
     zero    [[2,0],[0,2]]    0                          1024  1,4      0  0
   kmax: two_i at kmax = 1 stops INSIDE a cycle (s >= 2) with status 0; perm at
   kmax = 1 stops after the inner step and at kmax = 2 AT the om step, status 0:
   the kmax stop wins over a breakdown that only the next step would find.
b. FLOOR: two_i (s = 2) and perm (s = 1) under scale_csr(s), and with dinv =
   0.5 * 2^-s.  With dinv every s repeats the row (x times 2^-s).  Without:
   two_i never forms a square and has no floor; perm's tt = t.t overflows at
   520 and 540 and underflows at -540: status 2 at k = 1 on a regular system
   (FLOOR); -520 is exact.
c. POISONED data on convdiff8 and cdpe10 at s = 1 and 4, without and with dinv,
   kmax 12, rtol 1e-10; dinv_nan and dinv_inf poison dinv alone: 48
   combinations.  POISON_OUTCOME: everything non-finite is k = 0, status 1, x =
   0; b_tiny k = 0, status 0; b_huge k = s, status 2, x finite -- the only
   WEAK kind (its s steps round): 8 of 48.
d. SCALED systems (2^s A, 2^t b, B^-1 scaled by 2^-s): x times 2^(t-s), the
   history times 2^t, at s = 1 and 4, PAIRS and the odd pair (101, 200), on
   convdiff8 (none, dinv, Chebyshev) and poisson8 (SGS, ILU(0), AMG rebuilt
   from the scaled matrix).  `pairs` drops (-400, -300) without a
   preconditioner: tt = 2^-1400 underflows.  (A, -b) gives -x for all; (-A, b)
   gives -x and the same history for none and dinv (dinv that of +A), bit for
   bit on the reference."""
import numpy as np

import gmres_cases as gc
import idrs_cases as ic
import minres_edges as me
import solver_edges as se
from idrs_cases import idrs_ref  # noqa: F401  (the reference, not a copy)
from minres_edges import pattern, rank1_nan  # noqa: F401
from solver_edges import (DOT, POISONS, SCALES, Result, _recording,  # noqa: F401
                          block_system, clean_rhs, dot_chunked, dot_reversed,
                          poisoned, same_bits, scale_csr)

ORDERS = (DOT, dot_reversed, dot_chunked)
KMAX = 40


def reference(csr, b, s, kmax, rtol, dinv=None, minv=None, dot=DOT, record=None,
              ref=None):
    """idrs_ref -> Result; dinv: the elementwise right preconditioner; minv:
    any other, a callable"""
    spmv = se.spmv_of(csr)
    if record is not None:
        spmv, dot = _recording(spmv, dot, record)
    if dinv is not None:
        minv = lambda q: dinv * q  # noqa: E731
    x, k, hist, status = (ref or ic.idrs_ref)(
        spmv, dot, minv, np.asarray(b, np.float64), s, kmax, rtol)
    return Result(x, k, hist, status)


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
def chosen(N, n, signs):
    """the first n two-row blocks of rows 0 .. N-1 whose signs of p_0 are
    `signs` -> their block indices"""
    P = ic.shadow_signs(0, N, 1)[0].reshape(-1, 2)
    hit = np.flatnonzero((P[:, 0] == signs[0]) & (P[:, 1] == signs[1]))
    assert len(hit) >= n, (N, n, len(hit))
    return hit[:n]


def swap(v):
    """exchange the two rows of every block (a tail row stays)"""
    n = len(v) - len(v) % 2
    out = np.array(v)
    out[:n] = np.asarray(v)[:n].reshape(-1, 2)[:, ::-1].reshape(-1)
    return out


I2, SKEW, PERM = ((2, 0), (0, 2)), ((0, 2), (-2, 0)), ((0, 1), (1, 0))


def _rhs(name, N):
    b = np.zeros(N)
    if name == "q0":
        P = ic.shadow_signs(0, N, 1)[0]
        for sign in (1.0, -1.0):
            b[np.flatnonzero(P == sign)[:512]] = 1.0
    elif name == "two_i":
        b[:] = 1.0
    elif name in ("skew", "perm"):
        b[2 * chosen(N, 256 if name == "skew" else 128, (1.0, 1.0))] = 1.0
    return b


SHAPES = {"q0": (I2, 1024), "two_i": (I2, 512), "skew": (SKEW, 2048),
          "perm": (PERM, 1024), "zero": (I2, 512)}
_SYS = {}


def system(name, tail):
    """-> (csr, b); tail: one more row, entry 1, b = 0"""
    if (name, tail) not in _SYS:
        block, nb = SHAPES[name]
        csr, _ = me.tailed_system(block, (0, 0), nb, tail)
        b = _rhs(name, 2 * nb)
        _SYS[name, tail] = (csr, np.append(b, 0.0) if tail else b)
    return _SYS[name, tail]


R2 = float(np.sqrt(2.0))


def _table():
    """(name, s, kmax) -> (k, status, hist, (xa, xb)): x = xa * b + xb * swap(b)"""
    h32, hs, hp = [32.0, 0.0], [16.0, 16.0 * R2], [8.0 * R2, 16.0]
    T = {("zero", 1, KMAX): (0, 0, [0.0], (0.0, 0.0)),
         ("zero", 4, KMAX): (0, 0, [0.0], (0.0, 0.0))}
    for s in (1, 2, 4, 8):
        T["q0", s, KMAX] = (0, 1, [32.0], (0.0, 0.0))
        T["q0", s, 0] = (0, 0, [32.0], (0.0, 0.0))
        # s = 1: the om step, not (tt > 0); s >= 2: M[1][1] == 0 at q = 1
        T["two_i", s, KMAX] = (1, 2 if s == 1 else 1, h32, (0.5, 0.0))
        T["two_i", s, 1] = (1, 0, h32, (0.5, 0.0))
        T["skew", s, 1] = (1, 0, hs, (-0.5, 0.0))
        T["perm", s, 1] = (1, 0, hp, (1.0, 0.0))
        T["perm", s, 2] = (2, 0, hp + [0.0], (0.0, 1.0))
    # s = 1: om not finite.  s >= 2: the second inner step solves the system
    # (x = swap(b) / 2), then s = 2 reaches the om step with t = 0 (status 2)
    # and s = 4, 8 the pivot M[2][2] == 0 (status 1)
    T["skew", 1, KMAX] = (1, 2, hs, (-0.5, 0.0))
    T["skew", 2, KMAX] = (2, 2, hs + [0.0], (0.0, 0.5))
    T["skew", 4, KMAX] = T["skew", 8, KMAX] = (2, 1, hs + [0.0], (0.0, 0.5))
    # s = 1: the om step solves, then M[0][0] == 0.  s >= 2: the second inner
    # step solves; s = 2 then meets tt == 0, s = 4, 8 a zero pivot
    T["perm", 1, KMAX] = (2, 1, hp + [0.0], (0.0, 1.0))
    T["perm", 2, KMAX] = (2, 2, hp + [0.0], (0.0, 1.0))
    T["perm", 4, KMAX] = T["perm", 8, KMAX] = (2, 1, hp + [0.0], (0.0, 1.0))
    return T


TABLE = _table()
SOLVED = {k for k, v in TABLE.items() if v[2][-1] == 0.0 and v[0] > 0}
TWO_RANKS = (("two_i", 2), ("perm", 1))


def want(key, tail):
    k, status, hist, (xa, xb) = TABLE[key]
    b = system(key[0], tail)[1]
    return Result(xa * b + xb * swap(b), k, hist, status)


# ---------------------------------------------------------------------------
# b. the floor of scaling
# ---------------------------------------------------------------------------
FLOOR_S = (520, -520, 540, -540)
FLOOR_CASES = (("two_i", 2), ("perm", 1))
EXACT_DINV = 0.5
# (name, s of idrs, scale) without a preconditioner -> (k, status, history, (xa,
# xb)); every key that is not listed, and EVERY case with dinv = 0.5 * 2^-scale,
# is the unscaled row with x times 2^-scale (both rows end with the exact
# solution, which a preconditioner does not move).  two_i forms no square
# of an entry of A (t = 0 or the pivot ends it first): no floor.  perm's om step
# forms tt = t.t = 2^(2 scale) 256: it overflows to Inf above (om = tr / Inf =
# 0, rho = 0, the kappa rule gives NaN: status 2 at k = 1 on a regular system,
# x = 2^-scale b the iterate of k = 1) and underflows to 0 at -540 (not (tt >
# 0): the same exit); 2^-1032 at -520 is subnormal but exact.
_HP = [8.0 * R2, 16.0]
FLOOR = {("perm", 1, 520): (1, 2, _HP, (2.0 ** -520, 0.0)),
         ("perm", 1, 540): (1, 2, _HP, (2.0 ** -540, 0.0)),
         ("perm", 1, -540): (1, 2, _HP, (2.0 ** 540, 0.0))}


def floor_case(name, s, scale, pre, tail):
    """-> (csr, b, dinv or None, want)"""
    csr, b = system(name, tail)
    k, status, hist, (xa, xb) = TABLE[name, s, KMAX]
    dinv = None
    if pre == "dinv":
        dinv = np.ldexp(np.full(len(b), EXACT_DINV), -scale)
    elif (name, s, scale) in FLOOR:
        k, status, hist, (xa, xb) = FLOOR[name, s, scale]
        return scale_csr(csr, scale), b, None, Result(xa * b + xb * swap(b), k,
                                                      hist, status)
    x = np.ldexp(xa * b + xb * swap(b), -scale)
    return scale_csr(csr, scale), b, dinv, Result(x, k, hist, status)


# ---------------------------------------------------------------------------
# c. poisoned data
# ---------------------------------------------------------------------------
POISON_SHAPES = ("convdiff8", "cdpe10")
POISON_S = (1, 4)
PRES = ("none", "dinv")
POISON_KMAX, POISON_RTOL = 12, 1e-10
DINV_POISONS = {"dinv_nan": np.nan, "dinv_inf": np.inf}
KINDS = POISONS + tuple(DINV_POISONS)
# kind -> (k (None: s, the om step of the first cycle), status, hist[0] class,
# x is +0.0 everywhere (else finite and not zero)).  Every non-finite input is
# caught by biortho's pivot test at q = 0; b = 1e200 has finite sign sums and
# pivots, rr = Inf and hist[k] / hist[0] = Inf / Inf goes on until the om step
# finds tt = Inf: om = tr / Inf = 0, status 2, x finite
POISON_OUTCOME = {
    "b_nan": (0, 1, "nan", True), "b_inf": (0, 1, "inf", True),
    "a_nan": (0, 1, "finite", True), "dinv_nan": (0, 1, "finite", True),
    "dinv_inf": (0, 1, "finite", True), "b_tiny": (0, 0, 0.0, True),
    "b_huge": (None, 2, "inf", False),
}


def csr_of(shape):
    return ic.cdpe(10, 5.0) if shape == "cdpe10" else ic.csr_by_name(shape)


def dinv_of(shape, s=0):
    return np.ldexp(1.0 / ic.diag_of(csr_of(shape)), -s)


def poison_combos():
    """(shape, kind, s, pre); WEAK below: b_huge, whose s steps round"""
    return [(shape, kind, s, pre) for shape in POISON_SHAPES for kind in KINDS
            for s in POISON_S for pre in PRES
            if pre == "dinv" or kind not in DINV_POISONS]


WEAK = {c for c in poison_combos() if c[1] == "b_huge"}  # 8 of 48


def poisoned_case(shape, kind, pre):
    """-> (csr, b, dinv or None); dinv is that of the CLEAN matrix"""
    csr = csr_of(shape)
    N = len(csr[0]) - 1
    dinv = dinv_of(shape) if pre == "dinv" else None
    if kind in DINV_POISONS:
        dinv = dinv.copy()
        dinv[N // 3] = DINV_POISONS[kind]
        return csr, clean_rhs(N), dinv
    pc, b = poisoned(csr, kind)
    return pc, b, dinv


def poisoned_reference(shape, kind, s, pre, dot=DOT, ref=None):
    csr, b, dinv = poisoned_case(shape, kind, pre)
    return reference(csr, b, s, POISON_KMAX, POISON_RTOL, dinv=dinv, dot=dot,
                     ref=ref)


# ---------------------------------------------------------------------------
# d. scaled and negated systems
# ---------------------------------------------------------------------------
PAIRS = SCALES + ((300, 0), (-400, -300))
SCALED_KMAX, SCALED_RTOL = 60, se.SCALED_RTOL
SCALED_S = (1, 4)
ODD_PAIR = (101, 200)  # s + t odd: tt scales by an even power all the same
# shape -> preconditioners; SGS, ILU(0) and AMG are rebuilt from the scaled
# matrix (an SPD shape), Chebyshev keeps its bounds in (dinv 2^-s)(2^s A)
SCALED = {"convdiff8": ("none", "dinv", "cheb"),
          "poisson8": ("sgs", "ilu0", "amg")}
NEGATED_A = ("none", "dinv")  # dinv stays that of +A


def pairs(pre):
    """without a preconditioner (-400, -300) is dropped: tt = t.t carries
    2^(2 (s + t)) = 2^-1400 and underflows on the reference itself; with any
    B^-1 that scales by 2^-s, t = A B^-1 r carries 2^t alone"""
    return PAIRS[:-1] if pre == "none" else PAIRS


def scaled_rhs(shape):
    return ic.case(shape)[1]


def minv_of(pre, shape, s=0):
    """the reference's B^-1 for 2^s * csr_of(shape)"""
    import amg_cases
    import ilu0_cases
    A = scale_csr(csr_of(shape), s)
    N = len(A[0]) - 1
    if pre == "none":
        return None
    dinv = dinv_of(shape, s)
    if pre == "dinv":
        return lambda q: dinv * q
    if pre == "cheb":
        spmv = se.spmv_of(A)
        return lambda q: gc.chebyshev_apply(spmv, q, dinv, *ic.CHEB)
    if pre == "sgs":
        return gc.SgsRef(A)
    if pre == "ilu0":
        ref = ilu0_cases.Ilu0Ref(A, N, gc.sgs_color(A), False)
        fac = ref.factor()
        return lambda q: ref.apply(fac, q)
    if pre == "amg":
        return amg_cases.AmgRef(A, N).apply
    raise KeyError(pre)
