"""Cases and expected outcomes for whole lobpcg solves on inputs that are not a
benign system: restarts that recover and restarts that collapse, blocks that
fill the space, exact arithmetic, poisoned data and systems scaled by powers of
two or negated.  Nothing here touches a GPU: test_lobpcg_edges_host.py holds
this module to its claims on the restatement alone, test_gpu_lobpcg_edges.py
runs host.lobpcg on it.  The companion of solver_edges.py, gmres_edges.py and
minres_edges.py.

The reference is lobpcg_cases.lobpcg_ref, imported unchanged.  Its comparisons
and divisors were read against blas1_lobpcg.hip and cg.h along the paths these
cases walk for the first time:
  - 1 / sqrt(Gb_jj) (the scaling): numpy scalars under errstate, so 1/sqrt(0) =
    Inf, 1/sqrt(Inf) = 0 and sqrt of a negative number = NaN as on the device;
    the products with them give NaN, and the pivot test `not piv > 0` refuses a
    NaN as `!(piv > 0.0)` does.  math.sqrt(piv) only ever sees piv > 0 (+Inf
    included, which it returns).
  - the Jacobi rotation: every operand is a numpy scalar, (aqq - app) / (2 apq)
    never raises; a NaN entry is neither == 0 nor "small", so it rotates for
    all 30 sweeps in both; the selection refuses a theta with theta - theta != 0.
  - norms_ref: `rn2 >= 0` comes before math.sqrt, which therefore never raises
    (NaN and negative sums give NaN as sqrt() does on the device; -0.0 and Inf
    pass through); `a > atol` and `r < tol` are false on a NaN in both.
  - the retry: `attempt == 1 and not (nb == 3 and has_p)` is the kernel's
    `break`; a restart leaves has_p = 1 in both (P' is then made from W alone).
  - reduce_column, rows_partials, gram_partials and the epilogue's true_res
    run under lobpcg_ref's errstate guards: an Inf gives Inf or NaN, never an
    exception (test_lobpcg_edges_host.py feeds them Inf, NaN and overflow).
  - status 1 leaves X, theta and the history as they were before the failed
    step in both; the history of a prologue that failed stays -1.0, theta 0.
Nothing disagreed: lobpcg_cases.py and the kernels are unchanged.

The table (TABLE; every (k, status, restarts) computed here, on the CPU):
a. restarts -- classes "recovered" (restarted, every column converged), "kmax"
   (restarted, status 0 at kmax), "collapsed" (restarted, status 1 later) and
   "no_p" (status 1 at k >= 1 and no restart counted: there was no P to drop,
   or the retry without P failed as well), each on two matrices or more; nev = 8 with all 24 columns
   (a_tri24_8, a_tri33_8); restarts on a compacted index list (a_diag15_l on
   0b111010, a_tri33_conv and a_tri24_l on 0b11011011, a_diag12 on 0b110).
   a_diag8 ends with status 0 at kmax and theta_0 = -2.5e59 (`wild`).
b. blocks that fill the space: N = nev (k = 0, status 0), N = 2, and nev <= N <
   3 nev, where S has more columns than rows from iteration 2 (or 1) on:
   diag(1..5), diag(1..6), tri(6), diag(1..23), diag(1..24) converge in 2 to 4
   iterations, tri(5) and tri(23) end with status 1 at k = 1; A = [0].
c. exact arithmetic: residuals exactly 0, theta = 0 with atol = 0 (status 1 at
   k = 0: `0 < 0` is false, W = 0, 1 / sqrt(0)) and with atol = 1e-300 (status
   0), a tie between Ritz values, a pivot that is exactly 0.
d. poisons, all held to bits (on one rank the device's summation order is the
   restatement's, and no result depends on a NaN's payload: same() takes NaN
   as a class): dinv[17] NaN, +Inf, -Inf (k = 0, status 1, X the prologue's
   rotated block), 0 (harmless); A.values[5] Inf, -Inf (X the orthonormalised
   X0), 1e308, 1e200 (finite theta, true_resnorm Inf); X0 with an Inf, with a
   NaN in row 70 (past the first Gram chunk) and in the last row (X = X0).
e. the bases of the relations; EDGES holds the working range found by
   bisect_edge, INSIDE points well within, NEGATED the (-A, smallest) pairs.
"""
import contextlib

import numpy as np

import gmres_cases as gc
import lobpcg_cases as lc
from lobpcg_cases import lobpcg_ref  # noqa: F401  (the reference, not a copy)

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------
# matrices and initial blocks
# ---------------------------------------------------------------------------
def diag(d):
    """the diagonal matrix of `d` (zeros are stored)"""
    d = np.array(d, np.float64)
    n = len(d)
    return (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)


def tri(N):
    """tridiagonal 2 / -1: eigenvalues 2 - 2 cos(j pi / (N + 1))"""
    i = np.arange(N)
    rows, cols, vals = [i], [i], [np.full(N, 2.0)]
    if N > 1:
        rows += [i[:-1], i[1:]]
        cols += [i[1:], i[:-1]]
        vals += [np.full(N - 1, -1.0)] * 2
    return gc.to_csr(N, rows, cols, vals)


def csr_by_name(name):
    """poisson11, shift11; diagA_B: diag(A, A + 1, ..., B); triN; ties9:
    diag(1, 1, 2, 3, ..., 8)"""
    if name.startswith("diag"):
        lo, hi = name[4:].split("_")
        return diag(np.arange(float(lo), float(hi) + 1.0))
    if name.startswith("tri"):
        return tri(int(name[3:]))
    if name == "ties9":
        return diag([1.0, 1.0] + list(range(2, 9)))
    return lc.csr_by_name(name)


class Mat(lc.Case):
    """lobpcg_cases.Case for the matrices of this file, and for a csr given
    outright (a poisoned or scaled copy)"""

    def __init__(self, name, csr=None):
        self.name = name
        self.csr = csr_by_name(name) if csr is None else csr
        self.N = len(self.csr[0]) - 1
        self.diag = gc.diag_of(self.csr)
        with np.errstate(all="ignore"):
            self.norm_a = float(np.abs(lc.dense(self.csr)).sum(axis=1).max())
        self._eig = None
        self._refs = {}


_MATS = {}


def mat(name):
    if name not in _MATS:
        _MATS[name] = Mat(name)
    return _MATS[name]


def vary_dinv(N):
    """a positive diagonal that is no multiple of the identity"""
    return 1.0 / (1.0 + 0.5 * ((np.arange(N) * 7) % 5))


def units(cols, extra=()):
    """X0 = the unit vectors e_c, c in cols, then X0[i, j] = v for (i, j, v) in
    extra"""
    def make(N, nev):
        X = np.zeros((N, nev))
        for j, c in enumerate(cols):
            X[c, j] = 1.0
        for i, j, v in extra:
            X[i, j] = v
        return X
    return make


def seed(s, extra=()):
    """X0 = lobpcg_cases.x0(N, nev, s), then X0[i, j] = v for (i, j, v) in extra
    (i < 0 counts from the last row)"""
    def make(N, nev):
        X = lc.x0(N, nev, s)
        for i, j, v in extra:
            X[i, j] = v
        return X
    return make


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
class Entry:
    """One whole solve.  want: (k, status, restarts) of the restatement, or
    None where a relation test holds the case.  poison: None, ("dinv", i, v)
    or ("a", i, v) (entry i of dinv or of A.values becomes v; a poisoned X0 is
    in x0).  bits: the device is held to the restatement's bits (else to (k,
    status), to `finite` and to the guard words).  finite: X comes back finite.
    cls: the class of group a.  order: "stable" -- (k, status, restarts) are the
    same under every summation order of ORDERS -- or "one" -- held to the
    device's order only (test_lobpcg_edges_host.py asserts the record).  wild:
    status 0 with a Ritz value outside [-2 ||A||, 2 ||A||] (`is_wild`)."""

    def __init__(self, id, group, matrix, nev, x0, kmax, rtol, want, atol=0.0,
                 largest=False, kind="none", poison=None, bits=True,
                 finite=True, cls=None, order="stable", wild=False):
        self.id, self.group, self.matrix, self.nev = id, group, matrix, nev
        self.x0, self.kmax, self.rtol, self.atol = x0, kmax, rtol, atol
        self.largest, self.kind, self.want = largest, kind, want
        self.poison, self.bits, self.finite = poison, bits, finite
        self.cls, self.order, self.wild = cls, order, wild

    def __repr__(self):
        return self.id

    def mat(self):
        M = mat(self.matrix)
        if self.poison and self.poison[0] == "a":
            rp, ci, va = M.csr
            va = va.copy()
            va[self.poison[1]] = self.poison[2]
            return Mat(self.id, (rp, ci, va))
        return M

    def X0(self):
        return self.x0(mat(self.matrix).N, self.nev)

    def dinv(self):
        """None, or the array of kind "dinv": 1 / |diag| of the clean matrix
        with the poisoned entry"""
        if self.kind != "dinv":
            return None
        d = mat(self.matrix).dinv()
        if self.poison and self.poison[0] == "dinv":
            d[self.poison[1]] = self.poison[2]
        return d


def reference(e, kmax=None, precond=None, dinv=None, M=None, X0=None, **kw):
    """lobpcg_ref on entry e (kmax, dinv, the matrix or X0 replaced on demand;
    cap and dot_blocks pass through)"""
    M = M or e.mat()
    return lc.lobpcg_ref(M.spmv, precond, e.X0() if X0 is None else X0,
                         e.kmax if kmax is None else kmax, e.rtol, e.atol,
                         e.largest, e.dinv() if dinv is None else dinv, **kw)


def is_wild(e, r):
    """status 0, yet some |theta_c| > 2 ||A||_inf: no Ritz value of an
    orthonormal block leaves the hull of the spectrum, so X is not one"""
    with np.errstate(all="ignore"):
        return bool(r["status"] == 0 and np.abs(r["theta"]).max()
                    > 2.0 * mat(e.matrix).norm_a)


def decisions(r):
    return (r["k"], r["status"], r["restarts"])


# ---------------------------------------------------------------------------
# probes: what the restatement has to tell beyond its result
# ---------------------------------------------------------------------------
_TINY = np.finfo(np.float64).tiny


class Probe:
    """While active, records of every Gram sum, every column norm, every block
    that combine and residual_ref return: whether all of it was finite, and
    whether a nonzero value was subnormal (`normal`); and of every Rayleigh-Ritz
    step that restarted, the active mask it ran on (`restart_masks`).  The
    restatement itself is not changed: its module-level names are wrapped for
    the duration."""
    NAMES = ("gram_sum", "reduce_column", "combine", "residual_ref")

    def __init__(self):
        self.finite = self.normal = True
        self.restart_masks = []

    def _see(self, out):
        for a in (out if isinstance(out, tuple) else (out,)):
            a = np.asarray(a, np.float64)
            self.finite &= bool(np.all(np.isfinite(a)))
            nz = np.abs(a[(a != 0.0) & np.isfinite(a)])
            self.normal &= bool(nz.size == 0 or nz.min() >= _TINY)

    def _wrap(self, fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            self._see(out)
            return out
        return wrapped

    def __enter__(self):
        self._saved = {n: getattr(lc, n) for n in self.NAMES + ("rr_ref",)}
        for n in self.NAMES:
            setattr(lc, n, self._wrap(self._saved[n]))
        rr = self._saved["rr_ref"]

        def rr_ref(gram, k, nb, active, *a, **kw):
            out = rr(gram, k, nb, active, *a, **kw)
            if out["ok"] and out["restart"]:
                self.restart_masks.append(active)
            return out
        lc.rr_ref = rr_ref
        return self

    def __exit__(self, *exc):
        for n, fn in self._saved.items():
            setattr(lc, n, fn)


@contextlib.contextmanager
def two_slabs():
    """Another summation order: the rows cut in two halves as two ranks own
    them, each half summed the kernels' way, the halves added in rank order
    (what the all-reduce of the Gram sums and of the norms does)."""
    gp, rp = lc.gram_partials, lc.rows_partials

    def gram_partials(S, AS, grid):
        h = (S.shape[0] + 1) // 2
        parts = [lc.gram_sum(gp(S[a:b], AS[a:b], lc.gram_grid(max(b - a, 1))))
                 for a, b in ((0, h), (h, S.shape[0]))]
        return np.stack(parts)

    def rows_partials(vals, grid):
        h = (vals.shape[0] + 1) // 2
        parts = [lc.reduce_column(rp(vals[a:b], lc.rows_grid(max(b - a, 1))))
                 for a, b in ((0, h), (h, vals.shape[0]))]
        return np.stack(parts)
    lc.gram_partials, lc.rows_partials = gram_partials, rows_partials
    try:
        yield
    finally:
        lc.gram_partials, lc.rows_partials = gp, rp


# name -> a context manager factory and the keywords of lobpcg_ref
ORDERS = {"cap1": (contextlib.nullcontext, dict(cap=1)),
          "cap3": (contextlib.nullcontext, dict(cap=3)),
          "dot1": (contextlib.nullcontext, dict(dot_blocks=1)),
          "slabs": (two_slabs, {})}


def other_orders(e):
    """-> {order name: (k, status, restarts)}; cap is left out where there is
    one Gram chunk (N <= 64) and dot_blocks where there is one block of rows
    (N <= 256): they are the restatement's own order there"""
    out = {}
    N = mat(e.matrix).N
    for name, (ctx, kw) in ORDERS.items():
        if (N <= lc.GRAM_ROWS and "cap" in kw) or (
                N <= lc.K_BLOCK and "dot_blocks" in kw):
            continue
        with ctx():
            out[name] = decisions(reference(e, **kw))
    return out


# ---------------------------------------------------------------------------
# e. scaled and negated systems
# ---------------------------------------------------------------------------
def scale_csr(csr, s, sign=1.0):
    rp, ci, va = csr
    return rp, ci, sign * np.ldexp(va, s)


def same(a, b):
    """bits, +0.0 and -0.0 alike, NaN equal to NaN; a scalar stands for an array
    of it"""
    a, b = np.asarray(a) + 0.0, np.asarray(b) + 0.0
    if a.ndim and b.ndim and a.shape != b.shape:
        return False
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def scaled_hist(h, s):
    """the history times 2^s; the -1.0 of a slot never written stays"""
    return np.where(h == -1.0, -1.0, np.ldexp(h, s))


def a_scaled(e, s):
    """entry e on 2^s A (dinv times 2^-s) -> (result, probe)"""
    d = e.dinv()
    with Probe() as p:
        r = reference(e, M=Mat("%s*2^%d" % (e.matrix, s),
                               scale_csr(mat(e.matrix).csr, s)),
                      dinv=None if d is None else np.ldexp(d, -s))
    return r, p


def a_relation(base, r, s):
    return (decisions(r) == decisions(base) and same(r["X"], base["X"])
            and same(r["theta"], np.ldexp(base["theta"], s))
            and same(r["hist"], scaled_hist(base["hist"], s))
            and same(r["true_resnorm"], np.ldexp(base["true_resnorm"], s)))


def x_exponents(t):
    return (t, 0, -(t // 2))


def x_scaled(e, t):
    """entry e with the columns of X0 times 2^(t, 0, -(t // 2)) -> (result,
    probe)"""
    with Probe() as p:
        r = reference(e, X0=np.ldexp(e.X0(), np.array(x_exponents(t))[None, :]))
    return r, p


def x_relation(base, r):
    return decisions(r) == decisions(base) and all(
        same(r[n], base[n]) for n in ("X", "theta", "hist", "true_resnorm"))


def holds(kind, e, base, v):
    """the relation of `kind` ("a" or "x") at exponent v, with every probed
    value finite and normal"""
    r, p = a_scaled(e, v) if kind == "a" else x_scaled(e, v)
    ok = a_relation(base, r, v) if kind == "a" else x_relation(base, r)
    return ok and p.finite and p.normal


def bisect_edge(kind, e, base, inside, outside):
    """the last exponent between `inside` (holds) and `outside` (does not) at
    which the relation holds; the search takes the property to be monotone, the
    host test asserts the edge and its neighbour only"""
    assert holds(kind, e, base, inside) and not holds(kind, e, base, outside)
    step = 1 if outside > inside else -1
    while abs(outside - inside) > 1:
        mid = inside + step * (abs(outside - inside) // 2)
        if holds(kind, e, base, mid):
            inside = mid
        else:
            outside = mid
    return inside


_S1 = seed(1)
_T, _W = 1e-14, 1e-6
_P = dict(kmax=8, rtol=1e-3)  # group d and e: poisson11, nev 3, seed 1
E = Entry
TABLE = [
    # ---- a. restarts that recover, restarts that collapse -------------------
    # id, group, matrix, nev, X0, kmax, rtol, (k, status, restarts)
    E("a_diag6_l", "a", "diag1_6", 3, seed(2), 40, _T, (3, 0, 2),
      largest=True, cls="recovered", order="one"),  # masks 0b111, 0b11
    E("a_diag15_l", "a", "diag1_15", 8, seed(2), 40, _T, (2, 0, 1),
      largest=True, cls="recovered", order="one"),  # mask 0b111010
    E("a_tri33_conv", "a", "tri33", 8, seed(3), 60, 1e-8, (37, 0, 1),
      cls="recovered", order="one"),        # restart on the mask 0b11011011
    E("a_diag12", "a", "diag1_12", 3, _S1, 40, _T, (40, 0, 6), cls="kmax",
      order="one"),
    # theta_0 = -2.5e59 and status 0: noise that no pivot refused (cg.h)
    E("a_diag8", "a", "diag1_8", 3, seed(2), 40, _T, (40, 0, 3), cls="kmax",
      order="one", wild=True),
    E("a_tri16_8", "a", "tri16", 8, _S1, 60, _T, (60, 0, 2), cls="kmax",
      order="one"),                         # m = 24
    E("a_tri24_8", "a", "tri24", 8, _S1, 10, _T, (10, 0, 1), cls="kmax"),
    # (m = 24, all columns active)
    E("a_diag7", "a", "diag1_7", 4, _S1, 40, _T, (13, 1, 1), cls="collapsed",
      order="one"),
    E("a_tri16_4", "a", "tri16", 4, _S1, 60, _T, (44, 1, 1), cls="collapsed",
      order="one"),
    E("a_tri33_8", "a", "tri33", 8, _S1, 60, _T, (50, 1, 2), cls="collapsed",
      order="one"),                         # m = 24
    E("a_tri24_l", "a", "tri24", 8, seed(2), 60, _T, (33, 1, 1), largest=True,
      cls="collapsed", order="one"),
    E("a_diag9", "a", "diag1_9", 4, _S1, 40, _T, (1, 1, 0), cls="no_p"),
    E("a_diag10", "a", "diag1_10", 3, _S1, 40, _T, (2, 1, 0), cls="no_p"),
    E("a_tri7", "a", "tri7", 2, _S1, 60, _T, (2, 1, 0), cls="no_p"),
    E("a_tri25", "a", "tri25", 8, _S1, 60, _T, (2, 1, 0), cls="no_p"),
    E("a_diag12_8", "a", "diag1_12", 8, _S1, 40, _T, (0, 1, 0)),
    # ---- b. blocks that fill the space ----------------------------------------
    E("b_full1", "b", "diag1_1", 1, _S1, 10, _T, (0, 0, 0)),
    E("b_full3", "b", "diag1_3", 3, _S1, 10, _T, (0, 0, 0)),
    E("b_full8", "b", "diag1_8", 8, _S1, 10, _T, (0, 0, 0)),
    E("b_fulltri3", "b", "tri3", 3, _S1, 10, _T, (0, 0, 0)),
    E("b_fulltri8", "b", "tri8", 8, _S1, 10, _T, (0, 0, 0)),
    E("b_tri2", "b", "tri2", 1, _S1, 10, _T, (1, 0, 0)),
    E("b_diag2", "b", "diag1_2", 1, _S1, 10, _T, (1, 0, 0)),
    E("b_diag5", "b", "diag1_5", 2, _S1, 10, _T, (2, 0, 0),
      order="one"),
    E("b_tri5", "b", "tri5", 2, _S1, 10, _T, (1, 1, 0)),
    E("b_diag6", "b", "diag1_6", 2, _S1, 10, _T, (2, 0, 0)),
    E("b_tri6", "b", "tri6", 2, _S1, 10, _T, (2, 0, 0)),
    E("b_diag23", "b", "diag1_23", 8, _S1, 10, _T, (2, 0, 0),
      order="one"),
    E("b_tri23", "b", "tri23", 8, _S1, 10, _T, (1, 1, 0)),
    E("b_diag24", "b", "diag1_24", 8, _S1, 10, _T, (4, 0, 0),
      order="one"),
    E("b_zero1", "b", "diag0_0", 1, _S1, 5, _W, (0, 1, 0)),  # A = [0]
    E("b_zero1_atol", "b", "diag0_0", 1, _S1, 5, _W, (0, 0, 0), atol=1e-300),
    # ---- c. exact arithmetic ------------------------------------------------------
    E("c_exact", "c", "diag1_40", 3, units((0, 1, 2)), 10, _W, (0, 0, 0)),
    E("c_one_active", "c", "diag1_40", 3, units((0, 1, 2), ((5, 2, 0.5),)), 10,
      _W, (1, 0, 0)),
    E("c_theta0", "c", "diag0_39", 2, units((0, 1)), 10, _W, (0, 1, 0)),
    E("c_theta0_atol", "c", "diag0_39", 2, units((0, 1)), 10, _W, (0, 0, 0),
      atol=1e-300),
    E("c_theta0_random", "c", "diag0_39", 2, _S1, 60, _W, (60, 0, 0)),
    # 1 twice: the tie goes to the smaller index, X comes back as e1, e0, e2
    E("c_ties", "c", "ties9", 3, units((1, 0, 2)), 10, _W, (0, 0, 0)),
    # two equal columns, Gb = [[1, 1], [1, 1]]: the pivot 1 - 1 * 1 is exactly 0
    E("c_dup", "c", "diag1_40", 2, units((0, 0)), 10, _W, (0, 1, 0)),
    # ---- d. poisons: poisson11, nev 3, x0(N, 3, 1), kmax 8, rtol 1e-3 -----------
    E("d_dinv_nan", "d", "poisson11", 3, _S1, want=(0, 1, 0), kind="dinv",
      poison=("dinv", 17, NAN), **_P),
    E("d_dinv_inf", "d", "poisson11", 3, _S1, want=(0, 1, 0), kind="dinv",
      poison=("dinv", 17, INF), **_P),
    E("d_dinv_minf", "d", "poisson11", 3, _S1, want=(0, 1, 0), kind="dinv",
      poison=("dinv", 17, -INF), **_P),
    E("d_dinv_zero", "d", "poisson11", 3, _S1, want=(8, 0, 0), kind="dinv",
      poison=("dinv", 17, 0.0), **_P),
    E("d_a_inf", "d", "poisson11", 3, _S1, want=(0, 1, 0),
      poison=("a", 5, INF), **_P),
    E("d_a_minf", "d", "poisson11", 3, _S1, want=(0, 1, 0),
      poison=("a", 5, -INF), **_P),
    E("d_a_1e308", "d", "poisson11", 3, _S1, want=(0, 1, 0),
      poison=("a", 5, 1e308), **_P),
    E("d_a_1e200", "d", "poisson11", 3, _S1, want=(0, 1, 0),
      poison=("a", 5, 1e200), **_P),
    E("d_a_1e200_dinv", "d", "poisson11", 3, _S1, want=(0, 1, 0), kind="dinv",
      poison=("a", 5, 1e200), **_P),
    E("d_x_inf", "d", "poisson11", 3, seed(1, ((7, 1, INF),)), want=(0, 1, 0),
      finite=False, **_P),
    E("d_x_nan70", "d", "poisson11", 3, seed(1, ((70, 1, NAN),)),
      want=(0, 1, 0), finite=False, **_P),
    E("d_x_nanlast", "d", "poisson11", 3, seed(1, ((-1, 2, NAN),)),
      want=(0, 1, 0), finite=False, **_P),
    # ---- e. the bases of the relations ----------------------------------------------
    E("e_none", "e", "poisson11", 3, _S1, want=(8, 0, 0), **_P),
    E("e_dinv", "e", "poisson11", 3, _S1, want=(8, 0, 0), kind="dinv", **_P),
    E("e_none_l", "e", "poisson11", 3, _S1, want=None, largest=True, **_P),
    E("e_shift_l", "e", "shift11", 4, _S1, 10, 1e-3, None, largest=True),
]
BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)
CLASSES = ("recovered", "kmax", "collapsed", "no_p")
# tri(16) in two slabs of 8 rows: status 1 under every summation order tried
TWO_RANKS = "a_tri16_4"

# The working range found by bisect_edge on e_none and e_dinv: the last exponent
# at which the relation holds with every probed value finite and normal, then a
# point outside with the (k, status, restarts) the restatement gives there.
#   kind, entry, inside edge, (outside point, its decisions)
EDGES = [
    # 2^s A (W = R carries 2^s, so W^T A W carries 2^3s: a third of the range)
    ("a", "e_none", 339, (340, (0, 1, 0))),     # Ga overflows: status 1 at k = 0
    ("a", "e_none", -335, (-480, (5, 1, 0))),   # products underflow: a later 1
    # with dinv 2^-s W does not scale and only theta, AX, AW carry 2^s
    ("a", "e_dinv", 510, (511, (8, 0, 0))),
    ("a", "e_dinv", -490, (-1000, (0, 0, 0))),
    # X0 columns times 2^(t, 0, -(t // 2)): x0.x0 = 2^(2t + 8.8)
    ("x", "e_none", 507, (508, (0, 1, 0))),
    ("x", "e_none", -512, (-545, (0, 1, 0))),
]
# (dinv plays no part in the prologue, where the scale of X0 is divided out)
INSIDE = {"a": (40, -300), "x": (40, -300)}


def negated(e):
    """(-A, the other end of the spectrum) for entry e -> result"""
    M = Mat("-" + e.matrix, scale_csr(mat(e.matrix).csr, 0, -1.0))
    return lc.lobpcg_ref(M.spmv, None, e.X0(), e.kmax, e.rtol, e.atol,
                         not e.largest, None)


def negation_relation(base, r):
    """the same k and history, theta negated, |X| equal and every column as a
    whole of the same or the opposite sign"""
    if decisions(r) != decisions(base) or not same(r["hist"], base["hist"]):
        return False
    if not same(r["theta"], -base["theta"]):
        return False
    X, Y = r["X"], base["X"]
    return all(same(X[:, c], Y[:, c]) or same(X[:, c], -Y[:, c])
               for c in range(X.shape[1]))


NEGATED = ("e_none_l", "e_shift_l")


def before_failure(e, ref):
    """the blocks X may equal after status 1: X0 or the orthonormalised X0 when
    the prologue failed (no history), else the iterate of k"""
    if np.all(ref["hist"][:, 0] == -1.0):
        X0 = e.X0()
        out = [X0]
        with np.errstate(all="ignore"):
            g = lc.gram_sum(lc.gram_partials(X0, X0, lc.gram_grid(X0.shape[0])))
            full = (1 << e.nev) - 1
            rr = lc.rr_ref(g, e.nev, 1, full, 0, e.largest, mode=1)
            if rr["ok"]:
                out.append(lc.combine([X0], rr["coef"], rr["basis"], full,
                                      e.nev)[0])
        return out
    return [reference(e, kmax=ref["k"])["X"]]
