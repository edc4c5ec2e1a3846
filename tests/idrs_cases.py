"""Cases and references for spmv::idrs (IDR(s), the biortho variant of van
Gijzen and Sonneveld 2011, on sign shadow vectors, right preconditioning).
Nothing here touches a GPU: test_idrs_host.py holds this module to its targets,
test_gpu_idrs_kernels.py and test_gpu_idrs.py run the device on it.

  shadow_signs   the s shadow vectors of rows row0 .. row0 + n - 1: one 64-bit
                 hash of the GLOBAL row index, bit j clear -> +1.0, set -> -1.0
  idrs_ref       the recurrence of host/cg.h restated on `spmv`, `dot` and
                 `minv` callables (every operation one float64 rounding)
  idrs_step, idrs_biortho, idrs_omega, idrs_prep, idrs_update,
  idrs_omega_update, idrs_sign_sums
                 one reference per kernel of blas1_idrs.hip, named after it; the
                 scalar ones on Python floats and a state dict with the fields
                 of IdrsScalars
  idrs_compose   the same solve, made of the kernel references alone, in the
                 launch sequence of idrs() on one rank
  sign_partials  the partial rows idrs_sign_dot leaves ([j][workgroup]): a
                 thread adds +-w of its elements in stream_dot's order, so the
                 depth model of blas1_cases.depth(n, dot_blocks) applies

Matrices (CSR triples of int32, int32, float64): cdpe(n, pe), 3-D central
difference convection-diffusion at cell Peclet number pe on n^3 (diagonal 6,
off-diagonals -(1 + pe) upwind of a row and -(1 - pe) downwind); skew2(n), 2x2
blocks [[0, 2], [-2, 0]]; and those of gmres_cases.py."""
import math

import numpy as np

import amg_cases
import cgs_cases as cc
import gmres_cases as gc
import ilu0_cases
from blas1_cases import f
from gmres_cases import (convdiff, csr_by_name, diag_of,  # noqa: F401
                         dot_chunked, poisson, to_csr)

MAX_S = 8
KMAX, RTOL, KAPPA = 2000, 1e-10, 0.7
# rows of the partial array and slots of `red` (spmv_hip.h)
ROW_RR, ROW_TR, ROW_TT, ROWS = 8, 9, 10, 11
_MASK = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------
# shadow vectors
# ---------------------------------------------------------------------------
def sign_hash(gi, seed=0):
    """the 64-bit word of global row gi (Python ints, wraparound spelled out)"""
    z = (gi + seed * _GOLD + _GOLD) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def shadow_signs(row0, n, s, seed=0):
    """-> P [s, n] of +1.0 / -1.0 for the global rows row0 .. row0 + n - 1"""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=u) + u((row0 + seed * _GOLD + _GOLD) & _MASK)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z ^= z >> u(31)
    return np.array([np.where((z >> u(j)) & u(1), -1.0, 1.0) for j in range(s)]
                    ).reshape(s, n)


# ---------------------------------------------------------------------------
# the scalar kernels: a state dict with the fields of IdrsScalars
# ---------------------------------------------------------------------------
def _sqrt(v):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def _sub(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) - np.float64(b))


def new_state(s, rtol, kmax, kappa=KAPPA):
    """the state spmv_hip_idrs_ws_reset leaves: M = I, om = 1"""
    M = [[1.0 if i == j else 0.0 for j in range(MAX_S)] for i in range(MAX_S)]
    return dict(rtol=float(rtol), kappa=float(kappa), om=1.0, rr=0.0, hist0=0.0,
                be=0.0, f=[0.0] * MAX_S, c=[0.0] * MAX_S, a=[0.0] * MAX_S,
                red=[0.0] * ROWS, M=M, done=0, kstop=-1, status=0, k=0,
                kmax=int(kmax), s=int(s))


def _raise(st, status):
    st.update(done=1, kstop=st["k"], status=status)


def _coef(st, q):
    """c_q .. c_{s-1} by forward substitution on M[q:, q:]"""
    s, M, c = st["s"], st["M"], st["c"]
    for i in range(q, s):
        t = st["f"][i]
        for j in range(q, i):
            t = _sub(t, _mul(M[i][j], c[j]))
        c[i] = _div(t, M[i][i])


def _goes_on(st, hist):
    """k += 1, the history and the stop test; a NaN goes on"""
    if st["k"] >= st["kmax"]:  # (no room in the history: the host never asks)
        _raise(st, 0)
        return False
    st["k"] += 1
    k = st["k"]
    hist[k] = _sqrt(st["rr"])
    if _div(hist[k], st["hist0"]) < st["rtol"] or k == st["kmax"]:
        _raise(st, 0)
        return False
    return True


def idrs_step(st, q, sums, rr, hist):
    """q = -1: start (f = sums, hist[0]); 0 <= q < s: the end of inner step q
    (rr; the update of f); q = s: the end of the om step (rr, f = sums).  Each
    leaves the coefficients c of the step that follows."""
    if st["done"]:
        return
    s = st["s"]
    st["rr"] = float(rr)
    if q < 0:
        st["f"][:s] = [float(v) for v in sums[:s]]
        st["hist0"] = hist[0] = _sqrt(rr)
        if rr == 0.0 or st["kmax"] == 0:
            return _raise(st, 0)
        return _coef(st, 0)
    if q == s:
        st["f"][:s] = [float(v) for v in sums[:s]]
        if _goes_on(st, hist):
            _coef(st, 0)
        return
    if not _goes_on(st, hist):
        return
    for i in range(q + 1, s):
        st["f"][i] = _sub(st["f"][i], _mul(st["be"], st["M"][i][q]))
    if q + 1 < s:
        _coef(st, q + 1)


def idrs_biortho(st, q, h):
    """h = P^T g of the un-orthogonalised g: a_0 .. a_{q-1}, column q of M, be;
    a zero or non-finite pivot ends the solve with status 1"""
    if st["done"]:
        return
    s, M, a = st["s"], st["M"], st["a"]
    for i in range(q):
        t = float(h[i])
        for j in range(i):
            t = _sub(t, _mul(a[j], M[i][j]))
        a[i] = _div(t, M[i][i])
    for i in range(q, s):
        t = float(h[i])
        for j in range(q):
            t = _sub(t, _mul(a[j], M[i][j]))
        M[i][q] = t
    piv = M[q][q]
    if piv == 0.0 or not math.isfinite(piv):
        return _raise(st, 1)
    st["be"] = _div(st["f"][q], piv)


def idrs_omega(st, tr, tt):
    """om = tr / tt, lengthened where |rho| < kappa; status 2 exits"""
    if st["done"]:
        return
    if not tt > 0.0:
        return _raise(st, 2)
    om = _div(tr, tt)
    rho = _div(tr, _mul(_sqrt(tt), _sqrt(st["rr"])))
    if abs(rho) < st["kappa"]:
        om = _div(_mul(om, st["kappa"]), abs(rho))
    if om == 0.0 or not math.isfinite(om):
        return _raise(st, 2)
    st["om"] = om


# ---------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------
FUSED, STORE_V, FROM_VH, PLAIN = range(4)


def idrs_prep(st, q, mode, r, G, U, dinv=None, vh=None):
    """-> the vector the kernel writes, or None where it writes nothing.
    FUSED:   u = om*(dinv*v) + c_q u_q + ..., v = r - c_q g_q - ... (registers)
    STORE_V: v
    FROM_VH: u = om*vh + c_q u_q + ...  (vh = B^-1 v, in place)
    PLAIN:   dinv*r, or r               (the vh of the om step)"""
    if st["done"]:
        return None
    s, c = st["s"], st["c"]
    with np.errstate(all="ignore"):
        if mode == PLAIN:
            return np.array(r) if dinv is None else dinv * r
        if mode != FROM_VH:
            v = np.array(r, np.float64)
            for i in range(q, s):
                v = v - f(c[i]) * G[i]
            if mode == STORE_V:
                return v
            vh = v if dinv is None else dinv * v
        u = f(st["om"]) * vh
        for i in range(q, s):
            u = u + f(c[i]) * U[i]
        return u


def idrs_update(st, q, g, u, G, U, r, x):
    """-> (g_q, u_q, r, x) or None where the kernel writes nothing"""
    if st["done"]:
        return None
    a, be = st["a"], f(st["be"])
    with np.errstate(all="ignore"):
        g, u = np.array(g, np.float64), np.array(u, np.float64)
        for i in range(q):
            g = g - f(a[i]) * G[i]
            u = u - f(a[i]) * U[i]
        return g, u, r - be * g, x + be * u


def idrs_omega_update(st, t, vh, r, x):
    """-> (r, x) or None"""
    if st["done"]:
        return None
    with np.errstate(all="ignore"):
        om = f(st["om"])
        return r - om * t, x + om * vh


def idrs_sign_sums(dot, P, w):
    """P^T w on a `dot` callable (p_j * w is exact)"""
    return [float(dot(p, w)) for p in P]


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
def idrs_ref(spmv, dot, minv, b, s, kmax, rtol, kappa=KAPPA, seed=0, row0=0):
    """-> (x, k, history, status).  The recurrence of host/cg.h, word for word;
    spmv(q) = A q, dot = the global dot product, minv(q) = B^-1 q or None."""
    with np.errstate(all="ignore"):
        return _idrs_ref(spmv, dot, minv, b, s, kmax, rtol, kappa, seed, row0)


def _idrs_ref(spmv, dot, minv, b, s, kmax, rtol, kappa, seed, row0):
    pre = (lambda q: q) if minv is None else minv
    b = np.asarray(b, np.float64)
    n = len(b)
    P = shadow_signs(row0, n, s, seed)
    x, r = np.zeros(n), b.copy()
    G, U = np.zeros((s, n)), np.zeros((s, n))
    M = [[1.0 if i == j else 0.0 for j in range(s)] for i in range(s)]
    om, k = 1.0, 0
    fv = [float(dot(p, r)) for p in P]
    rr = float(dot(r, r))
    hist = [_sqrt(rr)]
    if rr == 0.0 or kmax == 0:
        return x, 0, np.array(hist), 0

    def stop():
        return _div(hist[k], hist[0]) < rtol or k == kmax

    while True:
        for q in range(s):
            c = [0.0] * s
            for i in range(q, s):
                t = fv[i]
                for j in range(q, i):
                    t = _sub(t, _mul(M[i][j], c[j]))
                c[i] = _div(t, M[i][i])
            v = r.copy()
            for i in range(q, s):
                v = v - f(c[i]) * G[i]
            u = f(om) * pre(v)
            for i in range(q, s):
                u = u + f(c[i]) * U[i]
            g = spmv(u)
            h = [float(dot(p, g)) for p in P]
            a = [0.0] * q
            for i in range(q):
                t = h[i]
                for j in range(i):
                    t = _sub(t, _mul(a[j], M[i][j]))
                a[i] = _div(t, M[i][i])
            for i in range(q):
                g = g - f(a[i]) * G[i]
                u = u - f(a[i]) * U[i]
            for i in range(q, s):
                t = h[i]
                for j in range(q):
                    t = _sub(t, _mul(a[j], M[i][j]))
                M[i][q] = t
            if M[q][q] == 0.0 or not math.isfinite(M[q][q]):
                return x, k, np.array(hist), 1
            G[q], U[q] = g, u
            be = _div(fv[q], M[q][q])
            r = r - f(be) * g
            x = x + f(be) * u
            rr = float(dot(r, r))
            k += 1
            hist.append(_sqrt(rr))
            if stop():
                return x, k, np.array(hist), 0
            for i in range(q + 1, s):
                fv[i] = _sub(fv[i], _mul(be, M[i][q]))
        vh = pre(r)
        t = spmv(vh)
        tr, tt = float(dot(t, r)), float(dot(t, t))
        if not tt > 0.0:
            return x, k, np.array(hist), 2
        om = _div(tr, tt)
        rho = _div(tr, _mul(_sqrt(tt), _sqrt(rr)))
        if abs(rho) < kappa:
            om = _div(_mul(om, kappa), abs(rho))
        if om == 0.0 or not math.isfinite(om):
            return x, k, np.array(hist), 2
        r = r - f(om) * t
        x = x + f(om) * vh
        rr = float(dot(r, r))
        fv = [float(dot(p, r)) for p in P]
        k += 1
        hist.append(_sqrt(rr))
        if stop():
            return x, k, np.array(hist), 0


def idrs_compose(spmv, dot, minv, b, s, kmax, rtol, kappa=KAPPA, seed=0,
                 row0=0, dinv=None):
    """idrs_ref made of the kernel references: the launch sequence of idrs() on
    one rank -> (x, k, history, status).  dinv: the fused path (minv is then
    ignored); minv: the STORE_V / FROM_VH path."""
    b = np.asarray(b, np.float64)
    n = len(b)
    P = shadow_signs(row0, n, s, seed)
    st = new_state(s, rtol, kmax, kappa)
    hist = np.zeros(kmax + 1)
    x, r = np.zeros(n), b.copy()
    G, U = np.zeros((s, n)), np.zeros((s, n))
    fused = minv is None or dinv is not None
    with np.errstate(all="ignore"):
        idrs_step(st, -1, idrs_sign_sums(dot, P, r), float(dot(r, r)), hist)
        steps = 0
        while steps < kmax and not st["done"]:
            for q in range(s):
                if steps == kmax or st["done"]:
                    break
                steps += 1
                if fused:
                    u = idrs_prep(st, q, FUSED, r, G, U, dinv=dinv)
                else:
                    v = idrs_prep(st, q, STORE_V, r, G, U)
                    u = idrs_prep(st, q, FROM_VH, r, G, U, vh=minv(v))
                g = spmv(u)
                idrs_biortho(st, q, idrs_sign_sums(dot, P, g))
                out = idrs_update(st, q, g, u, G, U, r, x)
                rr = 0.0
                if out is not None:
                    G[q], U[q], r, x = out
                    rr = float(dot(r, r))
                idrs_step(st, q, None, rr, hist)
            else:
                if steps == kmax or st["done"]:
                    break
                steps += 1
                vh = idrs_prep(st, s, PLAIN, r, G, U, dinv=dinv) if fused \
                    else minv(r)
                t = spmv(vh)
                idrs_omega(st, float(dot(t, r)), float(dot(t, t)))
                out = idrs_omega_update(st, t, vh, r, x)
                rr, sums = 0.0, [0.0] * s
                if out is not None:
                    r, x = out
                    rr, sums = float(dot(r, r)), idrs_sign_sums(dot, P, r)
                idrs_step(st, s, sums, rr, hist)
    k = st["k"]
    return x, k, hist[:k + 1].copy(), st["status"]


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def sign_partials(w, P, dot_blocks, with_ww=False):
    """the rows idrs_sign_dot leaves: [len(P) (+ 1), dot_blocks]"""
    rows = [cc.stream_partials(p, w, dot_blocks) for p in P]
    if with_ww:
        rows.append(cc.stream_partials(w, w, dot_blocks))
    return np.array(rows)


def device_dot(dot_blocks):
    return cc.device_dot(dot_blocks)


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def cdpe(n, pe):
    """central differences for -lap u + w.grad u on n^3, cell Peclet number pe
    in every direction: diagonal 6, -(1 + pe) to the upwind neighbour, -(1 -
    pe) to the downwind one"""
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, 6.0)]
    for d in range(3):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [np.full(len(a), -(1.0 + pe)), np.full(len(a), -(1.0 - pe))]
    return to_csr(N, rows, cols, vals)


def cdpe_rhs(N):
    return np.sin(0.37 * np.arange(N)) + 0.5


def skew2(n):
    assert n % 2 == 0
    i = np.arange(n // 2)
    a = np.full(n // 2, 2.0)
    return to_csr(n, [2 * i, 2 * i + 1], [2 * i + 1, 2 * i], [a, -a])


def identity(n):
    i = np.arange(n)
    return to_csr(n, [i], [i], [np.ones(n)])


def opposite_rows(seed=0, row0=0):
    """the first two rows whose sign of shadow vector 0 differs"""
    P = shadow_signs(row0, 64, 1, seed)[0]
    i = 0
    j = int(np.flatnonzero(P != P[0])[0])
    return i, j


def fast_spmv(csr):
    """gmres_cases.csr_spmv's order (row sums left to right, the product
    rounded first), one numpy pass per entry position"""
    rp, ci, va = csr
    n = len(rp) - 1
    rows = np.arange(n)
    width = int(np.diff(rp).max()) if n else 0

    def spmv(x):
        with np.errstate(all="ignore"):
            out = np.zeros(n)
            for e in range(width):
                has = rp[rows] + e < rp[rows + 1]
                at = rp[rows[has]] + e
                out[has] = out[has] + va[at] * x[ci[at]]
            return out
    return spmv


def dense(csr):
    return cc.dense(csr)


def case(name):
    """-> (csr, b): the three systems of the whole-solve tests and poisson8"""
    if name == "cdpe10":
        csr = cdpe(10, 5.0)
        return csr, cdpe_rhs(1000)
    csr = csr_by_name(name)
    N = len(csr[0]) - 1
    return csr, fast_spmv(csr)(np.random.default_rng(N + 3).uniform(-1, 1, N))


CASES = ("convdiff8", "banded2000", "cdpe10")

# ---------------------------------------------------------------------------
# the whole solves of test_idrs_host.py and test_gpu_idrs.py: the bar, the
# spread of the restatement's iteration counts, and its solves, computed once
# ---------------------------------------------------------------------------
L = 2048  # a dot_blocks for the device's summation order
# the TRUE relative residual of every whole solve: 4 * 9.661e-11, the largest
# the restatement ends with in either summation order (test_idrs_host.py)
BAR = 3.9e-10
# |k(device order) - k(chunked order)| of the restatement where it is not zero,
# by (matrix, s, preconditioner)
SPREAD = {("cdpe10", 4, None): 2, ("cdpe10", 8, None): 1}
# (matrix, s, preconditioner) of the preconditioned solves and of poisson8
PRECONDITIONED = (("convdiff8", 4, "dinv"), ("convdiff8", 4, "sgs"),
                  ("convdiff8", 4, "ilu0"), ("poisson8", 4, "amg"),
                  ("poisson8", 4, "cheb"))
PLAIN_EXTRA = (("poisson8", 1, None), ("poisson8", 4, None))
CHEB = (3, 0.1, 2.2)  # degree and bounds of the Chebyshev runs, in dinv*A

_CACHE = {}


def spread(name, s, pre=None):
    return SPREAD.get((name, s, pre), 0)


def problem(name):
    """-> (csr, b, spmv, dense A)"""
    if name not in _CACHE:
        csr, b = case(name)
        _CACHE[name] = (csr, b, fast_spmv(csr), dense(csr))
    return _CACHE[name]


def minv_of(name, pre):
    """the numpy restatement of a preconditioner on problem(name), or None"""
    key = (name, "minv", pre)
    if key not in _CACHE:
        csr, _, spmv, _ = problem(name)
        N = len(csr[0]) - 1
        if pre is None:
            m = None
        elif pre == "dinv":
            dinv = 1.0 / diag_of(csr)
            m = lambda q: dinv * q  # noqa: E731
        elif pre == "sgs":
            m = gc.SgsRef(csr)
        elif pre == "ilu0":
            ref = ilu0_cases.Ilu0Ref(csr, N, gc.sgs_color(csr), False)
            fac = ref.factor()
            m = lambda q: ref.apply(fac, q)  # noqa: E731
        elif pre == "amg":
            m = amg_cases.AmgRef(csr, N).apply
        elif pre == "cheb":
            dinv = 1.0 / diag_of(csr)
            m = lambda q: gc.chebyshev_apply(spmv, q, dinv, *CHEB)  # noqa: E731
        else:
            raise KeyError(pre)
        _CACHE[key] = m
    return _CACHE[key]


def solve(name, s, order, pre=None, **kw):
    """idrs_ref on problem(name) in the summation order "device" or "chunked"
    -> (x, k, history, status)"""
    key = (name, s, order, pre, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _, b, spmv, _ = problem(name)
        dot = device_dot(L) if order == "device" else dot_chunked
        _CACHE[key] = idrs_ref(spmv, dot, minv_of(name, pre), b, s, KMAX, RTOL,
                               **kw)
    return _CACHE[key]
