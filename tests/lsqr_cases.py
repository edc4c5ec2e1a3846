"""Cases and references for spmv::lsqr (LSQR on Matrix::mult and
Matrix::transpmult).  Nothing here touches a GPU: test_lsqr_host.py holds this
module to its targets, test_gpu_lsqr_kernels.py and test_gpu_lsqr.py run the
device on it.

  lsqr_ref         the recurrence of host/cg.h restated, word for word, on
                   `spmv`, `spmvt` and `dot` callables (every operation one
                   float64 rounding)
  lsqr_*           one reference per kernel of blas1_lsqr.hip, named after it;
                   the scalar ones (start, step) on Python floats; data sets E
                   and R, the lengths, depth and sum_bound are blas1_cases.py's
  stable_transpose the CSR of A^T with every column's entries in row order:
                   oracle.csr_spmv on it adds in Matrix::transpmult's order

Depth of the dot products of update_u and update_v, read off the kernels: a
thread adds 2 * kU products per trip (.x then .y, element order), trips as
stream_dot's; the odd tail element last; the shuffle tree and the wave slots of
spmv_block_sum; reduce, start and step are sum_partials.  That is
blas1_cases.depth(n, dot_blocks) unchanged; a term t * t carries one rounding.

Matrices (CSR triples of int32, int32, float64):
  convdiff11_C  7-point diffusion plus first-order upwind convection on 11^3:
                diagonal 6 + 3 C, upper neighbours -1, lower neighbours -1 - C
                (C = 0.5, 2): square, nonsymmetric
  poisson11     gmres_cases.poisson(11), for symmetric storage
  skew64        gmres_cases.skew(64): bicgstab breaks down on it at k = 0
  tall          900 x 300, 6 entries per row: 3 + uniform(0, 1) in column i mod
                300 and five of uniform(-0.5, 0.5) elsewhere, seeded; the
                columns are nearly orthogonal (condition number below 3)
  wide          its transpose, 300 x 900
Right-hand sides: "ones" = A.1 (consistent), "rand" = uniform(-1, 1), seeded
(inconsistent for `tall`)."""
import numpy as np

import gmres_cases as gc
from blas1_cases import f

KMAX, RTOL, LTOL = 600, 1e-10, 1e-10

# (matrix, right-hand side, damp) -> (k, status) of the restatement at RTOL,
# LTOL, KMAX with np.dot (dot_chunks64 gives 155 on the first row, the same
# counts on the others)
TABLE = {("convdiff11_0.5", "ones", 0.0): (156, 0),
         ("convdiff11_0.5", "rand", 0.0): (222, 0),
         ("convdiff11_2", "ones", 0.0): (134, 0),
         ("convdiff11_2", "rand", 0.0): (184, 0),
         ("tall", "ones", 0.0): (14, 0),
         ("tall", "rand", 0.0): (13, 1),
         ("tall", "rand", 0.5): (13, 1),
         ("wide", "ones", 0.0): (14, 0),
         ("wide", "rand", 0.0): (14, 0)}


# ---------------------------------------------------------------------------
# the scalar kernels (Python floats are float64; numpy's sqrt is correctly
# rounded)
# ---------------------------------------------------------------------------
STATE = ("alpha", "beta", "phibar", "rhobar", "anorm2", "psi2")
COEFS = ("ia", "ib", "t1", "t2")


def _sqrt(s):
    """IEEE square root of a float (a NaN passes)"""
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(s)))


def _div(a, b):
    """IEEE quotient of two floats (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def lsqr_start(uu, vv):
    """-> dict(done, status, hist_r0, hist_ar0 (None: not written), and, when
    the solve goes on, the state in front of the first step with ia and ib)"""
    beta = _sqrt(uu)
    if beta == 0.0:
        return dict(done=True, status=0, hist_r0=beta, hist_ar0=None)
    alpha = _sqrt(vv)
    if alpha == 0.0:
        return dict(done=True, status=2, hist_r0=beta, hist_ar0=alpha * beta)
    return dict(done=False, status=0, hist_r0=beta, hist_ar0=alpha * beta,
                alpha=alpha, beta=beta, ia=1.0 / alpha, ib=1.0 / beta,
                phibar=beta, rhobar=alpha, anorm2=0.0, psi2=0.0)


def lsqr_step(st, uu, vv, hist0, k, kmax, rtol, ltol, damp):
    """One step from the state `st` (the keys of STATE) -> dict: done, status,
    k (steps completed), res and ares (hist_r[k], hist_ar[k]); beta, phibar,
    rhobar, anorm2, psi2, t1; alpha, ia, ib, t2 when the solve goes on."""
    alpha = st["alpha"]
    beta = _sqrt(uu)
    alpha_n = _sqrt(vv) if beta != 0.0 else 0.0
    anorm2 = st["anorm2"] + alpha * alpha + beta * beta + damp * damp
    rhobar1 = _sqrt(st["rhobar"] * st["rhobar"] + damp * damp)
    cs1 = _div(st["rhobar"], rhobar1)
    sn1 = _div(damp, rhobar1)
    psi = sn1 * st["phibar"]
    phibar1 = cs1 * st["phibar"]
    psi2 = st["psi2"] + psi * psi
    rho = _sqrt(rhobar1 * rhobar1 + beta * beta)
    cs = _div(rhobar1, rho)
    sn = _div(beta, rho)
    theta = sn * alpha_n
    rhobar = -cs * alpha_n
    phi = cs * phibar1
    phibar = sn * phibar1
    res = _sqrt(phibar * phibar + psi2)
    ares = abs(phibar * alpha_n * cs)
    out = dict(done=True, status=0, k=k + 1, res=res, ares=ares, beta=beta,
               phibar=phibar, rhobar=rhobar, anorm2=anorm2, psi2=psi2,
               t1=_div(phi, rho))
    if beta == 0.0 or alpha_n == 0.0:
        out["status"] = 2
        return out
    if _div(res, hist0) < rtol:
        return out
    if _div(ares, _sqrt(anorm2) * res) < ltol:
        out["status"] = 1
        return out
    if k + 1 == kmax:
        return out
    out.update(done=False, alpha=alpha_n, ia=_div(1.0, alpha_n),
               ib=_div(1.0, beta), t2=_div(theta, rho))
    return out


# ---------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------
def lsqr_update_u(Av, ut, ia, alpha, ib):
    """-> ut = Av * ia - alpha * (ut * ib)"""
    return Av * f(ia) - f(alpha) * (ut * f(ib))


def lsqr_update_v(Atu, vt, uu, ia, first=False):
    """-> vn = Atu * (1 / beta) - beta * (vt * ia), beta = sqrt(uu) (first:
    without vt); None when beta == 0: the kernel leaves vt alone"""
    beta = np.sqrt(f(uu))
    if beta == 0.0:
        return None
    t = Atu * (f(1.0) / beta)
    return t if first else t - beta * (vt * f(ia))


def lsqr_update_xw(vt, w, x, t1, t2, ia, go_on=True):
    """-> (x, w): x = x + t1 * w; then w = vt * ia - t2 * w (not after `done`:
    w stays)"""
    xn = x + f(t1) * w
    return xn, (vt * f(ia) - f(t2) * w if go_on else np.array(w, np.float64))


def lsqr_scale(vt, ia):
    """update_xw with k = 0: w = vt * ia alone"""
    return vt * f(ia)


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
def lsqr_ref(spmv, spmvt, dot, b, kmax, rtol, ltol, damp):
    """-> (x, k, hist_r, hist_ar, status); spmv(q) = A q, spmvt(q) = A^T q over
    the owned columns, dot = the global dot product.  The recurrence of
    host/cg.h, word for word."""
    with np.errstate(all="ignore"):
        return _lsqr_ref(spmv, spmvt, dot, b, kmax, rtol, ltol, damp)


def _lsqr_ref(spmv, spmvt, dot, b, kmax, rtol, ltol, damp):
    sqrt = _sqrt
    ut = np.array(b, np.float64)
    beta = sqrt(dot(ut, ut))
    hist_r, hist_ar = [beta], [0.0]
    n = len(spmvt(ut))
    x = np.zeros(n)
    if beta == 0.0:
        return x, 0, np.array(hist_r), np.array(hist_ar), 0
    ib = _div(1.0, beta)
    vt = spmvt(ut) * f(ib)
    alpha = sqrt(dot(vt, vt))
    hist_ar[0] = alpha * beta
    if alpha == 0.0:
        return x, 0, np.array(hist_r), np.array(hist_ar), 2
    ia = _div(1.0, alpha)
    w = vt * f(ia)
    phibar, rhobar, anorm2, psi2 = beta, alpha, 0.0, 0.0
    k = status = 0
    while k < kmax:
        ut = spmv(vt) * f(ia) - f(alpha) * (ut * f(ib))
        beta = sqrt(dot(ut, ut))
        anorm2 = anorm2 + alpha * alpha + beta * beta + damp * damp
        if beta != 0.0:
            ib = _div(1.0, beta)
            vn = spmvt(ut) * f(ib) - f(beta) * (vt * f(ia))
            alpha_n = sqrt(dot(vn, vn))
        else:
            vn, alpha_n = vt, 0.0
        rhobar1 = sqrt(rhobar * rhobar + damp * damp)
        cs1 = _div(rhobar, rhobar1)
        sn1 = _div(damp, rhobar1)
        psi = sn1 * phibar
        phibar = cs1 * phibar
        psi2 = psi2 + psi * psi
        rho = sqrt(rhobar1 * rhobar1 + beta * beta)
        cs = _div(rhobar1, rho)
        sn = _div(beta, rho)
        theta = sn * alpha_n
        rhobar = -cs * alpha_n
        phi = cs * phibar
        phibar = sn * phibar
        x = x + f(_div(phi, rho)) * w
        k += 1
        hist_r.append(sqrt(phibar * phibar + psi2))
        hist_ar.append(abs(phibar * alpha_n * cs))
        if beta == 0.0 or alpha_n == 0.0:
            status = 2
            break
        if _div(hist_r[k], hist_r[0]) < rtol:
            break
        if _div(hist_ar[k], sqrt(anorm2) * hist_r[k]) < ltol:
            status = 1
            break
        vt = vn
        alpha = alpha_n
        ia = _div(1.0, alpha)
        w = vt * f(ia) - f(_div(theta, rho)) * w
    return x, k, np.array(hist_r), np.array(hist_ar), status


def dot_chunks64(a, b):
    """the second summation order: the products in chunks of 64, every chunk
    summed by numpy, the chunk sums left to right"""
    prod = np.asarray(a) * np.asarray(b)
    s = 0.0
    for i in range(0, len(prod), 64):
        s += float(np.sum(prod[i:i + 64]))
    return s


def dot_plain(a, b):
    """products rounded one by one and added left to right"""
    s = 0.0
    for t in (np.asarray(a, np.float64) * np.asarray(b, np.float64)).tolist():
        s += t
    return s


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def stable_transpose(csr, ncols):
    """CSR of A^T: entries sorted by column, ties in CSR (row) order"""
    rp, ci, va = csr
    rows = gc.row_of(rp).astype(np.int32)
    order = np.argsort(np.asarray(ci), kind="stable")
    tp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncols))])
    return tp.astype(np.int32), rows[order], np.asarray(va)[order].copy()


def convdiff(n, c):
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, 6.0 + 3.0 * c)]
    for d in range(3):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [np.full(len(a), -1.0 - c), np.full(len(a), -1.0)]
    return gc.to_csr(N, rows, cols, vals)


def tall(m=900, n=300):
    rng = np.random.default_rng(m + n)
    rows, cols, vals = [], [], []
    for i in range(m):
        main = i % n
        others = rng.choice(n - 1, 5, replace=False)
        others = others + (others >= main)
        c = np.concatenate([[main], others])
        v = np.concatenate([[3.0 + rng.uniform(0, 1)], rng.uniform(-0.5, 0.5, 5)])
        rows.append(np.full(6, i)), cols.append(c), vals.append(v)
    return gc.to_csr(m, rows, cols, vals)


_CSR = {}


def csr_by_name(name):
    """-> (csr, ncols)"""
    if name not in _CSR:
        if name.startswith("convdiff11_"):
            _CSR[name] = (convdiff(11, float(name[11:])), 1331)
        elif name == "poisson11":
            _CSR[name] = (gc.poisson(11), 1331)
        elif name == "skew64":
            _CSR[name] = (gc.skew(64), 64)
        elif name == "tall":
            _CSR[name] = (tall(), 300)
        elif name == "wide":
            _CSR[name] = (stable_transpose(tall(), 300), 900)
        else:
            raise KeyError(name)
    return _CSR[name]


def rhs(name, kind, spmv):
    csr, ncols = csr_by_name(name)
    nrows = len(csr[0]) - 1
    if kind == "ones":
        return spmv(np.ones(ncols))
    if kind == "rand":
        return np.random.default_rng(nrows + 1).uniform(-1, 1, nrows)
    raise KeyError(kind)


def dense(csr, ncols):
    rp, ci, va = csr
    A = np.zeros((len(rp) - 1, ncols))
    np.add.at(A, (gc.row_of(rp), ci), va)
    return A
