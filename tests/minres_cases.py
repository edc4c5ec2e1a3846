"""Cases and references for spmv::minres (preconditioned MINRES for symmetric,
possibly indefinite systems).  Nothing here touches a GPU: test_minres_host.py
holds this module to its targets, test_gpu_minres_kernels.py and
test_gpu_minres.py run the device on it.

  minres_ref       the recurrence of host/cg.h restated, word for word, on
                   `spmv`, `dot` and `minv` callables (every operation one
                   float64 rounding)
  minres_*         one reference per kernel of blas1_minres.hip, named after it;
                   the scalar ones (start, step) on Python floats with
                   math.sqrt; data sets E and R, the lengths, depth and
                   sum_bound are blas1_cases.py's

Depth of the dot products of minres_init and minres_update_r, read off the
kernels: a thread adds 2 * kU products per trip (.x then .y, element order),
trips as stream_dot's; the odd tail element last; the shuffle tree and the wave
slots of spmv_block_sum; minres_reduce is sum_partials.  That is
blas1_cases.depth(n, dot_blocks) unchanged; a term carries two roundings with a
dinv (t * (dinv * t)), one without.

Matrices (CSR triples of int32, int32, float64):
  shift11     7-point Poisson on 11^3 minus 1.0 I: 17 negative eigenvalues,
              smallest |lambda| 0.078 (sigma = 3 would be exactly singular)
  poisson11   the unshifted matrix: positive definite
  saddle500   [[K, B^T], [B, 0]], K = tridiag(-1, 2, -1) of order 400, B 100 x
              400 with B[i, 4i] = 1, B[i, 4i+1] = -1, B[i, (4i+5) mod 400] =
              0.5; the zero block stores explicit zeros on its diagonal; its
              dinv is 1 / diag K, then 1 / diag(B diag(K)^-1 B^T)
  sas         S shift11 S, S = diag(2^e), e uniform in -6..6; Jacobi's dinv is
              1 / |diag|
Right-hand sides: A.1 and A.uniform(-1, 1), seeded as in gmres_cases.py."""
import math

import numpy as np

import gmres_cases as gc
from blas1_cases import f

KMAX, RTOL = 600, 1e-10

# the CPU prototype's iteration counts at RTOL, KMAX (np.dot order)
TABLE = {("shift11", "ones", "none"): 36, ("shift11", "rand", "none"): 99,
         ("poisson11", "ones", "none"): 31, ("poisson11", "rand", "none"): 50,
         ("saddle500", "rand", "none"): 181, ("saddle500", "rand", "dinv"): 185}


# ---------------------------------------------------------------------------
# the scalar kernels (Python floats are float64; math.sqrt is correctly rounded)
# ---------------------------------------------------------------------------
STATE = ("beta", "oldb", "dbar", "epsln", "phibar", "cs", "sn")
COEFS = ("bob", "oldeps", "delta", "inv_gamma", "phi", "inv_beta")


def minres_start(ry):
    """-> dict(done, status, hist0 (None: not written), and, when the solve goes
    on, the state in front of the first step and inv_beta)"""
    ry = float(ry)
    if ry < 0.0:
        return dict(done=True, status=2, hist0=None)
    beta1 = math.sqrt(ry)
    if beta1 == 0.0:
        return dict(done=True, status=0, hist0=beta1)
    return dict(done=False, status=0, hist0=beta1, oldb=0.0, beta=beta1,
                dbar=0.0, epsln=0.0, phibar=beta1, cs=-1.0, sn=0.0,
                inv_beta=1.0 / beta1)


def minres_step(st, alfa, ry, hist0, k, kmax, rtol):
    """One step from the state `st` (the keys of STATE) -> dict: done, status,
    k (steps completed), res (hist[k] or None); the keys of STATE where the
    step got that far; oldeps, delta, inv_gamma, phi when x moves; inv_beta and
    bob when the solve goes on."""
    alfa, ry = float(alfa), float(ry)
    out = dict(done=True, status=0, k=k, res=None)
    if ry < 0.0:
        out["status"] = 2
        return out
    oldb = st["beta"]
    beta = math.sqrt(ry)
    oldeps = st["epsln"]
    delta = st["cs"] * st["dbar"] + st["sn"] * alfa
    gbar = st["sn"] * st["dbar"] - st["cs"] * alfa
    epsln = st["sn"] * beta
    dbar = -st["cs"] * beta
    gamma = math.sqrt(gbar * gbar + beta * beta)
    if gamma == 0.0:
        out["status"] = 3
        return out
    cs = gbar / gamma
    sn = beta / gamma
    phi = cs * st["phibar"]
    phibar = sn * st["phibar"]
    out.update(oldb=oldb, beta=beta, epsln=epsln, dbar=dbar, cs=cs, sn=sn,
               phibar=phibar, oldeps=oldeps, delta=delta,
               inv_gamma=1.0 / gamma, phi=phi, k=k + 1, res=abs(phibar))
    if beta == 0.0:
        out["status"] = 1
        return out
    if out["res"] / hist0 < rtol or k + 1 == kmax:
        return out
    out.update(done=False, inv_beta=1.0 / beta, bob=beta / oldb)
    return out


# ---------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------
def minres_init(r2, dinv=None):
    """-> y (dinv None: r2 itself, the kernel writes nothing)"""
    return r2 if dinv is None else dinv * r2


def minres_update_r(Av, r1, r2, dinv, alfa, beta, bob, first):
    """-> (t, y): t = (Av - bob*r1) - (alfa/beta)*r2 (first: without r1), y =
    dinv*t (dinv None: t itself, the kernel writes no y)"""
    q = f(alfa) / f(beta)
    t = np.array(Av, np.float64)
    if not first:
        t = t - f(bob) * r1
    t = t - q * r2
    return t, (t if dinv is None else dinv * t)


def minres_update_xwv(v, w1, w2, x, y, oldeps, delta, inv_gamma, phi, inv_beta,
                      go_on=True):
    """-> (w, x, v): w = ((v - oldeps*w1) - delta*w2) * inv_gamma; x = x +
    phi*w; v = y * inv_beta (not after `done`: v stays)"""
    w = ((v - f(oldeps) * w1) - f(delta) * w2) * f(inv_gamma)
    xn = x + f(phi) * w
    return w, xn, (y * f(inv_beta) if go_on else np.array(v, np.float64))


def minres_scale(y, inv_beta):
    """update_xwv with k = 0: v = y * inv_beta alone"""
    return y * f(inv_beta)


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
def minres_ref(spmv, dot, minv, b, kmax, rtol):
    """-> (x, k, history, status); spmv(q) = A q, dot = the global dot product,
    minv(q) = M^-1 q or None.  The recurrence of host/cg.h, word for word."""
    apply = (lambda q: q) if minv is None else minv
    b = np.asarray(b, np.float64)
    x = np.zeros(len(b))
    r1 = r2 = b.copy()
    y = apply(r2)
    ry = float(dot(r2, y))
    if ry < 0.0:
        return x, 0, np.array([0.0]), 2
    beta1 = math.sqrt(ry)
    hist = [beta1]
    if beta1 == 0.0:
        return x, 0, np.array(hist), 0
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w = np.zeros(len(b))
    w2 = np.zeros(len(b))
    k = status = 0
    v = y * f(1.0 / beta)
    while k < kmax:
        Av = spmv(v)
        alfa = float(dot(v, Av))
        if k == 0:
            t = Av - f(alfa / beta) * r2
        else:
            t = (Av - f(beta / oldb) * r1) - f(alfa / beta) * r2
        r1 = r2
        r2 = t
        y = apply(r2)
        ry = float(dot(r2, y))
        if ry < 0.0:
            status = 2
            break
        oldb = beta
        beta = math.sqrt(ry)
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = math.sqrt(gbar * gbar + beta * beta)
        if gamma == 0.0:
            status = 3
            break
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        w1 = w2
        w2 = w
        w = ((v - f(oldeps) * w1) - f(delta) * w2) * f(1.0 / gamma)
        x = x + f(phi) * w
        k += 1
        hist.append(abs(phibar))
        if beta == 0.0:
            status = 1
            break
        if hist[k] / hist[0] < rtol:
            break
        v = y * f(1.0 / beta)
    return x, k, np.array(hist), status


def dot_plain(a, b):
    """products rounded one by one and added left to right (np.dot may fuse)"""
    s = 0.0
    for t in (np.asarray(a, np.float64) * np.asarray(b, np.float64)).tolist():
        s += t
    return s


def dot_chunks64(a, b):
    """the prototype's second summation order: the products in chunks of 64,
    every chunk summed by numpy, the chunk sums left to right"""
    prod = np.asarray(a) * np.asarray(b)
    s = 0.0
    for i in range(0, len(prod), 64):
        s += float(np.sum(prod[i:i + 64]))
    return s


def cg_norms(spmv, b, kmax):
    """||r_k||, k = 0..kmax, of plain CG from x0 = 0 (np.dot)"""
    x = np.zeros(len(b))
    r = np.array(b, np.float64)
    p = r.copy()
    rr = float(np.dot(r, r))
    out = [math.sqrt(rr)]
    for _ in range(kmax):
        Ap = spmv(p)
        alpha = rr / float(np.dot(p, Ap))
        x = x + alpha * p
        r = r - alpha * Ap
        rr_new = float(np.dot(r, r))
        out.append(math.sqrt(rr_new))
        p = r + (rr_new / rr) * p
        rr = rr_new
    return np.array(out)


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def shifted_poisson(n, sigma):
    rp, ci, va = gc.poisson(n)
    va = va.copy()
    va[ci == gc.row_of(rp)] -= sigma
    return rp, ci, va


def saddle(nk=400, nb=100):
    i = np.arange(nk)
    j = np.arange(nb)
    brow = np.concatenate([j, j, j])
    bcol = np.concatenate([4 * j, 4 * j + 1, (4 * j + 5) % nk])
    bval = np.concatenate([np.full(nb, 1.0), np.full(nb, -1.0), np.full(nb, 0.5)])
    rows = [i, i[:-1], i[1:], bcol, nk + brow, nk + j]
    cols = [i, i[1:], i[:-1], nk + brow, bcol, nk + j]
    vals = [np.full(nk, 2.0), np.full(nk - 1, -1.0), np.full(nk - 1, -1.0), bval,
            bval, np.zeros(nb)]
    return gc.to_csr(nk + nb, rows, cols, vals)


def saddle_dinv(nk=400, nb=100):
    """1 / diag K, then 1 / diag(B diag(K)^-1 B^T) = 1 / ((1 + 1 + 0.25) / 2)"""
    return np.concatenate([np.full(nk, 0.5), np.full(nb, 1.0 / 1.125)])


def sas_scaling(N):
    e = np.random.default_rng(N).integers(-6, 7, N)
    return np.ldexp(1.0, e)


def csr_by_name(name):
    if name == "shift11":
        return shifted_poisson(11, 1.0)
    if name == "poisson11":
        return gc.poisson(11)
    if name == "saddle500":
        return saddle()
    if name == "sas":
        rp, ci, va = shifted_poisson(11, 1.0)
        s = sas_scaling(len(rp) - 1)
        return rp, ci, va * (s[gc.row_of(rp)] * s[ci])  # powers of 2: exact
    raise KeyError(name)


def dinv_by_name(name):
    if name == "saddle500":
        return saddle_dinv()
    return 1.0 / np.abs(gc.diag_of(csr_by_name(name)))


def rhs(csr, kind, spmv=None):
    N = len(csr[0]) - 1
    spmv = spmv or (lambda q: gc.csr_spmv(csr, q))
    if kind == "ones":
        return spmv(np.ones(N))
    if kind == "rand":
        return spmv(np.random.default_rng(N + 1).uniform(-1, 1, N))
    raise KeyError(kind)


def lower_csr(csr):
    """the strictly lower triangle and the diagonal of a symmetric matrix, as
    symmetric storage takes it"""
    rp, ci, va = csr
    rows = gc.row_of(rp)
    keep = ci < rows
    n = len(rp) - 1
    lrp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    return (lrp.astype(np.int32), ci[keep].astype(np.int32), va[keep].copy(),
            gc.diag_of(csr))
