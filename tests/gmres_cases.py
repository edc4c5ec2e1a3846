"""Cases and references for spmv::gmres (restarted GMRES, right preconditioning,
CGS2).  Nothing here touches a GPU: test_gmres_host.py holds this module to its
targets, test_gpu_gmres_kernels.py and test_gpu_gmres.py run the device on it.

  gmres_ref        the recurrence of host/cg.h restated on `spmv`, `dot` and
                   `minv` callables (every operation one float64 rounding)
  gmres_*          one numpy reference per kernel of blas1_gmres.hip, named
                   after it; data sets E and R, the lengths, depth and sum_bound
                   are blas1_cases.py's

Depth of one v_i . w of gmres_multi_dot + gmres_reduce, read off the kernel: a
thread adds 2 * kU products per trip into the accumulator of v_i (.x then .y,
element order), trips as stream_dot's; the odd tail element last; the shuffle
tree and the wave slots of spmv_block_sum; gmres_reduce is sum_partials on row
i.  That is blas1_cases.depth(n, dot_blocks) unchanged: the grouping of the
basis vectors changes which loads are in flight, not the chain of additions.
The w.w of the second gmres_multi_axpy and the r.r of gmres_residual have the
same chain.

Matrices restate those of test_gpu_bicgstab.py (convdiff, banded, S A S) and
add the skew 2x2-block matrix bicgstab breaks down on."""
import math

import numpy as np

import blas1_cases as bc
from blas1_cases import f

MAX_RESTART = 64
GROUP = 8
BASIS_SIZES = (1, 2, GROUP, GROUP + 1, MAX_RESTART)
KMAX, RTOL = 400, 1e-10


# ---------------------------------------------------------------------------
# the scalar parts (Python floats are float64; math.sqrt is correctly rounded)
# ---------------------------------------------------------------------------
def rotation(a, b):
    """the new rotation from a = col_j, b = col_{j+1} -> (c, s)"""
    a, b = float(a), float(b)
    if b == 0.0:
        return 1.0, 0.0
    if abs(b) > abs(a):
        tau = a / b
        s = 1.0 / math.sqrt(1.0 + tau * tau)
        return s * tau, s
    tau = b / a
    c = 1.0 / math.sqrt(1.0 + tau * tau)
    return c, c * tau


def gmres_givens(j, h, ww, cs, sn, g, hist0, k, kmax, rtol):
    """Inner step j after the second pass: h[0..j] the summed coefficients, ww
    = w.w; cs, sn the rotations 0..j-1, g[0..j].  -> dict(col (R's column j,
    j + 1 entries, None when discarded), cs, sn, g (j + 2 entries), k, jn, res
    (hist[k] or None), done, status, inv (None unless the loop goes on))"""
    hn = math.sqrt(float(ww))
    col = [float(v) for v in h[:j + 1]] + [hn]
    for i in range(j):
        t = cs[i] * col[i] + sn[i] * col[i + 1]
        col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
        col[i] = t
    a, b = col[j], col[j + 1]
    c, s = rotation(a, b)
    rjj = c * a + s * b
    out = dict(col=None, cs=list(cs[:j]), sn=list(sn[:j]), g=list(g[:j + 1]),
               k=k, jn=j, res=None, done=True, status=2, inv=None)
    if rjj == 0.0:
        return out
    gj = float(g[j])
    out.update(col=col[:j] + [rjj], cs=out["cs"] + [c], sn=out["sn"] + [s],
               g=list(g[:j]) + [c * gj, -s * gj], k=k + 1, jn=j + 1)
    out["res"] = abs(out["g"][j + 1])
    if hn == 0.0:
        out["status"] = 1
        return out
    out["status"] = 0
    if out["res"] / hist0 < rtol or k + 1 == kmax:
        return out
    out.update(done=False, inv=1.0 / hn)
    return out


def gmres_solve_y(R, g, jn):
    """back substitution on the jn columns kept; R[i][l] = R_il"""
    y = [0.0] * jn
    for i in range(jn - 1, -1, -1):
        s = float(g[i])
        for l in range(i + 1, jn):
            s = s - float(R[i][l]) * y[l]
        y[i] = s / float(R[i][i])
    return y


# ---------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------
def gmres_multi_axpy(V, coef, w):
    """w - coef_0 v_0 - ... in that order, the multiply rounded first"""
    w = np.array(w, np.float64)
    for v, a in zip(V, coef):
        w = w - f(a) * v
    return w


def gmres_scale(inv, src):
    return src * f(inv)


def gmres_combine(V, y):
    u = f(y[0]) * V[0]
    for v, a in zip(V[1:], y[1:]):
        u = u + f(a) * v
    return u


def gmres_add(z, x):
    return x + z


def gmres_residual(b, Ax=None):
    return np.array(b, np.float64) if Ax is None else b - Ax


def gmres_diag(dinv, v):
    return dinv * v


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
def gmres_ref(spmv, dot, minv, b, m, kmax, rtol):
    """-> (x, k, history, status); spmv(q) = A q, dot = the global dot product,
    minv(q) = M^-1 q or None"""
    apply = (lambda q: q) if minv is None else minv
    b = np.asarray(b, np.float64)
    n = len(b)
    x = np.zeros(n)
    r = b.copy()
    rr0 = dot(r, r)
    hist = [math.sqrt(rr0)]
    k = status = 0
    if rr0 == 0.0 or kmax == 0:  # (kmax == 0: no step is taken, as in cg())
        return x, 0, np.array(hist), 0
    first = True
    while True:
        beta = hist[0] if first else math.sqrt(dot(r, r))
        first = False
        V = [r * f(1.0 / beta)]
        g = [beta]
        cs, sn, R = [], [], [[0.0] * m for _ in range(m)]
        jn, early = 0, False
        for j in range(m):
            w = spmv(apply(V[j]))
            h = [dot(v, w) for v in V]
            w = gmres_multi_axpy(V, h, w)
            c = [dot(v, w) for v in V]
            w = gmres_multi_axpy(V, c, w)
            h = [hi + ci for hi, ci in zip(h, c)]
            ww = dot(w, w)
            st = gmres_givens(j, h, ww, cs, sn, g, hist[0], k, kmax, rtol)
            if st["col"] is None:
                status, early = 2, True
                break
            for i in range(j + 1):
                R[i][j] = st["col"][i]
            cs, sn, g, k, jn = st["cs"], st["sn"], st["g"], st["k"], st["jn"]
            hist.append(st["res"])
            if st["done"]:
                status, early = st["status"], True
                break
            V.append(w * f(st["inv"]))
        if jn > 0:
            y = gmres_solve_y(R, g, jn)
            x = x + apply(gmres_combine(V[:jn], y))
        if early:
            return x, k, np.array(hist), status
        r = b - spmv(x)
        if dot(r, r) == 0.0:
            return x, k, np.array(hist), status


def dot_chunked(a, b):
    """the second summation order of test_gpu_bicgstab.py: chunks of 1 024
    products summed pairwise, the chunk sums then left to right"""
    prod = np.asarray(a) * np.asarray(b)
    pad = (-len(prod)) % 1024
    v = np.concatenate([prod, np.zeros(pad)]).reshape(-1, 1024)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    s = 0.0
    for c in v[:, 0]:
        s += float(c)
    return s


# ---------------------------------------------------------------------------
# matrices (CSR triples of int32, int32, float64)
# ---------------------------------------------------------------------------
def to_csr(n, rows, cols, vals):
    rows, cols, vals = map(np.concatenate, (rows, cols, vals))
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32),
            vals[order].astype(np.float64))


def convdiff(n):
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, 7.6)]
    for d, c in enumerate((0.9, 0.5, 0.2)):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [-(1 + c) * (1 + 0.3 * np.sin(b.astype(np.float64))),
                 -(1 + 0.3 * np.cos(a.astype(np.float64)))]
    return to_csr(N, rows, cols, vals)


def banded(n):
    i = np.arange(n)
    rows, cols, vals = [i], [i], [6.0 + 0.3 * np.sin(i)]
    for d in (1, 37, 600):
        a, b = i[:-d], i[:-d] + d
        rows += [a, b]
        cols += [b, a]
        vals += [-(0.3 + 0.25 * np.sin((a + 2 * b).astype(np.float64))),
                 -(0.5 + 0.4 * np.cos((a + b).astype(np.float64)))]
    return to_csr(n, rows, cols, vals)


def skew(n):
    """2x2 blocks [[0, a], [-a, 0]], a = 1 + 0.5 (1 + sin i), i the block;
    n even.  b.(A b) = 0 for every b: bicgstab stops at k = 0."""
    assert n % 2 == 0
    i = np.arange(n // 2)
    a = 1.0 + 0.5 * (1.0 + np.sin(i.astype(np.float64)))
    return to_csr(n, [2 * i, 2 * i + 1], [2 * i + 1, 2 * i], [a, -a])


def poisson(n):
    """the symmetric 7-point Poisson matrix on n^3, diagonal 6"""
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, 6.0)]
    for d in range(3):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [np.full(len(a), -1.0)] * 2
    return to_csr(N, rows, cols, vals)


def row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def scaled(csr):
    """S A S, the S of test_gpu_pcg.py"""
    rp, ci, va = csr
    N = len(rp) - 1
    s = 10.0 ** np.random.default_rng(N).uniform(-1, 1, N)
    return rp, ci, va * (s[row_of(rp)] * s[ci])


def diag_of(csr):
    rp, ci, va = csr
    rows = row_of(rp)
    d = np.zeros(len(rp) - 1)
    on = ci == rows
    d[rows[on]] = va[on]
    return d


def csr_spmv(csr, x):
    """row sums left to right, product rounded first (oracle.csr_spmv's order)"""
    rp, ci, va = csr
    out = np.zeros(len(rp) - 1)
    prod = va * x[ci]
    for i in range(len(out)):
        s = 0.0
        for e in range(rp[i], rp[i + 1]):
            s += prod[e]
        out[i] = s
    return out


def csr_by_name(name):
    if name.startswith("convdiff"):
        return convdiff(int(name[8:]))
    if name.startswith("banded"):
        return banded(int(name[6:]))
    if name.startswith("skew"):
        return skew(int(name[4:]))
    if name.startswith("poisson"):
        return poisson(int(name[7:]))
    raise KeyError(name)


# ---------------------------------------------------------------------------
# preconditioners, restated (test_gpu_chebyshev.py / test_gpu_sgs.py)
# ---------------------------------------------------------------------------
def chebyshev_coefficients(degree, lmin, lmax):
    theta = 0.5 * (lmax + lmin)
    delta = 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    a, b = [0.0], [1.0 / theta]
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        a.append(rho_new * rho)
        b.append(2.0 * rho_new / delta)
        rho = rho_new
    return a, b


def chebyshev_apply(spmv, r, dinv, degree, lmin, lmax):
    """z = q(dinv*A) dinv r as host/cg.h states it"""
    ca, cb = chebyshev_coefficients(degree, lmin, lmax)
    sc = (lambda v: v) if dinv is None else (lambda v: dinv * v)
    d = f(cb[0]) * sc(r)
    z = d.copy()
    for j in range(1, degree):
        w = spmv(z)
        d = f(ca[j]) * d + f(cb[j]) * sc(r - w)
        z = z + d
    return z


def sgs_color(csr):
    """greedy colouring in natural row order over the pattern of B + B^T"""
    rp, ci, _ = csr
    n = len(rp) - 1
    rows = row_of(rp)
    off = ci != rows
    a = np.concatenate([rows[off], ci[off]])
    b = np.concatenate([ci[off], rows[off]])
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))])
    colors = np.full(n, -1, np.int64)
    for i in range(n):
        used = set(colors[b[ptr[i]:ptr[i + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        colors[i] = c
    return colors


class SgsRef:
    """z = M^-1 r of host/cg.h on one rank: forward over colours 0..C-1 with the
    entries of smaller colour, backward over C-2..0 with those of larger
    colour, each ascending by column, every product and sum rounded."""

    def __init__(self, csr):
        rp, ci, va = csr
        self.n = n = len(rp) - 1
        self.colors = col = sgs_color(csr)
        self.C = int(col.max()) + 1 if n else 0
        self.dinv = 1.0 / diag_of(csr)
        rows = row_of(rp)
        self.parts = {}
        for name, keep in (("before", col[ci] < col[rows]),
                           ("after", col[ci] > col[rows])):
            keep = keep & (ci != rows)
            r_, c_, v_ = rows[keep], ci[keep], va[keep]
            ptr = np.concatenate([[0], np.cumsum(np.bincount(r_, minlength=n))])
            self.parts[name] = (ptr, c_, v_)  # CSR order: ascending column

    def _sums(self, part, rows, z):
        ptr, c, v = self.parts[part]
        s = np.zeros(len(rows))
        width = int((ptr[rows + 1] - ptr[rows]).max()) if len(rows) else 0
        for e in range(width):
            has = ptr[rows] + e < ptr[rows + 1]
            at = ptr[rows[has]] + e
            s[has] = s[has] + v[at] * z[c[at]]
        return s

    def __call__(self, r):
        z = np.zeros(self.n)
        for c in range(self.C):
            rows = np.flatnonzero(self.colors == c)
            z[rows] = (r[rows] - self._sums("before", rows, z)) * self.dinv[rows]
        for c in range(self.C - 2, -1, -1):
            rows = np.flatnonzero(self.colors == c)
            z[rows] = z[rows] - self.dinv[rows] * self._sums("after", rows, z)
        return z
