"""spmv::lobpcg restated in numpy: one reference per kernel of
hip/blas1_lobpcg.hip, and lobpcg_ref composed of them with oracle.csr_spmv and
the preconditioner references of the suite.  No GPU.

Every function here does the kernel's arithmetic in the kernel's order, one
rounding per operation, so the device results are compared bit for bit.

Summation order of ONE Gram entry (i, j) (gram_partials, gram_sum; the kernel
file states the same): the rows are walked in chunks of 64; workgroup b of g
takes the chunks b, b + g, b + 2g, ...  Inside a chunk row r (0..63) belongs
to row group r % G, G = 256 // (2 T), T the number of 4 x 4 tiles in the upper
triangle of the m x m matrix padded to a multiple of 4.  A row group adds its
products s_i(row) * as_j(row) one by one, rows ascending, chunks in the
workgroup's order, from 0.0; the workgroup adds its G row groups in order from
0.0; the workgroups are added in index order from 0.0.

||r_c||^2 (rows_partials, reduce_column): thread t of workgroup b adds its rows
b * 256 + t + j * 256 * grid one by one; the workgroup sums its threads with
the shuffle tree of common.h (offsets 32 ... 1 inside a wave, the four waves in
order); one workgroup adds the partials the same way.

Iteration counts of lobpcg_ref recorded here (K_REF) were computed with this
file on the CPU; test_lobpcg_host.py asserts them."""
import math

import numpy as np

import gmres_cases as gc
import minres_cases as mc
import oracle

GRAM_ROWS = 64
K_BLOCK = 256
SWEEPS = 30
GRAM_CAP = 512      # 2 workgroups per CU on 256 CUs
NEV = (1, 2, 3, 4, 8)
KMAX_DEFAULT = 200


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def seq_sum(a):
    """a[0] + a[1] + ... along axis 0, left to right from 0.0"""
    a = np.asarray(a, np.float64)
    z = np.zeros((1,) + a.shape[1:])
    return np.cumsum(np.concatenate([z, a], axis=0), axis=0)[-1]


def block_sum(v):
    """spmv_block_sum over axis 0 (256 values): -> the value thread 0 holds"""
    v = np.array(v, np.float64).reshape((4, 64) + v.shape[1:])
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
    r = np.zeros(v.shape[2:])
    for w in range(4):
        r = r + v[w, 0]
    return r


def rows_grid(M, dot_blocks=2048):
    return min(max(1, -(-M // K_BLOCK)), dot_blocks)


def rows_partials(vals, grid):
    """vals[M, k] -> partials[grid, k] of the one-thread-per-row kernels"""
    M, k = vals.shape
    T = grid * K_BLOCK
    trips = max(1, -(-M // T))
    pad = np.zeros((trips * T, k))
    pad[:M] = vals
    acc = seq_sum(pad.reshape(trips, T, k))          # per thread
    return np.stack([block_sum(acc[b * K_BLOCK:(b + 1) * K_BLOCK])
                     for b in range(grid)])


def reduce_column(partials):
    """partials[len, k] -> [k]: reduce_column of blas1_block.h"""
    n, k = partials.shape
    trips = max(1, -(-n // K_BLOCK))
    pad = np.zeros((trips * K_BLOCK, k))
    pad[:n] = partials
    return block_sum(seq_sum(pad.reshape(trips, K_BLOCK, k)))


# ---------------------------------------------------------------------------
# gram
# ---------------------------------------------------------------------------
def gram_grid(M, cap=GRAM_CAP):
    return min(max(1, -(-M // GRAM_ROWS)), cap)


def gram_groups(m):
    mt = (m + 3) // 4
    return K_BLOCK // (mt * (mt + 1))


def gram_partials(S, AS, grid):
    """S, AS: [M, m] (the blocks side by side) -> partials[grid, 2, m, m], the
    upper triangles, zero below"""
    M, m = S.shape
    G = gram_groups(m)
    nchunks = -(-M // GRAM_ROWS)
    out = np.zeros((grid, 2, m, m))
    upper = np.triu(np.ones((m, m), bool))
    for b in range(grid):
        total = np.zeros((2, m, m))
        for g in range(G):
            rows = [np.arange(c * GRAM_ROWS + g,
                              min(M, (c + 1) * GRAM_ROWS), G)
                    for c in range(b, nchunks, grid)]
            rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
            s, a = S[rows], AS[rows]
            acc = np.stack([seq_sum(s[:, :, None] * s[:, None, :]),
                            seq_sum(s[:, :, None] * a[:, None, :])])
            total = total + acc
        out[b] = np.where(upper, total, 0.0)
    return out


def gram_sum(partials):
    """-> [2, m, m]: the workgroups in index order"""
    return seq_sum(partials)


# ---------------------------------------------------------------------------
# rr
# ---------------------------------------------------------------------------
def _rr_attempt(raw, idx, mode, largest, k):
    """one pass of the kernel's retry loop -> None (failed) or
    (theta_sel, V[m, k], d[m])"""
    m = len(idx)
    gb_raw, ga_raw = raw
    d = np.zeros(m)
    with np.errstate(all="ignore"):
        for a in range(m):
            d[a] = 1.0 / np.sqrt(np.float64(gb_raw[idx[a], idx[a]]))
        B = np.zeros((m, m))
        A = np.zeros((m, m))
        for a in range(m):
            for b in range(m):
                lo, hi = min(a, b), max(a, b)
                B[a, b] = (gb_raw[idx[lo], idx[hi]] * d[lo]) * d[hi]
                A[a, b] = (ga_raw[idx[lo], idx[hi]] * d[lo]) * d[hi]
        rd = np.zeros(m)
        for j in range(m):
            piv = B[j, j]
            for p in range(j):
                piv = piv - B[p, j] * B[p, j]
            if not piv > 0.0:
                return None
            rd[j] = math.sqrt(piv)
            v = B[j, j + 1:].copy()
            for p in range(j):
                v = v - B[p, j] * B[p, j + 1:]
            B[j, j + 1:] = v / rd[j]
        Z = np.eye(m)
        if mode == 0:
            for i in range(m):          # Y = R^-T Ga, all columns at once
                v = A[i, :].copy()
                for p in range(i):
                    v = v - B[p, i] * A[p, :]
                A[i, :] = v / rd[i]
            for j in range(m):          # B = Y R^-1, all rows at once
                v = A[:, j].copy()
                for p in range(j):
                    v = v - A[:, p] * B[p, j]
                A[:, j] = v / rd[j]
            A = np.triu(A) + np.triu(A, 1).T
            for _ in range(SWEEPS):
                rotated = False
                for p in range(m - 1):
                    for q in range(p + 1, m):
                        apq, app, aqq = A[p, q], A[p, p], A[q, q]
                        if apq == 0.0:
                            continue
                        g = abs(apq)
                        if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                            A[p, q] = A[q, p] = 0.0
                            continue
                        rotated = True
                        tau = (aqq - app) / (2.0 * apq)
                        t = 1.0 / (abs(tau) + np.sqrt(1.0 + tau * tau))
                        if tau < 0.0:
                            t = -t
                        c = 1.0 / np.sqrt(1.0 + t * t)
                        s = t * c
                        brp, brq = A[:, p].copy(), A[:, q].copy()
                        np_, nq = c * brp - s * brq, s * brp + c * brq
                        A[:, p] = np_
                        A[p, :] = np_
                        A[:, q] = nq
                        A[q, :] = nq
                        A[p, p] = app - t * apq
                        A[q, q] = aqq + t * apq
                        A[p, q] = A[q, p] = 0.0
                        zp, zq = Z[:, p].copy(), Z[:, q].copy()
                        Z[:, p] = c * zp - s * zq
                        Z[:, q] = s * zp + c * zq
                if not rotated:
                    break
            th = np.diag(A).copy()
            if not np.all(th - th == 0.0):
                return None
            sel = [0] * k
            for a in range(m):
                rank = 0
                for b in range(m):
                    before = th[b] > th[a] if largest else th[b] < th[a]
                    if before or (th[b] == th[a] and b < a):
                        rank += 1
                if rank < k:
                    sel[rank] = a
            theta = th[sel]
        else:
            sel = list(range(k))
            theta = None
        V = np.zeros((m, k))
        for i in range(m - 1, -1, -1):
            v = Z[i, sel].copy()
            for p in range(i + 1, m):
                v = v - B[i, p] * V[p, :]
            V[i, :] = v / rd[i]
    return theta, V, d


def rr_ref(gram, k, nb, active, has_p, largest=False, mode=0):
    """gram: [2, mf, mf] (upper triangles) -> dict(ok, theta, coef[mf, k],
    basis, restart); ok False: the basis collapsed (status 1)"""
    mf = nb * k
    raw = np.asarray(gram, np.float64).reshape(2, mf, mf)
    for attempt in (0, 1):
        use_p = nb == 3 and has_p and attempt == 0
        if attempt == 1 and not (nb == 3 and has_p):
            break
        idx = list(range(k))
        if nb >= 2:
            idx += [k + c for c in range(k) if (active >> c) & 1]
        if use_p:
            idx += [2 * k + c for c in range(k) if (active >> c) & 1]
        got = _rr_attempt(raw, idx, mode, largest, k)
        if got is not None:
            theta, V, d = got
            coef = np.zeros((mf, k))
            for a, j in enumerate(idx):
                coef[j] = V[a] * d[a]
            basis = sum(1 << j for j in idx)
            return dict(ok=True, theta=theta, coef=coef, basis=basis,
                        restart=attempt == 1)
    return dict(ok=False)


# ---------------------------------------------------------------------------
# update, residual, norms
# ---------------------------------------------------------------------------
def combine(blocks, coef, basis, active, k):
    """blocks: list of nb [M, k] arrays -> (S C, [W, P] C_wp with the inactive
    columns of the last block kept)"""
    nb = len(blocks)
    M = blocks[0].shape[0]
    xo = np.zeros((M, k))
    po = np.zeros((M, k))
    for c in range(k):
        ax = np.zeros(M)
        ap = np.zeros(M)
        for b in range(nb):
            for j in range(k):
                if (basis >> (b * k + j)) & 1:
                    t = blocks[b][:, j] * coef[b * k + j, c]
                    ax = ax + t
                    if b > 0:
                        ap = ap + t
        xo[:, c] = ax
        po[:, c] = ap if (active >> c) & 1 else blocks[-1][:, c]
    return xo, po


def residual_ref(X, AX, theta, dinv=None):
    """-> (R, W, r * r)"""
    R = AX - X * theta[None, :]
    W = R if dinv is None else dinv[:, None] * R
    return R, W, R * R


def norms_ref(rn2, theta, active, it, kmax, rtol, atol, hist):
    """the decision of the norms kernel -> (active, done)"""
    for c in range(len(rn2)):
        if not (active >> c) & 1:
            continue
        r = math.sqrt(rn2[c]) if rn2[c] >= 0.0 else math.nan
        hist[c, it] = r
        a = rtol * abs(theta[c])
        tol = a if a > atol else atol
        if r < tol:
            active &= ~(1 << c)
    return active, active == 0 or it >= kmax


def lobpcg_ref(spmv, precond, X0, kmax, rtol, atol=0.0, largest=False,
               dinv=None, cap=GRAM_CAP, dot_blocks=2048):
    """spmv: column -> A column; precond: None (W = R, or W = dinv * R with
    dinv), or column -> M^-1 column.  -> dict(k, theta, hist[nev, kmax + 1],
    X, status, restarts, true_resnorm, P, active)"""
    X = np.array(X0, np.float64)
    M, k = X.shape
    gg, rg = gram_grid(M, cap), rows_grid(M, dot_blocks)
    hist = np.full((k, kmax + 1), -1.0)
    full = (1 << k) - 1
    out = dict(k=0, theta=np.zeros(k), hist=hist, X=X, status=0, restarts=0,
               P=np.zeros((M, k)), active=full)

    def mult(V):
        return np.stack([spmv(np.ascontiguousarray(V[:, c]))
                         for c in range(k)], axis=1)

    def true_res(Xn, theta):
        with np.errstate(all="ignore"):
            _, _, rr = residual_ref(Xn, mult(Xn), theta)
            return np.sqrt(reduce_column(rows_partials(rr, rg)))

    with np.errstate(all="ignore"):
        g = gram_sum(gram_partials(X, X, gg))
        rr = rr_ref(g, k, 1, full, 0, largest, mode=1)
        if not rr["ok"]:
            out.update(status=1, true_resnorm=true_res(X, out["theta"]))
            return out
        X, _ = combine([X], rr["coef"], rr["basis"], full, k)
        AX = mult(X)
        g = gram_sum(gram_partials(X, AX, gg))
        rr = rr_ref(g, k, 1, full, 0, largest)
        if not rr["ok"]:
            out.update(status=1, X=X, true_resnorm=true_res(X, out["theta"]))
            return out
        theta = rr["theta"]
        X, _ = combine([X], rr["coef"], rr["basis"], full, k)
        AX, _ = combine([AX], rr["coef"], rr["basis"], full, k)
        P, AP = np.zeros((M, k)), np.zeros((M, k))
        active, has_p, it, restarts, status = full, 0, 0, 0, 0
        while True:
            R, W, r2 = residual_ref(X, AX, theta, dinv)
            rn2 = reduce_column(rows_partials(r2, rg))
            active, done = norms_ref(rn2, theta, active, it, kmax, rtol, atol,
                                     hist)
            if done:
                break
            if precond is not None:
                W = np.stack([precond(np.ascontiguousarray(R[:, c]))
                              for c in range(k)], axis=1)
            AW = mult(W)
            S = np.concatenate([X, W, P], axis=1)
            AS = np.concatenate([AX, AW, AP], axis=1)
            g = gram_sum(gram_partials(S, AS, gg))
            rr = rr_ref(g, k, 3, active, has_p, largest)
            if not rr["ok"]:
                status = 1
                break
            restarts += int(rr["restart"])
            theta = rr["theta"]
            Xn, Pn = combine([X, W, P], rr["coef"], rr["basis"], active, k)
            AXn, APn = combine([AX, AW, AP], rr["coef"], rr["basis"], active, k)
            X, P, AX, AP = Xn, Pn, AXn, APn
            has_p = 1
            it += 1
    out.update(k=it, theta=theta, X=X, status=status, restarts=restarts, P=P,
               active=active, true_resnorm=true_res(X, theta))
    return out


# ---------------------------------------------------------------------------
# matrices and initial blocks
# ---------------------------------------------------------------------------
def diag_cluster(n=300):
    """diagonal, known spectrum: 1, 2, 2, 2 (a cluster of three), 3, 4, ..."""
    d = np.concatenate([[1.0, 2.0, 2.0, 2.0], np.arange(3.0, n - 1.0)])
    rp = np.arange(n + 1, dtype=np.int32)
    return rp, np.arange(n, dtype=np.int32), d[:n].copy()


def aniso2d(nx=24, ny=20, eps=0.05):
    """5-point -eps u_xx - u_yy with a diagonal that varies (so that Jacobi is
    not a scaled identity): strong coupling in y, where SGS helps and Jacobi
    does not"""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rows, cols, vals = [], [], []
    shift = 1.0 + 0.5 * ((np.arange(n) * 7) % 5)
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append((2.0 * eps + 2.0) * shift)
    for (a, b, v) in ((idx[:, :-1], idx[:, 1:], -eps),
                      (idx[:-1, :], idx[1:, :], -1.0)):
        for (r, c) in ((a, b), (b, a)):
            rows.append(r.ravel())
            cols.append(c.ravel())
            vals.append(np.full(r.size, v))
    return gc.to_csr(n, rows, cols, vals)


def csr_by_name(name):
    if name == "poisson11":
        return gc.poisson(11)
    if name == "shift11":
        return mc.shifted_poisson(11, 1.0)
    if name == "diag300":
        return diag_cluster()
    if name == "aniso480":
        return aniso2d()
    raise KeyError(name)


def dense(csr):
    rp, ci, va = csr
    n = len(rp) - 1
    D = np.zeros((n, n))
    D[gc.row_of(rp), ci] = va
    return D


def x0(n, nev, seed):
    return np.random.default_rng(1000 * seed + nev).uniform(-1.0, 1.0, (n, nev))


class Case:
    def __init__(self, name):
        self.name = name
        self.csr = csr_by_name(name)
        self.N = len(self.csr[0]) - 1
        self.diag = gc.diag_of(self.csr)
        self.norm_a = float(np.abs(dense(self.csr)).sum(axis=1).max())
        self._eig = None
        self._refs = {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, np.ascontiguousarray(v))

    def eigvals(self):
        if self._eig is None:
            self._eig = np.linalg.eigvalsh(dense(self.csr))
        return self._eig

    def dinv(self):
        return 1.0 / np.abs(self.diag)

    def ref(self, nev, kind="none", kmax=KMAX_DEFAULT, rtol=1e-6, atol=0.0,
            largest=False, seed=1, X0=None, precond=None):
        key = (nev, kind, kmax, rtol, atol, largest, seed)
        if X0 is not None or key not in self._refs:
            r = lobpcg_ref(self.spmv, precond,
                           x0(self.N, nev, seed) if X0 is None else X0, kmax,
                           rtol, atol, largest,
                           self.dinv() if kind == "dinv" else None)
            if X0 is not None:
                return r
            self._refs[key] = r
        return self._refs[key]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def theorem_check(csr, norm_a, eig, theta, X, largest, what):
    """Every theta_c lies within ||A x_c - theta_c x_c|| / ||x_c|| of an
    eigenvalue (symmetric A), plus n eps ||A||_inf for eigvalsh's own error;
    the nev values match the nev smallest (largest) one to one."""
    n, nev = X.shape
    eps = np.finfo(np.float64).eps
    want = eig[::-1][:nev] if largest else eig[:nev]
    for c in range(nev):
        x = np.ascontiguousarray(X[:, c])
        r = oracle.csr_spmv(*csr, x) - theta[c] * x
        bound = np.linalg.norm(r) / np.linalg.norm(x) + n * eps * norm_a
        assert np.abs(eig - theta[c]).min() <= bound, (what, c, theta[c], bound)
        assert abs(want[c] - theta[c]) <= bound, (what, c, theta[c], want[c],
                                                  bound)


# (matrix, nev, kind, largest) -> iterations of lobpcg_ref at KMAX_DEFAULT
# (200), rtol 1e-6, seed 1
K_REF = {("poisson11", 4, "none", False): 82,
         ("poisson11", 4, "dinv", False): 82,
         ("poisson11", 8, "none", False): 80,
         ("poisson11", 2, "none", True): 61,
         ("shift11", 3, "none", False): 67,
         ("shift11", 3, "none", True): 81,
         ("diag300", 5, "none", False): 150}
# measured on those solutions: max |X^T X - I| <= 1.3e-15,
# max off-diagonal |X^T A X| <= 5.0e-15
