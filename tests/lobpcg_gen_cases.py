"""spmv::lobpcg with B (the pencil A x = lambda B x) restated in numpy, on top
of lobpcg_cases.py: the Gram pass over nine blocks, the update of the three
triples, the residual with BX, and lobpcg_gen_ref composed of them with
oracle.csr_spmv.  No GPU.

What differs from the solve without B, and nothing else:
  gram_partials_gen  Gb entry (i, j), i <= j, is the sum over the rows of
                     s_i * (Bs)_j (not s_i * s_j), in the summation order
                     lobpcg_cases states; Ga is as there.  BS = S gives
                     lobpcg_cases.gram_partials' bits.
  update             lobpcg_cases.combine on a third triple [BX, BW, BP].
  residual_gen       R = AX - BX diag(theta): lobpcg_cases.residual_ref with BX
                     in X's place.
The Rayleigh-Ritz step, the norms, the masks and the restart rules are
lobpcg_cases' own functions.  With B the identity every BX, BW, BP has the
bits of X, W, P, so lobpcg_gen_ref returns the bits of lobpcg_ref
(test_lobpcg_gen_host.py asserts it).

The pencils of the tests and the recorded iteration counts (K_GEN, computed
with this file on the CPU) are at the end."""
import numpy as np

import gmres_cases as gc
import lobpcg_cases as lc
import oracle


def gram_partials_gen(S, AS, BS, grid):
    """S, AS, BS: [M, m] -> partials[grid, 2, m, m]: Gb = S^T BS, Ga = S^T AS,
    the upper triangles, zero below"""
    M, m = S.shape
    G = lc.gram_groups(m)
    nchunks = -(-M // lc.GRAM_ROWS)
    out = np.zeros((grid, 2, m, m))
    upper = np.triu(np.ones((m, m), bool))
    for b in range(grid):
        total = np.zeros((2, m, m))
        for g in range(G):
            rows = [np.arange(c * lc.GRAM_ROWS + g,
                              min(M, (c + 1) * lc.GRAM_ROWS), G)
                    for c in range(b, nchunks, grid)]
            rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
            s, a, bs = S[rows], AS[rows], BS[rows]
            acc = np.stack([lc.seq_sum(s[:, :, None] * bs[:, None, :]),
                            lc.seq_sum(s[:, :, None] * a[:, None, :])])
            total = total + acc
        out[b] = np.where(upper, total, 0.0)
    return out


def update_gen(triples, coef, basis, active, k):
    """triples: [[X, W, P], [AX, AW, AP], [BX, BW, BP]] (or one block each) ->
    [(X', P'), (AX', AP'), (BX', BP')]: combine on each triple"""
    return [lc.combine(t, coef, basis, active, k) for t in triples]


def residual_gen(AX, BX, theta, dinv=None):
    """-> (R, W, r * r) with R = AX - BX diag(theta)"""
    return lc.residual_ref(BX, AX, theta, dinv)


def lobpcg_gen_ref(spmv_a, spmv_b, precond, X0, kmax, rtol, atol=0.0,
                   largest=False, dinv=None, cap=lc.GRAM_CAP, dot_blocks=2048):
    """lobpcg_cases.lobpcg_ref for the pencil (spmv_a, spmv_b): column -> A
    column, column -> B column.  -> the same dict; X is B-orthonormal and
    true_resnorm is ||A x_c - theta_c B x_c|| from explicit products."""
    X = np.array(X0, np.float64)
    M, k = X.shape
    gg, rg = lc.gram_grid(M, cap), lc.rows_grid(M, dot_blocks)
    hist = np.full((k, kmax + 1), -1.0)
    full = (1 << k) - 1
    out = dict(k=0, theta=np.zeros(k), hist=hist, X=X, status=0, restarts=0,
               P=np.zeros((M, k)), active=full)

    def mult(spmv, V):
        return np.stack([spmv(np.ascontiguousarray(V[:, c]))
                         for c in range(k)], axis=1)

    def true_res(Xn, theta):
        with np.errstate(all="ignore"):
            _, _, rr = residual_gen(mult(spmv_a, Xn), mult(spmv_b, Xn), theta)
            return np.sqrt(lc.reduce_column(lc.rows_partials(rr, rg)))

    with np.errstate(all="ignore"):
        BX = mult(spmv_b, X)
        # (mode 1 reads Gb alone; the device passes BX for AS as well)
        g = lc.gram_sum(gram_partials_gen(X, BX, BX, gg))
        rr = lc.rr_ref(g, k, 1, full, 0, largest, mode=1)
        if not rr["ok"]:
            out.update(status=1, true_resnorm=true_res(X, out["theta"]))
            return out
        (X, _), (BX, _) = update_gen([[X], [BX]], rr["coef"], rr["basis"],
                                     full, k)
        AX = mult(spmv_a, X)
        g = lc.gram_sum(gram_partials_gen(X, AX, BX, gg))
        rr = lc.rr_ref(g, k, 1, full, 0, largest)
        if not rr["ok"]:
            out.update(status=1, X=X, true_resnorm=true_res(X, out["theta"]))
            return out
        theta = rr["theta"]
        (X, _), (AX, _), (BX, _) = update_gen([[X], [AX], [BX]], rr["coef"],
                                              rr["basis"], full, k)
        P, AP, BP = (np.zeros((M, k)) for _ in range(3))
        active, has_p, it, restarts, status = full, 0, 0, 0, 0
        while True:
            R, W, r2 = residual_gen(AX, BX, theta, dinv)
            rn2 = lc.reduce_column(lc.rows_partials(r2, rg))
            active, done = lc.norms_ref(rn2, theta, active, it, kmax, rtol,
                                        atol, hist)
            if done:
                break
            if precond is not None:
                W = np.stack([precond(np.ascontiguousarray(R[:, c]))
                              for c in range(k)], axis=1)
            AW, BW = mult(spmv_a, W), mult(spmv_b, W)
            g = lc.gram_sum(gram_partials_gen(
                np.concatenate([X, W, P], axis=1),
                np.concatenate([AX, AW, AP], axis=1),
                np.concatenate([BX, BW, BP], axis=1), gg))
            rr = lc.rr_ref(g, k, 3, active, has_p, largest)
            if not rr["ok"]:
                status = 1
                break
            restarts += int(rr["restart"])
            theta = rr["theta"]
            (X, P), (AX, AP), (BX, BP) = update_gen(
                [[X, W, P], [AX, AW, AP], [BX, BW, BP]], rr["coef"],
                rr["basis"], active, k)
            has_p = 1
            it += 1
    out.update(k=it, theta=theta, X=X, status=status, restarts=restarts, P=P,
               active=active, true_resnorm=true_res(X, theta))
    return out


# ---------------------------------------------------------------------------
# pencils
# ---------------------------------------------------------------------------
def tri(n, d, o):
    """tridiagonal, d on the diagonal and o beside it"""
    i = np.arange(n)
    return gc.to_csr(n, [i, i[:-1], i[1:]], [i, i[1:], i[:-1]],
                     [np.full(n, float(d)), np.full(n - 1, float(o)),
                      np.full(n - 1, float(o))])


def identity(n):
    i = np.arange(n, dtype=np.int32)
    return np.arange(n + 1, dtype=np.int32), i, np.ones(n)


def lumped(n):
    """a varying positive diagonal (a lumped mass matrix): 1, 1.5, 2, 2.5, 3"""
    rp, ci, _ = identity(n)
    return rp, ci, 1.0 + 0.5 * ((np.arange(n) * 7) % 5)


def mass_like(csr):
    """I + 0.1 (the pattern of A, entries 1): 1.1 on the diagonal, 0.1 beside
    it; strictly diagonally dominant where a row has fewer than 11 neighbours"""
    rp, ci, _ = csr
    va = np.where(ci == gc.row_of(rp), 1.1, 0.1)
    return rp, ci, va


def pencil_by_name(name):
    """-> (csr of A, csr of B)"""
    if name == "tri200":     # 1-D stiffness and consistent mass (h = 1)
        rp, ci, va = tri(200, 4, 1)
        return tri(200, 2, -1), (rp, ci, va * (1.0 / 6.0))
    if name == "lumped11":
        A = gc.poisson(11)
        return A, lumped(11 ** 3)
    if name == "mass11":
        A = gc.poisson(11)
        return A, mass_like(A)
    if name == "tri40":
        rp, ci, va = tri(40, 4, 1)
        return tri(40, 2, -1), (rp, ci, va * (1.0 / 6.0))
    if name == "mass8":
        A = gc.poisson(8)
        return A, mass_like(A)
    if name == "identity11":
        return gc.poisson(11), identity(11 ** 3)
    raise KeyError(name)


class Pencil:
    def __init__(self, name):
        self.name = name
        self.A, self.B = pencil_by_name(name)
        self.N = len(self.A[0]) - 1
        self.diag = gc.diag_of(self.A)
        self._dense = self._eig = None

    def spmv_a(self, v):
        return oracle.csr_spmv(*self.A, np.ascontiguousarray(v))

    def spmv_b(self, v):
        return oracle.csr_spmv(*self.B, np.ascontiguousarray(v))

    def dinv(self):
        return 1.0 / np.abs(self.diag)

    def dense(self):
        if self._dense is None:
            self._dense = lc.dense(self.A), lc.dense(self.B)
        return self._dense

    def eig(self):
        """eigenvalues of the pencil (ascending) from eigh of L^-1 A L^-T, and
        lambda_min(B), ||L^-1 A L^-T||_2"""
        if self._eig is None:
            Ad, Bd = self.dense()
            L = np.linalg.cholesky(Bd)
            Wt = np.linalg.solve(L, np.linalg.solve(L, Ad).T).T
            lam = np.linalg.eigvalsh((Wt + Wt.T) / 2)
            self._eig = (lam, float(np.linalg.eigvalsh(Bd)[0]),
                         float(np.abs(lam).max()), float(np.linalg.cond(Bd)))
        return self._eig

    def ref(self, X0, kmax, rtol, kind="none", atol=0.0, largest=False,
            precond=None):
        return lobpcg_gen_ref(self.spmv_a, self.spmv_b, precond, X0, kmax, rtol,
                              atol, largest,
                              self.dinv() if kind == "dinv" else None)


_PENCILS = {}


def pencil(name):
    if name not in _PENCILS:
        _PENCILS[name] = Pencil(name)
    return _PENCILS[name]


def theorem_check_gen(P, theta, X, largest, what, match=True):
    """For symmetric A, SPD B = L L^T and any x, theta there is an eigenvalue
    lambda of the pencil with
        |lambda - theta| <= ||A x - theta B x||_2 / (sqrt(lambda_min(B)) ||x||_B):
    y = L^T x is a vector of the symmetric L^-1 A L^-T with residual L^-1 r,
    ||L^-1 r|| <= ||r|| / sqrt(lambda_min(B)) and ||y|| = ||x||_B.  Added:
    n eps cond(B) ||L^-1 A L^-T||_2 for the error of the dense eigenvalues
    themselves (the whitening solves with L twice).  The residual comes from
    oracle.csr_spmv.  match: the nev values also pair off with the nev
    smallest (largest) eigenvalues one to one."""
    lam, lmin_b, norm_w, cond_b = P.eig()
    n, nev = X.shape
    eps = np.finfo(np.float64).eps
    want = lam[::-1][:nev] if largest else lam[:nev]
    for c in range(nev):
        x = np.ascontiguousarray(X[:, c])
        bx = P.spmv_b(x)
        r = P.spmv_a(x) - theta[c] * bx
        bound = (np.linalg.norm(r) / (np.sqrt(lmin_b) * np.sqrt(x @ bx))
                 + n * eps * cond_b * norm_w)
        assert np.abs(lam - theta[c]).min() <= bound, (what, c, theta[c], bound)
        if match:
            assert abs(want[c] - theta[c]) <= bound, (what, c, theta[c],
                                                      want[c], bound)


# (pencil, nev, kind, largest) -> iterations of lobpcg_gen_ref at kmax 300,
# rtol 1e-6, X0 = lobpcg_cases.x0(N, nev, 1); every column met its test.
# (tri200 is not here: the 1-D stiffness matrix of 200 rows, condition 1.6e4,
# does not meet 1e-6 within 300 iterations behind none or dinv; it is a case of
# the bit comparisons at a small kmax.)  mass8 with X0 = x0(512, 3, 9), dinv:
# 58 iterations (the two-rank test's pencil).
KMAX_GEN = 300
K_GEN = {("tri40", 3, "none", False): 62,
         ("tri40", 2, "none", True): 63,
         ("lumped11", 4, "none", False): 98,
         ("lumped11", 4, "dinv", False): 98,
         ("mass11", 4, "none", False): 83,
         ("mass11", 4, "dinv", False): 83,
         ("mass11", 3, "none", True): 85}
