"""spmv::lobpcg without a GPU: the numpy restatement of lobpcg_cases.py against
dense eigvalsh, the Rayleigh-Ritz restatement against eigh of the whitened
pencil, the argument rules, the symbols, the ABI number and NULL handles."""
import os
import re

import numpy as np
import pytest

import lobpcg_cases as lc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ["spmv_hip_lobpcg_ws_create", "spmv_hip_lobpcg_ws_destroy",
           "spmv_hip_lobpcg_ws_reset", "spmv_hip_lobpcg_ws_capacity",
           "spmv_hip_lobpcg_ws_array", "spmv_hip_lobpcg_ws_read_async",
           "spmv_hip_lobpcg_ws_set_state", "spmv_hip_lobpcg_gram_grid",
           "spmv_hip_lobpcg_gram_f64", "spmv_hip_lobpcg_gram_reduce",
           "spmv_hip_lobpcg_rr", "spmv_hip_lobpcg_update_f64",
           "spmv_hip_lobpcg_residual_f64", "spmv_hip_lobpcg_norms"]
HOST_NEW = ["spmvh_lobpcg_workspace_create", "spmvh_lobpcg_workspace_destroy",
            "spmvh_lobpcg_workspace_reserve_timing", "spmvh_lobpcg_check_rules",
            "spmvh_lobpcg"]


# ---- the restatement against dense eigvalsh ------------------------------------------
@pytest.mark.parametrize("key", sorted(lc.K_REF, key=str))
def test_restatement_against_dense_eigvalsh(key):
    """By the theorem for symmetric A every theta_c lies within
    ||A x_c - theta_c x_c|| / ||x_c|| of an eigenvalue (+ n eps ||A||_inf for
    eigvalsh's own error), and the nev values match the nev smallest (largest)
    one to one.  Recorded on these solutions: max |X^T X - I| 1.3e-15, max
    off-diagonal |X^T A X| 5.0e-15."""
    name, nev, kind, largest = key
    C = lc.case(name)
    r = C.ref(nev, kind, largest=largest)
    assert (r["k"], r["status"]) == (lc.K_REF[key], 0)
    assert r["k"] < lc.KMAX_DEFAULT
    X = r["X"]
    lc.theorem_check(C.csr, C.norm_a, C.eigvals(), r["theta"], X, largest, key)
    G = X.T @ lc.dense(C.csr) @ X
    orth = np.abs(X.T @ X - np.eye(nev)).max()
    off = np.abs(G - np.diag(np.diag(G))).max()
    print(key, "k", r["k"], "orth %.2e" % orth, "offdiag %.2e" % off)
    assert orth <= 1e-14 and off <= 1e-13 * C.norm_a
    # the history: -1.0 from the iteration after a column met its test
    for c in range(nev):
        h = r["hist"][c]
        last = int(np.nonzero(h >= 0.0)[0][-1])
        assert np.all(h[:last + 1] >= 0.0) and np.all(h[last + 1:] == -1.0)
        assert h[last] < 1e-6 * abs(r["theta"][c])
    # the true residuals are the recurrence's, up to the drift of the implicit AX
    assert np.all(r["true_resnorm"] < 2e-6 * np.abs(r["theta"]))


def test_kernel_references_compose_into_lobpcg_ref():
    """two iterations by hand from the kernel references equal lobpcg_ref"""
    C = lc.case("poisson11")
    k = 3
    X0 = lc.x0(C.N, k, 4)
    full = 7

    def mult(V):
        return np.stack([C.spmv(V[:, c]) for c in range(k)], axis=1)
    gg, rg = lc.gram_grid(C.N), lc.rows_grid(C.N)
    rr = lc.rr_ref(lc.gram_sum(lc.gram_partials(X0, X0, gg)), k, 1, full, 0, mode=1)
    X, _ = lc.combine([X0], rr["coef"], rr["basis"], full, k)
    AX = mult(X)
    rr = lc.rr_ref(lc.gram_sum(lc.gram_partials(X, AX, gg)), k, 1, full, 0)
    X, _ = lc.combine([X], rr["coef"], rr["basis"], full, k)
    AX, _ = lc.combine([AX], rr["coef"], rr["basis"], full, k)
    theta = rr["theta"]
    P = AP = np.zeros((C.N, k))
    hist = np.full((k, 3), -1.0)
    active, has_p = full, 0
    for it in range(3):
        R, W, r2 = lc.residual_ref(X, AX, theta)
        rn2 = lc.reduce_column(lc.rows_partials(r2, rg))
        active, done = lc.norms_ref(rn2, theta, active, it, 2, 1e-9, 0.0, hist)
        if done:
            break
        AW = mult(W)
        g = lc.gram_sum(lc.gram_partials(np.concatenate([X, W, P], axis=1),
                                         np.concatenate([AX, AW, AP], axis=1), gg))
        rr = lc.rr_ref(g, k, 3, active, has_p)
        theta = rr["theta"]
        X, P, AX, AP = (*lc.combine([X, W, P], rr["coef"], rr["basis"], active, k),
                        *lc.combine([AX, AW, AP], rr["coef"], rr["basis"], active, k))
        has_p = 1
    ref = lc.lobpcg_ref(C.spmv, None, X0, 2, 1e-9)
    assert ref["k"] == 2 and np.array_equal(ref["X"], X)
    assert np.array_equal(ref["theta"], theta) and np.array_equal(ref["hist"], hist)


def test_sgs_beats_jacobi_on_the_anisotropic_matrix():
    """strong coupling in y: after 40 iterations every column's residual behind
    SGS is less than half of the one behind Jacobi (recorded: 7 to 12 times
    smaller)"""
    import test_gpu_sgs as ts
    C = lc.case("aniso480")
    colours = host.sgs_color(C.csr[0], C.csr[1], C.N, C.N, False)[0]
    sw = ts.Sweeps(C.csr, C.N, colours, False)
    dinv = 1.0 / C.diag
    X0 = lc.x0(C.N, 4, 1)
    jac = lc.lobpcg_ref(C.spmv, None, X0, 40, 1e-12, dinv=dinv)
    sgs = lc.lobpcg_ref(C.spmv, lambda r: sw.apply(dinv, r), X0, 40, 1e-12)
    assert jac["k"] == sgs["k"] == 40
    print("jacobi", jac["hist"][:, 40], "sgs", sgs["hist"][:, 40])
    assert np.all(sgs["hist"][:, 40] < 0.5 * jac["hist"][:, 40])


def test_gram_restatement_is_a_gram_matrix():
    rng = np.random.default_rng(0)
    for M, m in ((1, 3), (65, 6), (300, 24), (1331, 9)):
        S, AS = rng.uniform(-1, 1, (M, m)), rng.uniform(-1, 1, (M, m))
        for grid in (1, lc.gram_grid(M), 3):
            g = lc.gram_sum(lc.gram_partials(S, AS, grid))
            assert np.allclose(g[0], np.triu(S.T @ S), rtol=0, atol=1e-12 * M)
            assert np.allclose(g[1], np.triu(S.T @ AS), rtol=0, atol=1e-12 * M)


@pytest.mark.parametrize("m,k", [(3, 1), (6, 2), (9, 3), (12, 4), (24, 8)])
def test_rr_restatement_against_eigh_of_the_whitened_pencil(m, k):
    """The Jacobi iteration stops after a sweep that rotated nothing: every
    off-diagonal g then satisfies |b_pp| + |g| == |b_pp|, |g| <= eps |b_pp|,
    so by Gershgorin the diagonal is within m eps ||B|| of the spectrum of the
    matrix it has become; each of the at most 30 m (m - 1) / 2 rotations adds
    a backward error of a few eps ||B||.  The whitening (Cholesky, two
    triangular solves) is common to both sides up to cond(Gb) eps ||B||."""
    rng = np.random.default_rng(m)
    Q = rng.uniform(-1, 1, (m + 3, m))
    Gb = Q.T @ Q
    Ga = rng.uniform(-1, 1, (m, m))
    Ga = Ga + Ga.T
    gram = np.stack([np.triu(Gb), np.triu(Ga)])
    for largest in (False, True):
        rr = lc.rr_ref(gram, k, 3, (1 << k) - 1, 1, largest)
        L = np.linalg.cholesky(Gb)
        Bw = np.linalg.solve(L, np.linalg.solve(L, Ga).T).T
        lam = np.linalg.eigvalsh((Bw + Bw.T) / 2)
        want = lam[::-1][:k] if largest else lam[:k]
        eps = np.finfo(np.float64).eps
        bar = 30 * m * m * eps * np.linalg.norm(Bw) * np.linalg.cond(Gb)
        assert rr["ok"] and not rr["restart"]
        assert np.abs(rr["theta"] - want).max() <= bar
        Cf = rr["coef"]
        assert np.abs(Cf.T @ Gb @ Cf - np.eye(k)).max() <= bar
        assert np.abs(Cf.T @ Ga @ Cf - np.diag(rr["theta"])).max() <= bar


def test_rr_restatement_breakdowns():
    eye = np.eye(6)
    ga = np.triu(np.random.default_rng(3).uniform(-1, 1, (6, 6)))
    gb = eye.copy()
    gb[4, 5] = 1.0
    rr = lc.rr_ref(np.stack([gb, ga]), 2, 3, 3, 1)
    assert rr["ok"] and rr["restart"] and rr["basis"] == 0b001111
    gb = eye.copy()
    gb[2, 3] = 1.0
    assert not lc.rr_ref(np.stack([gb, ga]), 2, 3, 3, 1)["ok"]
    assert lc.rr_ref(np.stack([gb, ga]), 2, 3, 1, 1)["basis"] == 0b010111
    g = np.stack([eye, ga])
    g[0, 0, 1] = np.nan
    assert not lc.rr_ref(g, 2, 3, 3, 1)["ok"]
    # a rank-deficient initial block: status 1 at k = 0.  With two equal
    # columns the last pivot is b - (b / sqrt(b))^2 - r12^2 in rounded
    # arithmetic; seed 6 is one for which it is not positive (the rule is
    # `piv > 0` and nothing else, so another seed may pass the factorisation
    # and fail later, or not at all)
    C = lc.case("poisson11")
    X0 = lc.x0(C.N, 3, 6)
    X0[:, 2] = X0[:, 0]
    r = lc.lobpcg_ref(C.spmv, None, X0, 5, 1e-6)
    assert (r["k"], r["status"]) == (0, 1) and np.array_equal(r["X"], X0)


# ---- argument rules ------------------------------------------------------------------
def test_argument_rules():
    host.lobpcg_check_rules(4, 10, 1e-8, 0.0)
    host.lobpcg_check_rules(8, 0, 0.0, 1e-9, has_sgs=True, sgs_rows=5, rows=5)
    bad = [(dict(nev=0), "nev"), (dict(nev=9), "nev"), (dict(kmax=-1), "kmax"),
           (dict(rtol=-1.0), "tol"), (dict(rtol=float("nan")), "tol"),
           (dict(rtol=float("inf")), "tol"), (dict(atol=-1.0), "tol"),
           (dict(atol=float("inf")), "tol"), (dict(rtol=0.0, atol=0.0), "tol"),
           (dict(has_dinv=True, has_amg=True), "preconditioner"),
           (dict(has_sgs=True, has_amg=True), "preconditioner"),
           (dict(has_sgs=True, sgs_rows=4, rows=5), "rows"),
           (dict(has_amg=True, amg_rows=6, rows=5), "rows"),
           (dict(has_sgs=True, sgs_rows=5, rows=5, sgs_negative_pivots=1),
            "pivot")]
    for kw, text in bad:
        args = dict(nev=2, kmax=5)
        args.update(kw)
        with pytest.raises(host.SpmvHostError, match=text):
            host.lobpcg_check_rules(**args)
    # the order: nev, kmax, tol, preconditioner, rows
    with pytest.raises(host.SpmvHostError, match="nev"):
        host.lobpcg_check_rules(0, -1, -1.0)
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.lobpcg_check_rules(1, -1, -1.0)
    with pytest.raises(host.SpmvHostError, match="tol"):
        host.lobpcg_check_rules(1, 1, -1.0, has_dinv=True, has_sgs=True)


# ---- the interface -----------------------------------------------------------------
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(\w+)\s*\(", txt))


def test_symbols_declared_exported_prototyped():
    hip_decl, host_decl = _declared("spmv_hip.h"), _declared("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
    assert callable(host.lobpcg) and callable(host.lobpcg_check_rules)
    assert issubclass(host.LobpcgWorkspace, object)


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)


def test_null_handles_rejected():
    h = _lib.hip
    for n in HIP_NEW:
        if n == "spmv_hip_lobpcg_ws_destroy":  # (destroying nothing is allowed)
            assert h.spmv_hip_lobpcg_ws_destroy(None) == 0
            continue
        fn = getattr(h, n)
        args = [0 if t in (_lib.C.c_int, _lib.C.c_int64, _lib.C.c_size_t)
                else 0.0 if t is _lib.C.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, n
    for n in ("spmvh_lobpcg_workspace_create",
              "spmvh_lobpcg_workspace_reserve_timing", "spmvh_lobpcg"):
        fn = getattr(host.lib, n)
        args = [0 if t is host.C.c_int else 0.0 if t is host.C.c_double else None
                for t in fn.argtypes]
        assert fn(*args) != 0, n
        assert b"NULL" in host.lib.spmvh_last_error(), n
