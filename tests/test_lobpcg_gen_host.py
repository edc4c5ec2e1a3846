"""spmv::lobpcg with B without a GPU: the numpy restatement of
lobpcg_gen_cases.py against lobpcg_cases.py (B = I: the same bits) and against
the dense pencil, the Gram restatement, the rule "pencil", the symbols and the
ABI number."""
import os
import re

import numpy as np
import pytest

import lobpcg_cases as lc
import lobpcg_gen_cases as lg
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ["spmv_hip_lobpcg_gram_gen_f64", "spmv_hip_lobpcg_update_gen_f64",
           "spmv_hip_lobpcg_residual_gen_f64"]
HOST_NEW = ["spmvh_lobpcg_gen", "spmvh_lobpcg_check_pencil"]


# ---- B = I: the bits of the solve without B ------------------------------------------
@pytest.mark.parametrize("nev,kind,largest", [(4, "none", False), (3, "dinv", False),
                                              (2, "none", True), (8, "none", False)])
def test_identity_b_has_the_bits_of_lobpcg_ref(nev, kind, largest):
    """0.0 + 1.0 * x is x, so BX, BW, BP have the bits of X, W, P, the Gram
    sums those of S^T S, and every later step follows"""
    C, P = lc.case("poisson11"), lg.pencil("identity11")
    X0 = lc.x0(C.N, nev, 1)
    a = C.ref(nev, kind, 14, 1e-2, largest=largest, X0=X0)
    b = P.ref(X0, 14, 1e-2, kind, largest=largest)
    assert (a["k"], a["status"], a["restarts"], a["active"]) == (
        b["k"], b["status"], b["restarts"], b["active"])
    for key in ("theta", "hist", "X", "P", "true_resnorm"):
        assert np.array_equal(a[key], b[key]), key


def test_gram_restatement():
    """BS = S: lobpcg_cases.gram_partials' bits; a random BS: a Gram matrix"""
    rng = np.random.default_rng(0)
    for M, m in ((1, 3), (65, 6), (300, 24), (1331, 9)):
        S, AS, BS = (rng.uniform(-1, 1, (M, m)) for _ in range(3))
        for grid in (1, lc.gram_grid(M), 3):
            assert np.array_equal(lg.gram_partials_gen(S, AS, S, grid),
                                  lc.gram_partials(S, AS, grid))
            g = lc.gram_sum(lg.gram_partials_gen(S, AS, BS, grid))
            assert np.allclose(g[0], np.triu(S.T @ BS), rtol=0, atol=1e-12 * M)
            assert np.allclose(g[1], np.triu(S.T @ AS), rtol=0, atol=1e-12 * M)


# ---- against the dense pencil ----------------------------------------------------------
@pytest.mark.parametrize("key", sorted(lg.K_GEN, key=str))
def test_restatement_against_the_dense_pencil(key):
    """Every column converges, and every theta_c lies within the bound of
    lobpcg_gen_cases.theorem_check_gen of a distinct eigenvalue of the dense
    pencil (eigh of L^-1 A L^-T): the nev values pair off with the nev smallest
    (largest) ones.

    X^T B X = I is asserted to
        (64 m cond(B) + n sqrt(cond(B))) eps,   m = 3 nev, n rows.
    Where it comes from: the last step leaves X = S C with C^T Gb C = I up to
    the error of the Cholesky factorisation and the two triangular solves of
    the m x m pencil (each backward stable: m eps per entry, a factor 64 for
    the three of them and the back substitution); the entries of Gb are sums
    over n rows of products s_i (Bs)_j, and for B-normalised columns
    ||s_i||_2 ||B s_j||_2 <= sqrt(lambda_max(B) / lambda_min(B)), so a Gram sum
    (and numpy's own X^T B X here) is off by at most n eps sqrt(cond(B));
    the implicit BX = BS C differs from B X by m roundings per step of that
    size, which is where cond(B) enters the first term.  Recorded on these
    solutions: at most 2.9e-15."""
    name, nev, kind, largest = key
    P = lg.pencil(name)
    r = P.ref(lc.x0(P.N, nev, 1), lg.KMAX_GEN, 1e-6, kind, largest=largest)
    assert (r["k"], r["status"], r["active"]) == (lg.K_GEN[key], 0, 0)
    assert r["k"] < lg.KMAX_GEN
    lg.theorem_check_gen(P, r["theta"], r["X"], largest, key)
    X, (Ad, Bd) = r["X"], P.dense()
    eps = np.finfo(np.float64).eps
    cond_b = P.eig()[3]
    orth = np.abs(X.T @ Bd @ X - np.eye(nev)).max()
    bound = (64 * 3 * nev * cond_b + P.N * np.sqrt(cond_b)) * eps
    print(key, "k", r["k"], "orth %.2e" % orth, "bound %.2e" % bound)
    assert orth <= bound
    for c in range(nev):
        h = r["hist"][c]
        last = int(np.nonzero(h >= 0.0)[0][-1])
        assert np.all(h[:last + 1] >= 0.0) and np.all(h[last + 1:] == -1.0)
        assert h[last] < 1e-6 * abs(r["theta"][c])
    # the true residuals are the recurrence's, up to the drift of AX and BX
    assert np.all(r["true_resnorm"] < 2e-6 * np.abs(r["theta"]))


def test_b_that_is_not_positive_definite():
    """one negative diagonal entry of B: x^T B x < 0 for the unit vector there.
    Whether the FIRST factorisation meets a pivot that is not positive depends
    on X0 (no other test of definiteness is made): column 0 of this X0 is
    that unit vector, so Gb[0, 0] < 0.  A NaN in B fails the first pivot too."""
    P = lg.pencil("lumped11")
    X0 = lc.x0(P.N, 3, 1)
    X0[:, 0] = 0.0
    X0[5, 0] = 1.0
    for bad in (-1.0, np.nan):
        rp, ci, va = P.B
        va = va.copy()
        va[5] = bad
        r = lg.lobpcg_gen_ref(
            P.spmv_a, lambda v: lg.oracle.csr_spmv(rp, ci, va, v), None, X0, 5, 1e-6)
        assert (r["k"], r["status"]) == (0, 1) and np.array_equal(r["X"], X0)


# ---- the rule "pencil" -------------------------------------------------------------
def test_pencil_rule():
    host.lobpcg_check_pencil(5, 5)
    host.lobpcg_check_pencil(5, 5, [7, 9, 12], [7, 9, 12])
    bad = [((5, 4), {}),                                  # another row count
           ((5, 5, [7, 9, 12], [7, 9]), {}),              # a missing ghost
           ((5, 5, [7, 9], [7, 9, 12]), {}),              # one too many
           ((5, 5, [7, 9, 12], [7, 12, 9]), {}),          # permuted ghosts
           ((5, 5, [7, 9, 12], [7, 9, 13]), {}),          # another ghost
           ((5, 5, [], [3]), {})]
    for args, kw in bad:
        with pytest.raises(host.SpmvHostError, match="pencil"):
            host.lobpcg_check_pencil(*args, **kw)


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
    assert callable(host.lobpcg_check_pencil)
    import inspect
    assert "B" in inspect.signature(host.lobpcg).parameters


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5


def test_null_handles_rejected():
    for n in HIP_NEW:
        fn = getattr(_lib.hip, n)
        args = [0 if t in (_lib.C.c_int, _lib.C.c_int64, _lib.C.c_size_t)
                else 0.0 if t is _lib.C.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, n
    fn = host.lib.spmvh_lobpcg_gen
    args = [0 if t is host.C.c_int else 0.0 if t is host.C.c_double else None
            for t in fn.argtypes]
    assert fn(*args) != 0
    assert b"NULL" in host.lib.spmvh_last_error()
    # a ghost list that is announced but absent
    assert host.lib.spmvh_lobpcg_check_pencil(1, 1, None, 2, None, 2) != 0
    assert b"NULL" in host.lib.spmvh_last_error()
