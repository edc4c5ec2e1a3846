"""CPU checks of the aggregation multigrid preconditioner
(spmv::AmgPreconditioner): the new symbols are declared in both headers,
exported and prototyped, the change is additive (ABI 5), NULL handles are
refused before anything touches a device, every option rule is refused by its
name, the host builder (host/amg_build.h) equals the numpy restatement of
amg_cases.py exactly, and the restatement itself has the defining properties:
P has one 1 per row, A_1 = P^T A P, M^-1 is symmetric and positive definite.
tools/amg_build_check.cpp is built with the sanitizers and run."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amg_cases as ac
import gmres_cases as gc
import ilu0_cases as ic
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53

HIP_NEW = ("spmv_hip_amg_plan_create", "spmv_hip_amg_plan_destroy",
           "spmv_hip_amg_plan_bytes", "spmv_hip_amg_galerkin_f64",
           "spmv_hip_amg_diag_f64", "spmv_hip_amg_restrict_f64",
           "spmv_hip_amg_prolong_f64", "spmv_hip_amg_post0_f64")
HOST_NEW = ("spmvh_amg_check_options", "spmvh_amg_symbolic_create",
            "spmvh_amg_symbolic_get", "spmvh_amg_symbolic_destroy",
            "spmvh_amg_create", "spmvh_amg_destroy", "spmvh_amg_refresh",
            "spmvh_amg_info", "spmvh_amg_level_info", "spmvh_amg_aggregates",
            "spmvh_amg_level_matrix", "spmvh_amg_apply", "spmvh_pcg_amg",
            "spmvh_gmres_amg")
EINVAL = -1


def ragged_spd(n=3001, seed=7):
    """test_gpu_sgs.ragged_spd (that module needs a GPU stack to import)"""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        if i == 7:
            continue
        js = rng.integers(0, n, rng.integers(0, 21))
        a += [i] * len(js)
        b += js.tolist()
    for i in range(n - 24, n):
        a += [i] * (n - 1 - i)
        b += list(range(i + 1, n))
    for hub in (100, n - 501):
        js = rng.choice(n, 500, replace=False)
        a += [hub] * len(js)
        b += js.tolist()
    a, b = np.array(a), np.array(b)
    ok = (a != b) & (a != 7) & (b != 7)
    lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
    pairs = np.unique(lo * n + hi)
    lo, hi = pairs // n, pairs % n
    v = -rng.uniform(0.1, 1.0, len(pairs))
    rows = np.concatenate([lo, hi, np.arange(n)])
    cols = np.concatenate([hi, lo, np.arange(n)])
    off = np.bincount(np.concatenate([lo, hi]),
                      weights=np.abs(np.concatenate([v, v])), minlength=n)
    vals = np.concatenate([v, v, off + 1.0 + rng.uniform(0, 1, n)])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32), vals[order])


def _diagonal_matrix(n):
    i = np.arange(n)
    return (np.arange(n + 1).astype(np.int32), i.astype(np.int32),
            2.0 + np.sin(i) ** 2)


def _csr(name):
    if name == "arrow130":
        return ic.arrow(130)
    if name == "ragged3001":
        return ragged_spd()
    if name.startswith("diag"):
        return _diagonal_matrix(int(name[4:]))
    return gc.csr_by_name(name)


NAMES = ("poisson5", "poisson11", "banded257", "convdiff4", "arrow130",
         "ragged3001", "diag40", "diag1")
SYMMETRIC_NAMES = ("poisson5", "poisson11", "ragged3001", "diag40", "diag1")


# ---- 1. the interface -------------------------------------------------------------
def _declared_arity(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_amg_symbols_declared_exported_prototyped():
    hip_decl = _declared_arity("spmv_hip.h")
    host_decl = _declared_arity("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert len(getattr(_lib.hip, n).argtypes) == hip_decl[n], n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert len(getattr(host.lib, n).argtypes) == host_decl[n], n


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5


def test_python_layer_has_the_entry_points():
    for name in ("refresh", "levels", "rows", "non_zeros", "lmax", "aggregates",
                 "level_matrix", "plan_bytes", "setup_ms"):
        assert callable(getattr(host.AmgPreconditioner, name)), name
    assert callable(host.amg_apply) and callable(host.pcg_amg)
    assert callable(host.amg_symbolic) and callable(host.amg_check_options)
    assert host.AmgPcgWorkspace is host.SgsWorkspace


def test_null_handles_refused_without_a_device():
    hip = _lib.hip
    out, n64 = C.c_void_p(), C.c_int64()
    assert hip.spmv_hip_amg_plan_create(None, None, C.byref(out)) == EINVAL
    assert hip.spmv_hip_amg_plan_destroy(None) == 0
    assert hip.spmv_hip_amg_plan_bytes(None, C.byref(n64)) == EINVAL
    assert hip.spmv_hip_amg_galerkin_f64(None, None, None, None, None,
                                         None) == EINVAL
    assert hip.spmv_hip_amg_diag_f64(None, None, 0, 0, None, None, None, None,
                                     None, None, None, None) == EINVAL
    assert hip.spmv_hip_amg_restrict_f64(None, None, None, None, None,
                                         None) == EINVAL
    assert hip.spmv_hip_amg_prolong_f64(None, None, 1.0, None, None,
                                        None) == EINVAL
    assert hip.spmv_hip_amg_post0_f64(None, 0, 1.0, None, None, None, None, None,
                                      None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    out = C.c_void_p()
    info = np.zeros(4, np.int64)
    lmax = C.c_double()
    k = C.c_int()
    assert lib.spmvh_amg_create(None, None, None, C.byref(out)) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_amg_refresh(None, None) != 0
    assert lib.spmvh_amg_info(None, info.ctypes.data_as(C.c_void_p)) != 0
    assert lib.spmvh_amg_level_info(None, 0, info.ctypes.data_as(C.c_void_p),
                                    C.byref(lmax)) != 0
    assert lib.spmvh_amg_aggregates(None, 0, None) != 0
    assert lib.spmvh_amg_level_matrix(None, 1, None, None, None) != 0
    assert lib.spmvh_amg_apply(None, None, None, None) != 0
    assert lib.spmvh_pcg_amg(None, None, None, None, None, None, 1, 0.0,
                             C.byref(k), None, None, 0, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_gmres_amg(None, None, None, None, None, None, 0, 0.0, 0.0,
                               None, 30, 1, 0.0, C.byref(k), None, None, None, 0,
                               None, None, None) != 0
    assert lib.spmvh_amg_symbolic_destroy(None) == 0
    assert lib.spmvh_amg_destroy(None) == 0


BAD_OPTIONS = [("theta", -0.1), ("theta", 1.5), ("theta", float("nan")),
               ("max_levels", 0), ("max_levels", 17), ("min_coarse_rows", 0),
               ("smooth_degree", 0), ("smooth_degree", 17),
               ("coarse_degree", 0), ("coarse_degree", 17), ("eig_ratio", 1.0),
               ("eig_ratio", float("inf")), ("coarse_scale", 0.99),
               ("coarse_scale", 2.0)]


@pytest.mark.parametrize("field,value", BAD_OPTIONS)
def test_every_option_rule_is_refused_by_its_name(field, value):
    with pytest.raises(host.SpmvHostError, match=field):
        host.amg_check_options(**{field: value})


def test_the_limits_of_the_options_are_accepted():
    host.amg_check_options()
    host.amg_check_options(theta=0.0, max_levels=1, min_coarse_rows=1,
                           smooth_degree=1, coarse_degree=16, eig_ratio=1.5,
                           coarse_scale=1.0)
    host.amg_check_options(theta=1.0, max_levels=16, smooth_degree=16,
                           coarse_degree=1, coarse_scale=1.999)


# ---- 2. the host builder against the restatement ------------------------------------
KEYS = ("agg", "member_ptr", "member", "rowptr", "colind", "src_ptr", "src")


def _check_symbolic(csr, n, what, symmetric=False, diagonal=None, theta=0.25):
    got = host.amg_symbolic(*csr, n, n, symmetric, diagonal, theta)
    ptr, col, src = ac.expand(csr[0], csr[1], n, symmetric)
    assert np.array_equal(got["xrow_ptr"], ptr), what
    assert np.array_equal(got["xrow_col"], col), what
    assert np.array_equal(got["xrow_src"], src), what
    val = ac.values_of(src, csr[2], diagonal)
    want = ac.coarsen(ptr, col, src, val, n, theta)
    assert got["n_agg"] == want["n_agg"], what
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (what, key)
    return got


@pytest.mark.parametrize("theta", [0.25, 0.0, 1.0])
@pytest.mark.parametrize("name", NAMES)
def test_symbolic_builder_equals_the_restatement(name, theta):
    csr = _csr(name)
    n = len(csr[0]) - 1
    got = _check_symbolic(csr, n, (name, theta), theta=theta)
    print(name, theta, "rows", n, "aggregates", got["n_agg"], "coarse entries",
          len(got["colind"]), "longest list", np.diff(got["src_ptr"]).max(initial=0))
    if name.startswith("diag"):
        assert got["n_agg"] == n  # nothing merges
    if name == "arrow130":
        assert got["n_agg"] == 1
    if name.startswith("poisson"):
        assert got["n_agg"] < n // 4


@pytest.mark.parametrize("name", SYMMETRIC_NAMES)
def test_both_storages_give_identical_aggregates_and_patterns(name):
    csr = _csr(name)
    n = len(csr[0]) - 1
    general = _check_symbolic(csr, n, name)
    lower, diag = ac.lower_split(csr)
    sym = _check_symbolic(lower, n, (name, "symmetric"), True, diag)
    for key in ("agg", "member_ptr", "member", "rowptr", "colind", "src_ptr"):
        assert np.array_equal(sym[key], general[key]), (name, key)


def test_ghost_columns_are_ignored():
    csr = gc.poisson(4)
    n = 40  # the first 40 rows; columns >= 40 are ghosts
    rp = csr[0][:n + 1]
    local = (rp, csr[1][:rp[-1]], csr[2][:rp[-1]])
    got = _check_symbolic(local, n, "ghosts")
    assert len(got["xrow_col"]) < rp[-1] and got["xrow_col"].max() < n


def test_an_explicit_zero_and_a_duplicate_column():
    rp = np.array([0, 4, 6, 9], np.int32)
    ci = np.array([0, 1, 2, 2, 0, 1, 0, 2, 0], np.int32)
    va = np.array([4.0, 0.0, -1.0, -0.5, 0.0, 4.0, -1.0, 4.0, -0.5])
    for theta in (0.0, 0.25, 1.0):
        got = _check_symbolic((rp, ci, va), 3, ("odd", theta), theta=theta)
        # the zero entry is no neighbour, yet it stays in the coarse pattern
        assert got["n_agg"] == 2 and got["agg"][0] == got["agg"][2] != got["agg"][1]
        assert len(got["colind"]) == 4


def test_rows_and_owned_columns_must_be_the_same_range():
    csr = gc.poisson(3)
    for ncols in (26, 28):
        with pytest.raises(host.SpmvHostError, match="same index range"):
            host.amg_symbolic(*csr, 27, ncols)
    with pytest.raises(host.SpmvHostError, match="theta"):
        host.amg_symbolic(*csr, 27, theta=1.5)


# ---- 3. the restatement has the defining properties -------------------------------------
@pytest.mark.parametrize("name", ["poisson5", "banded257"])
def test_the_restatement_is_a_galerkin_hierarchy(name):
    """A_1 = P^T A P to 8 ulps of the entry's absolute contribution sum (every
    entry is a sum of terms of that size, as in test_ilu0_host's product
    test)."""
    csr = _csr(name)
    n = len(csr[0]) - 1
    ref = ac.AmgRef(csr, n, min_coarse_rows=20)
    assert len(ref.levels) >= 2
    A = ac.dense(csr, n)
    P = ref.dense_p(0)
    assert np.all(P.sum(axis=1) == 1.0) and np.all((P == 0) | (P == 1))
    c = ref.levels[1]["csr"]
    nc = ref.levels[1]["n"]
    got = ac.dense(c, nc)
    want, scale = P.T @ A @ P, P.T @ np.abs(A) @ P
    pattern = np.zeros((nc, nc), bool)
    pattern[gc.row_of(c[0]), c[1]] = True
    assert np.array_equal(pattern, scale != 0)  # zero sums stay in the pattern
    err = np.abs(got - want)[pattern] / scale[pattern]
    print(name, "levels", [L["n"] for L in ref.levels],
          "max error of A_1 / contribution sum", err.max())
    assert np.all(err <= 8 * U), (name, err.max())


@pytest.mark.parametrize("coarse_scale", [1.0, 1.6])
@pytest.mark.parametrize("name", ["poisson5", "banded257"])
def test_the_restated_cycle_is_symmetric_positive_definite(name, coarse_scale):
    """banded257 is not symmetric: its symmetric part stands in.  M^-1 e_j for
    every j; the asymmetry is held to 64 ulps of the largest entry (a cycle is
    a few dozen operations deep), the eigenvalues must be > 0."""
    rp, ci, va = _csr(name)
    n = len(rp) - 1
    A = ac.dense((rp, ci, va), n)
    A = 0.5 * (A + A.T)
    rows, cols = np.nonzero(A)
    csr = gc.to_csr(n, [rows], [cols], [A[rows, cols]])
    ref = ac.AmgRef(csr, n, min_coarse_rows=20, coarse_scale=coarse_scale)
    assert len(ref.levels) >= 2
    Minv = np.column_stack([ref.apply(e) for e in np.eye(n)])
    asym = np.abs(Minv - Minv.T).max() / np.abs(Minv).max()
    eig = np.linalg.eigvalsh(0.5 * (Minv + Minv.T))
    print(name, coarse_scale, "asymmetry / max entry", asym, "eigenvalues",
          eig.min(), eig.max())
    assert asym <= 64 * U, (name, asym)
    assert eig.min() > 0, (name, eig.min())


def test_amg_beats_one_level_methods_on_the_restatement():
    """k_amg < k_sgs on Poisson 24^3 to 1e-10 with the defaults, restatement
    against restatement (the inequality alone)."""
    csr = gc.poisson(24)
    n = 24 ** 3
    b = ac.spmv_ltr(csr, np.random.default_rng(n).uniform(-1, 1, n))
    amg = ac.AmgRef(csr, n)
    sgs = gc.SgsRef(csr)

    def pcg(precond):
        x, r = np.zeros(n), b.copy()
        z = precond(r)
        p, rz, rr0 = z.copy(), r @ z, b @ b
        for k in range(1, 400):
            Ap = ac.spmv_ltr(csr, p)
            alpha = rz / (p @ Ap)
            r = r - alpha * Ap
            x = x + alpha * p
            if np.sqrt(r @ r) / np.sqrt(rr0) < 1e-10:
                return k
            z = precond(r)
            rz, beta = r @ z, (r @ z) / rz
            p = beta * p + z
        return 400
    k_amg, k_sgs = pcg(amg.apply), pcg(sgs)
    print("levels", [L["n"] for L in amg.levels], "k_amg", k_amg, "k_sgs", k_sgs)
    assert k_amg < k_sgs


# ---- 4. the host builder under the sanitizers ---------------------------------------------
def test_amg_build_check_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "amg_build_check")
    src = os.path.join(ROOT, "spmv_amd", "csrc", "host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-I" + src,
                    os.path.join(ROOT, "tools", "amg_build_check.cpp"),
                    os.path.join(src, "amg_build.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
