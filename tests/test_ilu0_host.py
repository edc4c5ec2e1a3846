"""CPU checks of the multicolour ILU(0) preconditioner (spmv::Ilu0Preconditioner):
the new symbols are declared in both headers, exported and prototyped, the
change is additive (ABI 5), NULL handles are refused before anything touches a
device, the symbolic builder (host/ilu0_build.h) equals the numpy restatement of
ilu0_cases.py, and the restatement itself has the defining property of ILU(0):
(D~ + L~) D~^-1 (D~ + U~) equals A on the pattern of A.

Matrices: Poisson 5^3, gmres_cases.banded(257) and convdiff(4) (nonsymmetric),
the arrow matrix of 130 rows, a diagonal matrix and n = 1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gmres_cases as gc
import ilu0_cases as ic
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_ilu0_plan_create", "spmv_hip_ilu0_plan_destroy",
           "spmv_hip_ilu0_plan_bytes", "spmv_hip_ilu0_mcgs_plan",
           "spmv_hip_ilu0_factor", "spmv_hip_ilu0_pivots",
           "spmv_hip_ilu0_get_pattern", "spmv_hip_ilu0_get_factor")
HOST_NEW = ("spmvh_ilu0_symbolic_create", "spmvh_ilu0_symbolic_get",
            "spmvh_ilu0_symbolic_destroy", "spmvh_ilu0_create",
            "spmvh_ilu0_refactor", "spmvh_ilu0_info", "spmvh_ilu0_pattern",
            "spmvh_ilu0_factor", "spmvh_matrix_local_values",
            "spmvh_matrix_plan_values_changed")
EINVAL = -1


def _diagonal_matrix(n):
    i = np.arange(n)
    return (np.arange(n + 1).astype(np.int32), i.astype(np.int32),
            2.0 + np.sin(i) ** 2)


def _csr(name):
    if name == "arrow130":
        return ic.arrow(130)
    if name.startswith("diag"):
        return _diagonal_matrix(int(name[4:]))
    return gc.csr_by_name(name)


NAMES = ("poisson5", "banded257", "convdiff4", "arrow130", "diag40", "diag1")
SYMMETRIC_NAMES = ("poisson5", "diag40", "diag1")


# ---- 1. the interface -------------------------------------------------------------
def _declared_arity(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_ilu0_symbols_declared_exported_prototyped():
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
    assert issubclass(host.Ilu0Preconditioner, host.SgsPreconditioner)
    for name in ("refactor", "negative_pivots", "factor", "pattern", "colors"):
        assert callable(getattr(host.Ilu0Preconditioner, name)), name
    assert callable(host.ilu0_apply) and callable(host.ilu0_symbolic)
    assert callable(host.Matrix.local_values)
    assert callable(host.Matrix.plan_values_changed)


def test_null_handles_refused_without_a_device():
    hip = _lib.hip
    out, n64 = C.c_void_p(), C.c_int64()
    assert hip.spmv_hip_ilu0_plan_create(None, None, C.byref(out)) == EINVAL
    assert hip.spmv_hip_ilu0_plan_destroy(None) == 0
    assert hip.spmv_hip_ilu0_plan_bytes(None, C.byref(n64)) == EINVAL
    assert hip.spmv_hip_ilu0_mcgs_plan(None, C.byref(out)) == EINVAL
    assert hip.spmv_hip_ilu0_factor(None, None, None, None, None) == EINVAL
    assert hip.spmv_hip_ilu0_pivots(None, None, C.byref(n64), C.byref(n64),
                                    None) == EINVAL
    assert hip.spmv_hip_ilu0_get_pattern(None, None, None, None, None,
                                         None) == EINVAL
    assert hip.spmv_hip_ilu0_get_factor(None, None, None, None, None,
                                        None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    out = C.c_void_p()
    info = np.zeros(6, np.int64)
    assert lib.spmvh_ilu0_create(None, None, C.byref(out)) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_ilu0_refactor(None, None) != 0
    assert lib.spmvh_ilu0_info(None, info.ctypes.data_as(C.c_void_p)) != 0
    assert lib.spmvh_ilu0_pattern(None, None, None, None, None) != 0
    assert lib.spmvh_ilu0_factor(None, None, None, None) != 0
    assert lib.spmvh_ilu0_symbolic_destroy(None) == 0
    assert lib.spmvh_matrix_plan_values_changed(None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_matrix_local_values(None, C.byref(out), C.byref(out)) != 0


# ---- 2. the symbolic builder against the restatement ----------------------------------
def _check_symbolic(csr, n, symmetric, what):
    sym = host.ilu0_symbolic(csr[0], csr[1], n, n, symmetric)
    colours, nc = host.sgs_color(csr[0], csr[1], n, n, symmetric)
    assert np.array_equal(sym["colors"], colours) and sym["num_colors"] == nc, what
    assert np.array_equal(colours, ic.greedy_colours(csr, n, symmetric)), what
    ref = ic.Ilu0Ref(csr, n, colours, symmetric)
    assert np.array_equal(sym["perm"], ref.perm), what
    assert np.array_equal(sym["pos"], ref.pos), what
    assert np.array_equal(sym["color_start"], ref.color_start), what
    for got, want in zip((sym["before"], sym["after"]), ref.parts):
        assert np.array_equal(got["ptr"], want["ptr"]), what
        assert np.array_equal(got["cpos"], want["cpos"]), what
        assert np.array_equal(got["src"], want["src"]), what
        # position order, and every entry's slot holds its column
        for p in range(n):
            row = got["cpos"][got["ptr"][p]:got["ptr"][p + 1]]
            assert np.all(np.diff(row) > 0), (what, p)
        slot = got["slot"]
        assert len(np.unique(slot)) == len(slot), what
        where = np.where(slot >= 0, slot, 0)
        in_slices = got["sliced_col"][where] if len(got["sliced_col"]) else where
        long_col = got["long_col"][np.where(slot < 0, ~slot, 0)] \
            if len(got["long_col"]) else where
        col = np.where(slot >= 0, in_slices, long_col)
        assert np.array_equal(col, want["col"]), what
    return sym, ref


@pytest.mark.parametrize("name", NAMES)
def test_symbolic_builder_equals_the_restatement(name):
    csr = _csr(name)
    n = len(csr[0]) - 1
    sym, ref = _check_symbolic(csr, n, False, name)
    if name == "arrow130":
        assert sym["num_colors"] == 2 and sym["color_start"][1] == n - 1
        assert len(sym["after"]["long_col"]) == 0  # rows of one entry
        assert len(sym["before"]["long_col"]) == n - 1  # the hub: a long row
    if name.startswith("diag"):
        assert sym["num_colors"] == 1
        assert len(sym["before"]["cpos"]) == len(sym["after"]["cpos"]) == 0
    if name == "poisson5":
        assert sym["num_colors"] == 2


@pytest.mark.parametrize("name", SYMMETRIC_NAMES)
def test_both_storages_of_a_symmetric_matrix_give_identical_parts(name):
    csr = _csr(name)
    n = len(csr[0]) - 1
    general, _ = _check_symbolic(csr, n, False, name)
    rows = gc.row_of(csr[0])
    low = csr[1] <= rows  # the input form: entries above the diagonal dropped
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[low], minlength=n))])
    lower = (rp.astype(np.int32), csr[1][low], csr[2][low])
    for stored in (csr, lower):
        sym, _ = _check_symbolic(stored, n, True, (name, "symmetric"))
        for key in ("colors", "perm", "pos", "color_start"):
            assert np.array_equal(sym[key], general[key]), (name, key)
        for part in ("before", "after"):
            for key in ("ptr", "cpos", "slot", "sliced_col", "long_col"):
                assert np.array_equal(sym[part][key], general[part][key]), \
                    (name, part, key)


def test_a_duplicate_column_is_refused():
    rp = np.array([0, 3, 5, 7], np.int32)
    ci = np.array([0, 2, 2, 1, 0, 2, 0], np.int32)  # row 0 holds (0, 2) twice
    with pytest.raises(host.SpmvHostError, match="duplicate"):
        host.ilu0_symbolic(rp, ci, 3, 3, False)
    with pytest.raises(ValueError, match="duplicate"):
        ic.Ilu0Ref((rp, ci, np.ones(7)), 3, [0, 0, 1], False)
    # a duplicate of the diagonal is Matrix::diagonal's business: their sum
    ci2 = np.array([0, 0, 2, 1, 0, 2, 0], np.int32)
    sym = host.ilu0_symbolic(rp, ci2, 3, 3, False)
    assert len(sym["before"]["cpos"]) + len(sym["after"]["cpos"]) == 3
    # symmetric storage: the stored lower entry and a stored mirror image of it
    rp3 = np.array([0, 1, 4], np.int32)
    ci3 = np.array([0, 0, 0, 1], np.int32)
    with pytest.raises(host.SpmvHostError, match="duplicate"):
        host.ilu0_symbolic(rp3, ci3, 2, 2, True)


def test_rows_and_owned_columns_must_be_the_same_range():
    csr = gc.poisson(3)
    for ncols in (26, 28):
        with pytest.raises(host.SpmvHostError, match="same index range"):
            host.ilu0_symbolic(csr[0], csr[1], 27, ncols, False)


def test_ghost_columns_are_ignored():
    csr = gc.poisson(4)
    n = 40  # the first 40 rows; columns >= 40 are ghosts
    rp = csr[0][:n + 1]
    local = (rp, csr[1][:rp[-1]], csr[2][:rp[-1]])
    _check_symbolic(local, n, False, "ghosts")


# ---- 3. the restatement has the defining property ----------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_reproduces_a_on_its_pattern(name):
    """(D~ + L~) D~^-1 (D~ + U~) = A at every entry of A (and on the diagonal):
    to 8 ulps of the sum of the absolute values of the row -- every entry of the
    product is a sum of at most a row's length of terms of that size."""
    csr = _csr(name)
    rp, ci, va = csr
    n = len(rp) - 1
    ref = ic.Ilu0Ref(csr, n, ic.greedy_colours(csr, n), False)
    fac = ref.factor()
    assert np.all(np.isfinite(fac[2])) and np.all(fac[2] > 0)
    M = ref.dense_m(fac)
    A = np.zeros((n, n))
    rows = gc.row_of(rp)
    A[rows, ci] = va
    on = A != 0
    scale = np.abs(A).sum(axis=1)[:, None] * np.ones((1, n))
    err = np.abs(M - A)[on] / scale[on]
    print(name, "max error on the pattern / row sum", err.max() if on.any() else 0)
    assert np.all(err <= 8 * 2.0 ** -53), (name, err.max())
    if name == "arrow130":  # no fill is dropped: M = A everywhere
        assert np.all(np.abs(M - A) <= 8 * 2.0 ** -53 * scale)
    if name in ("banded257", "convdiff4"):  # fill IS dropped somewhere
        assert np.any(M[~on] != 0.0)
    # the sweeps invert that product
    r = np.random.default_rng(n).uniform(-1, 1, n)
    z = ref.apply(fac, r)
    assert np.allclose(M @ z, r, rtol=0, atol=1e-12 * np.abs(M).sum(axis=1).max())
