"""spmv::cg_shifted without a GPU: cgs_cases.py's restatement is held to
numpy.linalg.solve on every shifted matrix, to plain CG where ns = 1 and sigma =
0, to its own symmetries (duplicates, permutations), the per-kernel references
are shown to compose into cgs_ref bit for bit, every exit is reached, and the
argument rules, the exported symbols and the NULL checks are exercised through
the two libraries.

The bar against the dense solutions: a solve whose relative residual met rtol
within a factor 10 has ||x - x_dense|| <= 10 * rtol * cond2(A + sigma I) *
||x_dense||; cond2 is computed here."""
import os
import re

import numpy as np
import pytest

import blas1_cases as bc
import cgs_cases as cc
import gmres_cases as gc
import minres_cases as mc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = tuple("spmv_hip_cgs_" + n for n in (
    "ws_create", "ws_destroy", "ws_reset", "ws_capacity", "ws_array",
    "ws_read_async", "ws_set_words", "ws_get_words", "update_r_f64", "reduce",
    "start", "step", "update_xp_f64"))
HOST_NEW = ("spmvh_cgs_workspace_create", "spmvh_cgs_workspace_destroy",
            "spmvh_cgs_workspace_reserve_timing", "spmvh_cgs_check_rules",
            "spmvh_cg_shifted")

_CACHE = {}


def spmv_of(csr):
    return lambda q: gc.csr_spmv(csr, q)


def poisson_case(which):
    """-> (csr, spmv, b, cgs_ref(...))"""
    if which not in _CACHE:
        csr = cc.poisson11()
        sp = spmv_of(csr)
        b = cc.poisson11_rhs()
        _CACHE[which] = (csr, sp, b, cc.cgs_ref(sp, np.dot, b,
                                                cc.SHIFT_SETS[which], cc.KMAX,
                                                cc.RTOL))
    return _CACHE[which]


def same(a, b):
    return bc.same_bits(a, b)


# ---- the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["four", "eight"])
def test_the_restatement_against_the_dense_solutions(which):
    csr, sp, b, (X, k, its, hist, status) = poisson_case(which)
    A = cc.dense(csr)
    print(which, "iterations", its, "status", status)
    assert status == 0 and tuple(its) == cc.COUNTS[which] and k == max(its)
    for s, sigma in enumerate(cc.SHIFT_SETS[which]):
        As = A + sigma * np.eye(len(b))
        x = np.linalg.solve(As, b)
        cond = np.linalg.cond(As, 2)
        err = np.linalg.norm(X[s] - x) / np.linalg.norm(x)
        res = np.linalg.norm(b - As @ X[s]) / np.linalg.norm(b)
        print("sigma", sigma, "k", its[s], "cond2", cond, "error", err, "bar",
              10 * cc.RTOL * cond, "true residual", res, "estimate",
              hist[s, its[s]] / hist[s, 0])
        assert hist[s, its[s]] / hist[s, 0] < cc.RTOL
        assert np.all(hist[s, its[s] + 1:] == -1.0)
        assert np.all(hist[s, :its[s]] / hist[s, 0] >= cc.RTOL)
        assert err <= 10 * cc.RTOL * cond
        assert res <= 10 * cc.RTOL


def test_one_shift_of_zero_is_plain_cg():
    """|k - k_cg| <= 1 and the history within the bars of test_gpu_minres.py:
    max(1e-9, 10 * dev_ref) of ||r_0||, dev_ref from the two summation orders"""
    csr, sp, b, (X, k, its, hist, status) = poisson_case("one")
    norms = mc.cg_norms(sp, b, cc.KMAX)
    k_cg = int(np.argmax(norms / norms[0] < cc.RTOL))
    second = cc.cgs_ref(sp, mc.dot_chunks64, b, cc.SHIFTS1, cc.KMAX, cc.RTOL)
    n = min(k, k_cg, second[1])
    dev_ref = np.abs(second[3][0, :n + 1] - hist[0, :n + 1]).max() / hist[0, 0]
    dev = np.abs(norms[:n + 1] - hist[0, :n + 1]).max() / hist[0, 0]
    print("k", k, "k_cg", k_cg, "history deviation", dev, "dev_ref", dev_ref)
    assert tuple(its) == cc.COUNTS["one"] and abs(k - k_cg) <= 1
    assert dev_ref <= 1e-5 and dev <= max(1e-9, 10 * dev_ref)


def test_duplicates_and_permutations_keep_the_bits():
    csr, sp, b, (X, k, its, hist, status) = poisson_case("four")
    dup = cc.cgs_ref(sp, np.dot, b, (1.0, 0.1, 1.0, 1.0), cc.KMAX, cc.RTOL)
    assert same(dup[0][0], dup[0][2]) and same(dup[0][0], dup[0][3])
    assert same(dup[3][0], dup[3][2]) and dup[2][0] == dup[2][2] == dup[2][3]
    assert same(dup[0][0], X[2]) and same(dup[0][1], X[1])
    perm = (2, 0, 3, 1)
    got = cc.cgs_ref(sp, np.dot, b, [cc.SHIFTS4[i] for i in perm], cc.KMAX,
                     cc.RTOL)
    for j, i in enumerate(perm):
        assert same(got[0][j], X[i]) and same(got[3][j], hist[i])
        assert got[2][j] == its[i]
    # a column of the eight-shift solve equals the one-shift solve
    X8, k8, its8, hist8, _ = poisson_case("eight")[3]
    for s in (0, 4):
        one = cc.cgs_ref(sp, np.dot, b, (cc.SHIFTS8[s],), cc.KMAX, cc.RTOL)
        assert one[2][0] == its8[s] and same(one[0][0], X8[s])


# ---- the exits -------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.EXITS)
def test_every_exit_is_reached(name):
    csr, b, shifts, kmax, rtol, k_want, status_want = cc.exit_case(name)
    X, k, its, hist, status = cc.cgs_ref(spmv_of(csr), np.dot, b, shifts, kmax,
                                         rtol)
    print(name, "k", k, "iterations", its, "status", status)
    assert status == status_want and (k_want is None or k == k_want)
    if name == "zero":
        assert its == [0] * len(shifts) and np.all(X == 0.0)
        assert np.all(hist[:, 0] == 0.0)
    if name == "indefinite":
        assert 0 < k < 10 and np.all(np.isfinite(X))
    if name == "negative":
        assert np.all(X == 0.0)
    if name == "underflow":
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(hist))
        assert hist[2, kmax] == 0.0  # zeta of sigma = 1e6 has underflowed
        A = cc.dense(csr)
        for s, sigma in enumerate(shifts):
            x = np.linalg.solve(A + sigma * np.eye(len(b)), b)
            err = np.linalg.norm(X[s] - x) / np.linalg.norm(x)
            print("sigma", sigma, "error", err)
            assert err <= 1e-12
    if name == "identity":
        for s, sigma in enumerate(shifts):
            assert np.allclose(X[s], b / (1.0 + sigma), rtol=1e-15, atol=0)
    if name == "nan":
        assert np.all(X == 0.0) and np.all(np.isnan(hist[:, 0]))


# ---- the kernel references ------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "four", "eight"])
def test_the_kernel_references_compose_into_the_recurrence(which):
    csr, sp, b, ref = poisson_case(which)
    got = cc.cgs_compose(sp, np.dot, b, cc.SHIFT_SETS[which], cc.KMAX, cc.RTOL)
    assert same(got[0], ref[0]) and same(got[3], ref[3])
    assert (got[1], list(got[2]), got[4]) == (ref[1], list(ref[2]), ref[4])
    # a fixed number of steps, and the device's summation order
    for dot, kmax, rtol in ((np.dot, 7, 0.0), (cc.device_dot(2048), 12, 1e-3)):
        a = cc.cgs_ref(sp, dot, b, cc.SHIFT_SETS[which], kmax, rtol)
        c = cc.cgs_compose(sp, dot, b, cc.SHIFT_SETS[which], kmax, rtol)
        assert same(a[0], c[0]) and same(a[3], c[3])
        assert (a[1], list(a[2]), a[4]) == (c[1], list(c[2]), c[4])


@pytest.mark.parametrize("name", cc.EXITS)
def test_the_kernel_references_compose_on_the_exits(name):
    csr, b, shifts, kmax, rtol, _, _ = cc.exit_case(name)
    kmax = min(kmax, 60)
    a = cc.cgs_ref(spmv_of(csr), np.dot, b, shifts, kmax, rtol)
    c = cc.cgs_compose(spmv_of(csr), np.dot, b, shifts, kmax, rtol)
    assert same(a[0], c[0]) and (a[1], list(a[2]), a[4]) == (c[1], list(c[2]), c[4])
    assert np.array_equal(a[3], c[3], equal_nan=True)


def test_the_device_dot_model():
    """set E: whatever the order, the sum is the exact integer; odd lengths,
    several workgroups, several trips"""
    for n in (0, 1, 2, 3, 511, 513, bc.UNIT + 1, 3 * bc.UNIT + 5):
        x, y = bc.exact_vec(n, 1), bc.exact_vec(n, 2)
        for blocks in (1, 2, 2048):
            assert cc.device_dot(blocks)(x, y) == bc.exact_dot_int(x, y)
    xr, yr = bc.round_vec(5000, 1), bc.round_vec(5000, 2)
    ex, sa = bc.exact_dot(xr, yr)
    assert bc.sum_within(cc.device_dot(2048)(xr, yr), ex, sa,
                         bc.depth(5000, 2048))


# ---- the argument rules ------------------------------------------------------------
def test_check_rules_error_strings():
    buf = np.zeros(64)
    p = buf.ctypes.data
    ok = dict(ns=2, kmax=5, rows=8, ldx=8, shifts=(0.0, 1.0), b_ptr=p,
              x_ptr=p + 8 * 8)
    host.cgs_check_rules(**ok)
    host.cgs_check_rules(**dict(ok, ldx=9, shifts=(2.0, 2.0)))
    host.cgs_check_rules(**dict(ok, b_ptr=p + 16 * 8, x_ptr=p))  # X in front
    host.cgs_check_rules(**dict(ok, ns=8, shifts=cc.SHIFTS8, x_ptr=p + 64 * 8))
    bad = [
        (dict(ok, ns=0), "ns"),
        (dict(ok, ns=9, shifts=(0.0,) * 9), "ns"),
        (dict(ok, kmax=-1), "kmax"),
        (dict(ok, ldx=7), "ldx"),
        (dict(ok, shifts=None), "shifts"),
        (dict(ok, shifts=(0.0, -1e-3)), "shifts"),
        (dict(ok, shifts=(float("nan"), 1.0)), "shifts"),
        (dict(ok, shifts=(0.0, float("inf"))), "shifts"),
        (dict(ok, x_ptr=p + 7 * 8), "overlaps"),
        (dict(ok, x_ptr=p), "overlaps"),
        # the second column reaches b
        (dict(ok, b_ptr=p + 16 * 8, x_ptr=p + 1 * 8), "overlaps"),
    ]
    for kw, name in bad:
        with pytest.raises(host.SpmvHostError, match=name):
            host.cgs_check_rules(**kw)
    # the order: ns before kmax before ldx before shifts before overlaps
    with pytest.raises(host.SpmvHostError, match="ns must"):
        host.cgs_check_rules(**dict(ok, ns=0, kmax=-1, ldx=0, shifts=None))
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.cgs_check_rules(**dict(ok, kmax=-1, ldx=0, shifts=None))
    with pytest.raises(host.SpmvHostError, match="ldx"):
        host.cgs_check_rules(**dict(ok, ldx=0, shifts=None))
    with pytest.raises(host.SpmvHostError, match="shifts"):
        host.cgs_check_rules(**dict(ok, shifts=(-1.0, 0.0), x_ptr=p))


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
    assert callable(host.cg_shifted) and callable(host.cgs_check_rules)
    assert issubclass(host.CgShiftedWorkspace, object)


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)


def test_null_handles_rejected():
    h = _lib.hip
    for n in HIP_NEW:
        if n == "spmv_hip_cgs_ws_destroy":  # (destroying nothing is allowed)
            assert h.spmv_hip_cgs_ws_destroy(None) == 0
            continue
        fn = getattr(h, n)
        args = [0 if t in (_lib.C.c_int, _lib.C.c_int64, _lib.C.c_size_t)
                else 0.0 if t is _lib.C.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, n
    for n in ("spmvh_cgs_workspace_create", "spmvh_cgs_workspace_reserve_timing",
              "spmvh_cg_shifted"):
        fn = getattr(host.lib, n)
        args = [0 if t in (host.C.c_int, host.C.c_int64) else 0.0
                if t is host.C.c_double else None for t in fn.argtypes]
        assert fn(*args) != 0, n
        assert b"NULL" in host.lib.spmvh_last_error(), n
