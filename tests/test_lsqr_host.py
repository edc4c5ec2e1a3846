"""spmv::lsqr without a GPU: lsqr_cases.py's restatement is held to
numpy.linalg.lstsq and to the damped normal equations, the per-kernel references
are shown to compose into lsqr_ref bit for bit, every exit is reached on a
hand-built case, and the argument rules, the exported symbols and the NULL
checks are exercised through the two libraries.

The bar against the dense solutions: the solves stop at a relative residual (or
least-squares) estimate of 1e-10, so x is off by at most about cond(A) * 1e-10;
cond is 1.5 for tall / wide and below 100 for convdiff11, hence 1e-8."""
import os
import re

import numpy as np
import pytest

import lsqr_cases as lc
import oracle
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = tuple("spmv_hip_lsqr_" + n for n in (
    "ws_create", "ws_destroy", "ws_reset", "ws_capacity", "ws_array",
    "ws_read_async", "ws_set_state", "ws_get_state", "update_u_f64",
    "update_v_f64", "reduce", "start", "step", "update_xw_f64"))
HOST_NEW = ("spmvh_lsqr_workspace_create", "spmvh_lsqr_workspace_destroy",
            "spmvh_lsqr_workspace_reserve_timing", "spmvh_lsqr_check_rules",
            "spmvh_lsqr")


def products(name):
    """-> (spmv, spmvt): oracle.csr_spmv on the matrix and on its stable
    transpose"""
    csr, ncols = lc.csr_by_name(name)
    T = lc.stable_transpose(csr, ncols)
    return (lambda q: oracle.csr_spmv(*csr, q)), (lambda q: oracle.csr_spmv(*T, q))


_CACHE = {}


def _case(name, kind, damp):
    key = (name, kind, damp)
    if key not in _CACHE:
        sp, spt = products(name)
        b = lc.rhs(name, kind, sp)
        args = (b, lc.KMAX, lc.RTOL, lc.LTOL, damp)
        _CACHE[key] = (sp, spt, b, lc.lsqr_ref(sp, spt, np.dot, *args),
                       lc.lsqr_ref(sp, spt, lc.dot_chunks64, *args))
    return _CACHE[key]


@pytest.mark.parametrize("case", sorted(lc.TABLE))
def test_the_restatement_against_the_dense_solution(case):
    name, kind, damp = case
    sp, spt, b, (x, k, hist_r, hist_ar, status), second = _case(*case)
    csr, ncols = lc.csr_by_name(name)
    A = lc.dense(csr, ncols)
    if damp == 0.0:  # (wide: lstsq returns the minimum-norm solution)
        want = np.linalg.lstsq(A, b, rcond=None)[0]
    else:
        want = np.linalg.solve(A.T @ A + damp * damp * np.eye(ncols), A.T @ b)
    err = np.linalg.norm(x - want) / np.linalg.norm(want)
    xdev = np.linalg.norm(second[0] - x) / np.linalg.norm(x)
    print(case, "k", k, second[1], "status", status, second[4], "error", err,
          "x of the two orders", xdev)
    assert (k, status) == lc.TABLE[case]
    assert abs(second[1] - k) <= 1 and second[4] == status
    assert len(hist_r) == len(hist_ar) == k + 1
    assert np.all(np.diff(hist_r) <= 0.0), "the residual estimate never grows"
    assert err <= 1e-8
    assert xdev <= 1e-9
    if status == 0:
        assert hist_r[k] / hist_r[0] < lc.RTOL <= hist_r[k - 1] / hist_r[0]
        assert np.linalg.norm(b - sp(x)) / np.linalg.norm(b) < 10 * lc.RTOL
    else:  # the estimate of hist_r against the true damped residual
        true = np.sqrt(np.linalg.norm(b - sp(x)) ** 2
                       + damp * damp * np.linalg.norm(x) ** 2)
        assert abs(hist_r[k] - true) <= 1e-9 * hist_r[0]
        g = spt(b - sp(x)) - damp * damp * x
        assert np.linalg.norm(g) <= 1e-8 * np.linalg.norm(spt(b))


def _by_kernels(sp, spt, b, kmax, rtol, ltol, damp, dot=np.dot):
    """the solve as the device runs it: update_v(first), start, update_xw(0),
    then update_u, update_v, step, update_xw per iteration, all from the kernel
    references"""
    ut = np.array(b, np.float64)
    n = len(spt(ut))
    x = np.zeros(n)
    uu = dot(ut, ut)
    vt = lc.lsqr_update_v(spt(ut), None, uu, 0.0, first=True)
    st = lc.lsqr_start(uu, 0.0 if vt is None else dot(vt, vt))
    hist_r, hist_ar = [st["hist_r0"]], [st["hist_ar0"] or 0.0]
    if st["done"]:
        return x, 0, np.array(hist_r), np.array(hist_ar), st["status"]
    w = lc.lsqr_scale(vt, st["ia"])
    k = 0
    while k < kmax:
        ut = lc.lsqr_update_u(sp(vt), ut, st["ia"], st["alpha"], st["ib"])
        uu = dot(ut, ut)
        vn = lc.lsqr_update_v(spt(ut), vt, uu, st["ia"])
        vv = 0.0 if vn is None else dot(vn, vn)
        vt = vt if vn is None else vn
        out = lc.lsqr_step(st, uu, vv, hist_r[0], k, kmax, rtol, ltol, damp)
        k = out["k"]
        hist_r.append(out["res"]), hist_ar.append(out["ares"])
        x, w = lc.lsqr_update_xw(vt, w, x, out["t1"], out.get("t2", 0.0),
                                 out.get("ia", 0.0), go_on=not out["done"])
        if out["done"]:
            return x, k, np.array(hist_r), np.array(hist_ar), out["status"]
        st = dict(out)
    return x, k, np.array(hist_r), np.array(hist_ar), 0


@pytest.mark.parametrize("name,kind,damp", [("convdiff11_2", "rand", 0.0),
                                            ("tall", "rand", 0.5),
                                            ("wide", "ones", 0.0)])
def test_the_kernel_references_compose_into_the_recurrence(name, kind, damp):
    sp, spt, b, first, _ = _case(name, kind, damp)
    for kmax, rtol, ltol in ((lc.KMAX, lc.RTOL, lc.LTOL), (7, 0.0, 0.0)):
        ref = first if kmax == lc.KMAX else lc.lsqr_ref(sp, spt, np.dot, b, kmax,
                                                        rtol, ltol, damp)
        x, k, hist_r, hist_ar, status = _by_kernels(sp, spt, b, kmax, rtol, ltol,
                                                    damp)
        assert (k, status) == (ref[1], ref[4])
        assert np.array_equal(hist_r, ref[2]) and np.array_equal(hist_ar, ref[3])
        assert np.array_equal(x, ref[0])


# ---- the exits, on hand-built cases ------------------------------------------
EXITS = {
    # one singular value: the bidiagonalisation ends after one step
    "identity": (np.eye(3), [1.0, 1.0, 1.0], 0.0, 50, 1e-12, 0.0, 1, 2),
    # A^T b = 0: x = 0 is the least-squares solution
    "orthogonal": ([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], [0.0, 0.0, 1.0], 0.0, 50,
                   1e-12, 0.0, 0, 2),
    # three distinct singular values: three steps
    "diag123": (np.diag([1.0, 2.0, 3.0]), [1.0, 1.0, 1.0], 0.0, 50, 1e-12, 0.0,
                3, None),
    # an inconsistent system: the least-squares test
    "ltol": ([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]], [1.0, 1.0, -1.0], 0.0, 50,
             1e-14, 1e-10, None, 1),
    # ... and damped
    "ltol_damped": ([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]], [1.0, 1.0, -1.0], 0.5,
                    50, 1e-14, 1e-10, None, 1),
    "kmax": (np.diag([1.0, 2.0, 3.0, 4.0]), [1.0, 1.0, 1.0, 1.0], 0.0, 2, 0.0, 0.0,
             2, 0),
    "rtol": (np.diag([1.0, 2.0, 3.0, 4.0]), [1.0, 1.0, 1.0, 1.0], 0.0, 50, 0.5,
             0.0, None, 0),
}


def _dense_products(A):
    A = np.asarray(A, np.float64)

    def mult(M):
        def go(q):  # row sums left to right, the product rounded first
            out = np.zeros(M.shape[0])
            for i in range(M.shape[0]):
                s = 0.0
                for j in range(M.shape[1]):
                    s += float(M[i, j] * q[j])
                out[i] = s
            return out
        return go
    return mult(A), mult(A.T.copy())


def exit_case(name):
    A, b, damp, kmax, rtol, ltol, k, status = EXITS[name]
    sp, spt = _dense_products(A)
    ref = lc.lsqr_ref(sp, spt, lc.dot_plain, np.array(b), kmax, rtol, ltol, damp)
    return np.asarray(A, np.float64), np.array(b), damp, kmax, rtol, ltol, ref, \
        k, status


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_exit_is_reached(name):
    A, b, damp, kmax, rtol, ltol, (x, k, hist_r, hist_ar, status), k_want, \
        status_want = exit_case(name)
    print(name, "k", k, "status", status, "x", x, "hist_r", hist_r, "hist_ar",
          hist_ar)
    assert status_want is None or status == status_want
    assert k_want is None or k == k_want
    assert np.all(np.isfinite(x)) and len(hist_r) == len(hist_ar) == k + 1
    if name in ("identity", "diag123"):
        assert np.allclose(A @ x, b, rtol=0, atol=1e-12)
    if name == "orthogonal":
        assert np.all(x == 0.0) and np.all(A.T @ b == 0.0)
    if name.startswith("ltol"):
        want = np.linalg.solve(A.T @ A + damp * damp * np.eye(2), A.T @ b)
        assert np.allclose(x, want, rtol=0, atol=1e-9)
    if name == "rtol":
        assert 0 < k < 4 and hist_r[k] / hist_r[0] < 0.5


def test_a_zero_right_hand_side_returns_at_once():
    sp, spt = _dense_products(np.eye(3))
    x, k, hist_r, hist_ar, status = lc.lsqr_ref(sp, spt, np.dot, np.zeros(3), 10,
                                                1e-10, 1e-10, 0.0)
    assert (k, status) == (0, 0) and np.all(x == 0.0)
    assert list(hist_r) == [0.0] and list(hist_ar) == [0.0]


def test_a_nan_runs_to_kmax():
    sp, spt = _dense_products(np.diag([1.0, 2.0, 3.0]))
    x, k, hist_r, hist_ar, status = lc.lsqr_ref(
        sp, spt, np.dot, np.array([1.0, np.nan, 1.0]), 6, 1e-10, 1e-10, 0.0)
    assert (k, status) == (6, 0) and np.all(np.isnan(hist_r))


# ---- the argument rules, through the host library ----------------------------
def test_check_rules_error_strings():
    buf = np.zeros(64)
    p = buf.ctypes.data
    ok = dict(kmax=5, rows=8, cols=4, b_ptr=p, x_ptr=p + 8 * 8)
    host.lsqr_check_rules(**ok)
    host.lsqr_check_rules(**ok, ltol=1e-8, damp=0.5)
    host.lsqr_check_rules(kmax=0)  # empty ranges never overlap
    host.lsqr_check_rules(**dict(ok, b_ptr=p + 4 * 8, x_ptr=p))  # x in front
    bad = [
        (dict(ok, kmax=-1), "kmax"),
        (dict(ok, ltol=-1e-3), "ltol"),
        (dict(ok, ltol=float("nan")), "ltol"),
        (dict(ok, ltol=float("inf")), "ltol"),
        (dict(ok, damp=-0.5), "damp"),
        (dict(ok, damp=float("nan")), "damp"),
        (dict(ok, damp=float("inf")), "damp"),
        (dict(ok, x_ptr=p + 7 * 8), "x overlaps b"),
        (dict(ok, b_ptr=p + 3 * 8, x_ptr=p), "x overlaps b"),
    ]
    for kw, text in bad:
        with pytest.raises(host.SpmvHostError, match=text):
            host.lsqr_check_rules(**kw)
    # the order: kmax before ltol before damp
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.lsqr_check_rules(kmax=-1, ltol=-1.0, damp=-1.0)
    with pytest.raises(host.SpmvHostError, match="ltol"):
        host.lsqr_check_rules(kmax=1, ltol=-1.0, damp=-1.0)


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
    assert callable(host.lsqr) and callable(host.lsqr_check_rules)
    assert issubclass(host.LsqrWorkspace, object)


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)


def test_null_handles_rejected():
    h = _lib.hip
    for n in HIP_NEW:
        if n == "spmv_hip_lsqr_ws_destroy":  # (destroying nothing is allowed)
            assert h.spmv_hip_lsqr_ws_destroy(None) == 0
            continue
        fn = getattr(h, n)
        args = [0 if t in (_lib.C.c_int, _lib.C.c_int64, _lib.C.c_size_t)
                else 0.0 if t is _lib.C.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, n
    for n in ("spmvh_lsqr_workspace_create", "spmvh_lsqr_workspace_reserve_timing",
              "spmvh_lsqr"):
        fn = getattr(host.lib, n)
        args = [0 if t is host.C.c_int else 0.0 if t is host.C.c_double else None
                for t in fn.argtypes]
        assert fn(*args) != 0, n
        assert b"NULL" in host.lib.spmvh_last_error(), n
