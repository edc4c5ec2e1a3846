"""CPU checks of the interface of the Chebyshev polynomial preconditioner
(spmv::chebyshev_coefficients, chebyshev_apply, pcg_chebyshev,
lambda_max_estimate): the new symbols are declared in both headers, exported and
prototyped with the declared number of arguments, the change is additive
(ABI 5), NULL handles and iteration indices are refused before anything touches
a device, cg.h states the rules, the Python layer has the entry points, and the
coefficients equal their restatement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_cheb_scale_f64", "spmv_hip_cheb_apply0_f64",
           "spmv_hip_cheb_step_f64", "spmv_hip_cheb_init_f64",
           "spmv_hip_cheb_update_r_f64", "spmv_hip_cheb_update_xp_f64")
HOST_NEW = ("spmvh_chebyshev_coefficients", "spmvh_chebyshev_workspace_create",
            "spmvh_chebyshev_workspace_destroy",
            "spmvh_chebyshev_workspace_reserve_timing", "spmvh_chebyshev_apply",
            "spmvh_pcg_chebyshev", "spmvh_lambda_max_estimate")
EINVAL = -1


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _declared_arity(header):
    """function name -> number of parameters of its declaration"""
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;",
                                 _header(header)):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_chebyshev_symbols_declared_exported_prototyped():
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
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)


def test_rules_are_stated():
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    for name in ("int pcg_chebyshev(", "void chebyshev_apply(",
                 "void chebyshev_coefficients(", "double lambda_max_estimate(",
                 "ChebyshevWorkspace"):
        assert name in cg_h, name
    # which options apply and which are ignored; the advised bounds
    part = cg_h[cg_h.index("CG with the Chebyshev polynomial preconditioner"):
                cg_h.index("int pcg_chebyshev(")]
    assert "consumer_reductions" in part and "defer_x and mixed are IGNORED" in part
    assert "poll_every and time_spmv apply" in part
    assert "lmax = 1.1 *" in part and "lmin = lmax / 30" in part
    hip_h = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert "d = a_j*d + b_j*(dinv*(r - w))" in hip_h


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    assert h.spmv_hip_cheb_scale_f64(None, 4, 1.0, None, None, None,
                                     None) == EINVAL
    assert h.spmv_hip_cheb_apply0_f64(None, 4, 1.0, None, None, None, None,
                                      None) == EINVAL
    assert h.spmv_hip_cheb_step_f64(None, None, 4, 0.5, 0.5, 0, None, None, None,
                                    None, None, None) == EINVAL
    assert h.spmv_hip_cheb_init_f64(None, None, 4, 1.0, None, None, None, None,
                                    None, None, None) == EINVAL
    assert h.spmv_hip_cheb_update_r_f64(None, None, 1, 4, 1.0, None, None, None,
                                        None, None, None) == EINVAL
    assert h.spmv_hip_cheb_update_xp_f64(None, None, 1, 4, None, None, None,
                                         None) == EINVAL
    # a context but no workspace, no vectors, a bad size or a vector that is not
    # 16-byte aligned: refused before the context is looked at -- the block of
    # memory standing in for it is never read
    ctx = C.create_string_buffer(4096)
    v = C.addressof(ctx) + 1024
    v -= v % 16
    assert h.spmv_hip_cheb_scale_f64(ctx, -1, 1.0, None, v, v, None) == EINVAL
    assert h.spmv_hip_cheb_scale_f64(ctx, 4, 1.0, None, None, v, None) == EINVAL
    assert h.spmv_hip_cheb_apply0_f64(ctx, 4, 1.0, None, None, None, None,
                                      None) == EINVAL
    assert h.spmv_hip_cheb_apply0_f64(ctx, -1, 1.0, v, None, v, v,
                                      None) == EINVAL
    assert h.spmv_hip_cheb_apply0_f64(ctx, 4, 1.0, v + 8, None, v, v,
                                      None) == EINVAL
    assert h.spmv_hip_cheb_step_f64(ctx, None, 4, 0.5, 0.5, 0, None, None, None,
                                    None, None, None) == EINVAL
    assert h.spmv_hip_cheb_step_f64(ctx, None, 4, 0.5, 0.5, 0, v, v, None, v,
                                    v + 8, None) == EINVAL
    assert h.spmv_hip_cheb_init_f64(ctx, None, 4, 1.0, v, None, v, v, v, v,
                                    None) == EINVAL
    assert h.spmv_hip_cheb_update_r_f64(ctx, None, 1, 4, 1.0, v, None, v, v, v,
                                        None) == EINVAL
    assert h.spmv_hip_cheb_update_xp_f64(ctx, None, 1, 4, v, v, v,
                                         None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k = C.c_int()
    lam = C.c_double()
    assert lib.spmvh_pcg_chebyshev(None, None, None, None, None, None, 4, 0.1,
                                   2.2, 10, 1e-8, C.byref(k), None, None, 0,
                                   None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_chebyshev_apply(None, None, None, None, None, 4, 0.1, 2.2,
                                     None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_lambda_max_estimate(None, None, None, None, None, 20,
                                         C.byref(lam)) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_chebyshev_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_chebyshev_workspace_reserve_timing(None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_chebyshev_workspace_destroy(None) == 0
    assert lib.spmvh_chebyshev_coefficients(2, 0.1, 2.2, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()


def test_python_layer_has_the_entry_points():
    assert callable(host.pcg_chebyshev) and callable(host.chebyshev_apply)
    assert callable(host.chebyshev_coefficients)
    assert callable(host.lambda_max_estimate)
    assert callable(host.ChebyshevWorkspace)
    assert callable(host.ChebyshevWorkspace.close)
    assert callable(host.ChebyshevWorkspace.reserve_timing)


# ---- the coefficients ------------------------------------------------------------
def coefficients_ref(degree, lmin, lmax):
    """cg.h restated: Python floats are fp64, one rounding per operation"""
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
    return np.array(a), np.array(b)


BOUNDS = ((2.2 / 30, 2.2), (0.013, 1.987654321), (3.0e-3, 1234.5678))


@pytest.mark.parametrize("degree", [1, 2, 5, 16])
@pytest.mark.parametrize("bounds", BOUNDS)
def test_coefficients_equal_the_restatement_bit_for_bit(degree, bounds):
    a, b = host.chebyshev_coefficients(degree, *bounds)
    a_ref, b_ref = coefficients_ref(degree, *bounds)
    assert a.shape == b.shape == (degree,)
    assert np.array_equal(a, a_ref), (degree, bounds, a, a_ref)
    assert np.array_equal(b, b_ref), (degree, bounds, b, b_ref)
    assert a[0] == 0.0 and np.all(b > 0.0) and np.all(a[1:] > 0.0)


def test_degree_and_bounds_errors():
    for degree in (0, -3, 17):
        with pytest.raises(host.SpmvHostError, match="degree"):
            host.chebyshev_coefficients(degree, 0.1, 2.2)
    inf, nan = float("inf"), float("nan")
    for lmin, lmax in ((0.0, 2.2), (-0.1, 2.2), (2.2, 2.2), (2.3, 2.2),
                       (0.1, inf), (nan, 2.2), (0.1, nan), (-inf, 2.2)):
        with pytest.raises(host.SpmvHostError, match="bounds"):
            host.chebyshev_coefficients(4, lmin, lmax)
