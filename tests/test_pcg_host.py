"""CPU checks of the interface of spmv::pcg (CG with a diagonal preconditioner),
Matrix::diagonal and jacobi_inverse: the new symbols are declared in both
headers, exported and prototyped with the declared number of arguments, the
change is additive (ABI 5), NULL handles and iteration indices are refused
before anything touches a device, cg.h states the rules, and the Python layer
has the entry points."""
import ctypes as C
import os
import re

from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_pcg_ws_create", "spmv_hip_pcg_ws_destroy",
           "spmv_hip_pcg_ws_reset", "spmv_hip_pcg_ws_capacity",
           "spmv_hip_pcg_ws_rz_rr", "spmv_hip_pcg_ws_pAp",
           "spmv_hip_pcg_ws_partials", "spmv_hip_pcg_ws_done_flag",
           "spmv_hip_pcg_ws_read_async", "spmv_hip_pcg_init_f64",
           "spmv_hip_pcg_update_r_f64", "spmv_hip_pcg_update_xp_f64",
           "spmv_hip_pcg_reduce_pAp", "spmv_hip_pcg_reduce_pAp2",
           "spmv_hip_pcg_reduce_rz_rr", "spmv_hip_pcg_update_r_cs_f64",
           "spmv_hip_pcg_update_xp_cs_f64", "spmv_hip_csr_diagonal_f64",
           "spmv_hip_csr_diagonal_f32", "spmv_hip_jacobi_invert_f64")
HOST_NEW = ("spmvh_matrix_diagonal", "spmvh_jacobi_inverse",
            "spmvh_pcg_workspace_create", "spmvh_pcg_workspace_destroy",
            "spmvh_pcg_workspace_reserve_timing", "spmvh_pcg")
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


def test_pcg_symbols_declared_exported_prototyped():
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
    assert "int pcg(" in cg_h and "PcgWorkspace" in cg_h
    assert "jacobi_inverse" in cg_h
    # which options apply, which are ignored, and the zero right-hand side
    assert "defer_x and" in cg_h and "IGNORED" in cg_h
    assert "r_0 . r_0 == 0 stops at k = 0" in cg_h
    m_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "matrix.h")).read()
    assert "void diagonal(T* d) const;" in m_h and "release_csr" in m_h
    hip_h = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert "{rz[k], rr[k]}" in hip_h and "ADJACENT" in hip_h


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    out = C.c_void_p()
    k = C.c_int()
    assert h.spmv_hip_pcg_ws_create(None, 10, C.byref(out)) == EINVAL
    assert out.value is None
    assert h.spmv_hip_pcg_ws_destroy(None) == 0  # like free(NULL)
    assert h.spmv_hip_pcg_ws_reset(None, 1e-8, None) == EINVAL
    assert h.spmv_hip_pcg_ws_capacity(None, C.byref(k)) == EINVAL
    assert h.spmv_hip_pcg_ws_rz_rr(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcg_ws_pAp(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcg_ws_partials(None, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcg_ws_done_flag(None, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcg_ws_read_async(None, None, None, 0, None) == EINVAL
    assert h.spmv_hip_pcg_init_f64(None, None, 4, None, None, None, None, None,
                                   None) == EINVAL
    assert h.spmv_hip_pcg_update_r_f64(None, None, 1, 4, None, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_pcg_update_xp_f64(None, None, 1, 4, None, None, None,
                                        None, None) == EINVAL
    assert h.spmv_hip_pcg_reduce_pAp(None, None, 1, None) == EINVAL
    assert h.spmv_hip_pcg_reduce_pAp2(None, None, 1, None, None) == EINVAL
    assert h.spmv_hip_pcg_reduce_rz_rr(None, None, 0, None) == EINVAL
    assert h.spmv_hip_pcg_update_r_cs_f64(None, None, 1, 4, None, None, None,
                                          None, None) == EINVAL
    assert h.spmv_hip_pcg_update_xp_cs_f64(None, None, 1, 4, None, None, None,
                                           None, None) == EINVAL
    assert h.spmv_hip_csr_diagonal_f64(None, 4, None, None, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_csr_diagonal_f32(None, 4, None, None, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_jacobi_invert_f64(None, 4, None, None, None,
                                        None) == EINVAL
    # a context but no workspace (or bad sizes): refused before the context is
    # looked at -- the block of memory standing in for it is never read
    ctx = C.create_string_buffer(4096)
    assert h.spmv_hip_pcg_ws_create(ctx, -1, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcg_ws_create(ctx, 10, None) == EINVAL
    assert h.spmv_hip_pcg_init_f64(ctx, None, 4, None, None, None, None, None,
                                   None) == EINVAL
    assert h.spmv_hip_pcg_reduce_pAp(ctx, None, 1, None) == EINVAL
    assert h.spmv_hip_pcg_reduce_rz_rr(ctx, None, 0, None) == EINVAL
    assert h.spmv_hip_pcg_update_r_cs_f64(ctx, None, 1, 4, None, None, None,
                                          None, None) == EINVAL
    assert h.spmv_hip_csr_diagonal_f64(ctx, -1, None, None, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_csr_diagonal_f64(ctx, 4, None, None, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_jacobi_invert_f64(ctx, 4, None, None, None,
                                        None) == EINVAL
    assert h.spmv_hip_jacobi_invert_f64(ctx, -1, None, None, ctx,
                                        None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k = C.c_int()
    assert lib.spmvh_pcg(None, None, None, None, None, None, 10, 1e-8,
                         C.byref(k), None, None, 0, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_matrix_diagonal(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_jacobi_inverse(None, None, None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_pcg_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_pcg_workspace_reserve_timing(None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_pcg_workspace_destroy(None) == 0


def test_python_layer_has_the_entry_points():
    assert callable(host.pcg) and callable(host.jacobi_inverse)
    assert callable(host.Matrix.diagonal)
    assert callable(host.PcgWorkspace) and callable(host.PcgWorkspace.close)
    assert callable(host.PcgWorkspace.reserve_timing)
