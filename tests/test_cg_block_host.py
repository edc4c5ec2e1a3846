"""CPU checks of the interface of spmv::cg_block (CG for a block of right-hand
sides): the new symbols are declared in both headers, exported and prototyped,
the change is additive (ABI 5), NULL handles and nrhs outside 1..8 are refused
before anything touches a device, and the Python layer has the entry points."""
import ctypes as C
import os
import re

from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_cgb_ws_create", "spmv_hip_cgb_ws_destroy",
           "spmv_hip_cgb_ws_reset", "spmv_hip_cgb_ws_capacity",
           "spmv_hip_cgb_ws_rr", "spmv_hip_cgb_ws_pAp",
           "spmv_hip_cgb_ws_partials", "spmv_hip_cgb_ws_done_flag",
           "spmv_hip_cgb_ws_read_async", "spmv_hip_cgb_init_f64",
           "spmv_hip_cgb_dot_f64", "spmv_hip_cgb_reduce_pAp",
           "spmv_hip_cgb_reduce_rr", "spmv_hip_cgb_update_r_f64",
           "spmv_hip_cgb_update_xp_f64")
HOST_NEW = ("spmvh_cg_block", "spmvh_cg_block_workspace_create",
            "spmvh_cg_block_workspace_destroy")
EINVAL = -1


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(\w+)\s*\(", txt))


def test_cg_block_symbols_declared_exported_prototyped():
    hip_decl, host_decl = _declared("spmv_hip.h"), _declared("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert getattr(_lib.hip, n).argtypes is not None, n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert getattr(host.lib, n).argtypes is not None, n


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)
    assert re.search(r"#define\s+SPMV_HIP_CGB_MAX_NRHS\s+8\b", txt)


def test_layout_and_zero_column_rule_are_stated():
    hip_h = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert "V[i * nrhs + c]" in hip_h
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    assert "cg_block" in cg_h and "CgBlockWorkspace" in cg_h
    # cg.h says how a zero column differs from cg(), and which options are
    # ignored
    assert "r_0 . r_0 == 0" in cg_h and "IGNORED" in cg_h


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    out = C.c_void_p()
    k, n = C.c_int(), C.c_int()
    assert h.spmv_hip_cgb_ws_create(None, 10, 4, C.byref(out)) == EINVAL
    assert out.value is None
    assert h.spmv_hip_cgb_ws_destroy(None) == 0  # like free(NULL)
    assert h.spmv_hip_cgb_ws_reset(None, 1e-8, None) == EINVAL
    assert h.spmv_hip_cgb_ws_capacity(None, C.byref(k), C.byref(n)) == EINVAL
    assert h.spmv_hip_cgb_ws_rr(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_cgb_ws_pAp(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_cgb_ws_partials(None, C.byref(out)) == EINVAL
    assert h.spmv_hip_cgb_ws_done_flag(None, C.byref(out)) == EINVAL
    assert h.spmv_hip_cgb_ws_read_async(None, None, 0, None, 0, None) == EINVAL
    assert h.spmv_hip_cgb_init_f64(None, None, 4, None, None, None, None,
                                   None) == EINVAL
    assert h.spmv_hip_cgb_dot_f64(None, None, 4, None, None, None) == EINVAL
    assert h.spmv_hip_cgb_reduce_pAp(None, None, 1, None) == EINVAL
    assert h.spmv_hip_cgb_reduce_rr(None, None, 0, None) == EINVAL
    assert h.spmv_hip_cgb_update_r_f64(None, None, 1, 4, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_cgb_update_xp_f64(None, None, 1, 4, None, None, None,
                                        None) == EINVAL
    # a context but no workspace: refused before the context is looked at
    ctx = C.create_string_buffer(4096)
    assert h.spmv_hip_cgb_dot_f64(ctx, None, 4, None, None, None) == EINVAL
    assert h.spmv_hip_cgb_reduce_pAp(ctx, None, 1, None) == EINVAL


def test_bad_nrhs_refused_without_a_device():
    """nrhs in {0, 9} (and a negative one) is SPMV_HIP_EINVAL before the
    context is dereferenced: the block of memory standing in for it is never
    read."""
    h = _lib.hip
    ctx = C.create_string_buffer(4096)
    for nrhs in (0, 9, -1):
        out = C.c_void_p()
        assert h.spmv_hip_cgb_ws_create(ctx, 10, nrhs, C.byref(out)) == EINVAL
        assert out.value is None
    out = C.c_void_p()
    assert h.spmv_hip_cgb_ws_create(ctx, -1, 4, C.byref(out)) == EINVAL
    assert h.spmv_hip_cgb_ws_create(ctx, 10, 4, None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k = C.c_int()
    its = (C.c_int * 8)()
    assert lib.spmvh_cg_block(None, None, None, None, None, 4, 10, 1e-8,
                              C.byref(k), its, None, None, 0, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_cg_block_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_cg_block_workspace_destroy(None) == 0


def test_python_layer_has_the_entry_points():
    assert callable(host.cg_block)
    assert callable(host.CgBlockWorkspace) and callable(host.CgBlockWorkspace.close)
