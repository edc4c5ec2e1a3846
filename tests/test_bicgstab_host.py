"""CPU checks of the interface of spmv::bicgstab (BiCGStab with an optional
diagonal right preconditioner): the new symbols are declared in both headers,
exported and prototyped with the declared number of arguments, the change is
additive (ABI 5), NULL handles and iteration indices are refused before
anything touches a device, cg.h states the rules, and the Python layer has the
entry points."""
import ctypes as C
import os
import re

from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_bicg_ws_create", "spmv_hip_bicg_ws_destroy",
           "spmv_hip_bicg_ws_reset", "spmv_hip_bicg_ws_capacity",
           "spmv_hip_bicg_ws_rv", "spmv_hip_bicg_ws_ts_tt",
           "spmv_hip_bicg_ws_rr_rho", "spmv_hip_bicg_ws_done_flag",
           "spmv_hip_bicg_ws_read_async", "spmv_hip_bicg_init_f64",
           "spmv_hip_bicg_dot_rv_f64", "spmv_hip_bicg_dot_ts_tt_f64",
           "spmv_hip_bicg_update_s_f64", "spmv_hip_bicg_update_xr_f64",
           "spmv_hip_bicg_update_p_f64", "spmv_hip_bicg_reduce_rv",
           "spmv_hip_bicg_reduce_ts_tt", "spmv_hip_bicg_reduce_rr_rho",
           "spmv_hip_bicg_update_s_cs_f64", "spmv_hip_bicg_update_xr_cs_f64",
           "spmv_hip_bicg_update_p_cs_f64")
HOST_NEW = ("spmvh_bicgstab_workspace_create",
            "spmvh_bicgstab_workspace_destroy",
            "spmvh_bicgstab_workspace_reserve_timing", "spmvh_bicgstab")
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


def test_bicgstab_symbols_declared_exported_prototyped():
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
    assert "int bicgstab(" in cg_h and "BicgstabWorkspace" in cg_h
    at = cg_h.index("BiCGStab from x0 = 0")
    rules = cg_h[at:cg_h.index("int bicgstab(")]
    # which options apply, which are ignored, the zero right-hand side, the
    # two breakdowns, the overlap rule and the status
    assert "defer_x and mixed are IGNORED" in rules
    assert "consumer_reductions apply" in rules and "poll_every" in rules
    assert "r_0 . r_0 == 0 stops at k = 0" in rules
    assert "breakdown 1" in rules and "breakdown 2" in rules
    assert "rv == 0" in rules and "omega == 0 or rho[k] == 0" in rules
    assert '"overlaps"' in rules and "kmax < 0 throws" in rules
    assert "no half-step exit" in rules
    assert "int* status = nullptr" in cg_h
    hip_h = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert "{ts[k], tt[k]}" in hip_h and "{rr[k], rho[k]}" in hip_h
    assert "each\n *   pair ADJACENT" in hip_h


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    out = C.c_void_p()
    k = C.c_int()
    assert h.spmv_hip_bicg_ws_create(None, 10, C.byref(out)) == EINVAL
    assert out.value is None
    assert h.spmv_hip_bicg_ws_destroy(None) == 0  # like free(NULL)
    assert h.spmv_hip_bicg_ws_reset(None, 1e-8, None) == EINVAL
    assert h.spmv_hip_bicg_ws_capacity(None, C.byref(k)) == EINVAL
    assert h.spmv_hip_bicg_ws_rv(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_ws_ts_tt(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_ws_rr_rho(None, 0, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_ws_done_flag(None, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_ws_read_async(None, None, None, 0, None) == EINVAL
    assert h.spmv_hip_bicg_init_f64(None, None, 4, None, None, None, None, None,
                                    None, None, None) == EINVAL
    assert h.spmv_hip_bicg_dot_rv_f64(None, None, 1, 4, None, None,
                                      None) == EINVAL
    assert h.spmv_hip_bicg_dot_ts_tt_f64(None, None, 1, 4, None, None,
                                         None) == EINVAL
    assert h.spmv_hip_bicg_reduce_rv(None, None, 1, None) == EINVAL
    assert h.spmv_hip_bicg_reduce_ts_tt(None, None, 1, None) == EINVAL
    assert h.spmv_hip_bicg_reduce_rr_rho(None, None, 0, None) == EINVAL
    for name in ("spmv_hip_bicg_update_s", "spmv_hip_bicg_update_p"):
        for form in ("_f64", "_cs_f64"):
            assert getattr(h, name + form)(None, None, 1, 4, None, None, None,
                                           None, None, None) == EINVAL
    for form in ("_f64", "_cs_f64"):
        assert getattr(h, "spmv_hip_bicg_update_xr" + form)(
            None, None, 1, 4, None, None, None, None, None, None, None,
            None) == EINVAL
    # a context but no workspace (or bad sizes): refused before the context is
    # looked at -- the block of memory standing in for it is never read
    ctx = C.create_string_buffer(4096)
    assert h.spmv_hip_bicg_ws_create(ctx, -1, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_ws_create(ctx, 10, None) == EINVAL
    assert h.spmv_hip_bicg_init_f64(ctx, None, 4, None, None, None, None, None,
                                    None, None, None) == EINVAL
    assert h.spmv_hip_bicg_dot_rv_f64(ctx, None, 1, 4, None, None,
                                      None) == EINVAL
    assert h.spmv_hip_bicg_dot_ts_tt_f64(ctx, None, 1, 4, None, None,
                                         None) == EINVAL
    assert h.spmv_hip_bicg_reduce_rv(ctx, None, 1, None) == EINVAL
    assert h.spmv_hip_bicg_reduce_rr_rho(ctx, None, 0, None) == EINVAL
    assert h.spmv_hip_bicg_update_s_cs_f64(ctx, None, 1, 4, None, None, None,
                                           None, None, None) == EINVAL
    assert h.spmv_hip_bicg_update_p_f64(ctx, None, 1, 4, None, None, None,
                                        None, None, None) == EINVAL


def test_iteration_indices_refused_without_a_device():
    """The range check of k reads only the workspace's own two leading fields
    {ctx, kmax}; a stand-in with those is refused for k outside 1..kmax (0..kmax
    for the slots and reduce_rr_rho) before the context is looked at."""
    h = _lib.hip
    ctx = C.create_string_buffer(4096)

    class Head(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("kmax", C.c_int)]

    buf = C.create_string_buffer(256)
    head = Head.from_buffer(buf)
    head.ctx, head.kmax = C.addressof(ctx), 5
    ws = C.cast(buf, C.c_void_p)
    out = C.c_void_p()
    for slot in (h.spmv_hip_bicg_ws_rv, h.spmv_hip_bicg_ws_ts_tt,
                 h.spmv_hip_bicg_ws_rr_rho):
        assert slot(ws, -1, C.byref(out)) == EINVAL
        assert slot(ws, 6, C.byref(out)) == EINVAL
    assert h.spmv_hip_bicg_reduce_rr_rho(ctx, ws, -1, None) == EINVAL
    assert h.spmv_hip_bicg_reduce_rr_rho(ctx, ws, 6, None) == EINVAL
    for k in (0, 6, -3):
        assert h.spmv_hip_bicg_reduce_rv(ctx, ws, k, None) == EINVAL
        assert h.spmv_hip_bicg_reduce_ts_tt(ctx, ws, k, None) == EINVAL
        assert h.spmv_hip_bicg_dot_rv_f64(ctx, ws, k, 4, None, None,
                                          None) == EINVAL
        assert h.spmv_hip_bicg_dot_ts_tt_f64(ctx, ws, k, 4, None, None,
                                             None) == EINVAL
        assert h.spmv_hip_bicg_update_s_f64(ctx, ws, k, 4, None, None, None,
                                            None, None, None) == EINVAL
        assert h.spmv_hip_bicg_update_xr_cs_f64(ctx, ws, k, 4, None, None, None,
                                                None, None, None, None,
                                                None) == EINVAL
        assert h.spmv_hip_bicg_update_p_cs_f64(ctx, ws, k, 4, None, None, None,
                                               None, None, None) == EINVAL
    # in range but without vectors, or with a vector off 16 bytes: refused too
    assert h.spmv_hip_bicg_dot_rv_f64(ctx, ws, 1, 4, None, None, None) == EINVAL
    assert h.spmv_hip_bicg_dot_rv_f64(ctx, ws, 1, 4, C.c_void_p(4096 + 8),
                                      C.c_void_p(4096), None) == EINVAL
    # another context's workspace
    other = C.create_string_buffer(64)
    assert h.spmv_hip_bicg_reduce_rv(other, ws, 1, None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k, st = C.c_int(), C.c_int()
    assert lib.spmvh_bicgstab(None, None, None, None, None, None, 10, 1e-8,
                              C.byref(k), C.byref(st), None, None, 0, None,
                              None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_bicgstab_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_bicgstab_workspace_reserve_timing(None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_bicgstab_workspace_destroy(None) == 0


def test_python_layer_has_the_entry_points():
    assert callable(host.bicgstab)
    assert callable(host.BicgstabWorkspace)
    assert callable(host.BicgstabWorkspace.close)
    assert callable(host.BicgstabWorkspace.reserve_timing)
