"""CPU checks of spmv::gmres: the new symbols are declared in both headers,
exported and prototyped with the declared number of arguments, the change is
additive (ABI 5), NULL handles are refused before anything touches a device,
the argument rules raise their messages without a device, and the numpy
restatement of gmres_cases.py -- the reference of the GPU tests -- is itself
held to dense least squares."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blas1_cases as bc
import gmres_cases as gc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

HIP_NEW = tuple("spmv_hip_gmres_" + s for s in (
    "ws_create", "ws_destroy", "ws_reset", "ws_capacity", "ws_done_flag",
    "ws_array", "ws_read_async", "ws_set_state", "ws_get_state",
    "multi_dot_f64", "reduce", "multi_axpy_f64", "givens", "start",
    "scale_f64", "solve_y", "combine_f64", "add_f64", "residual_f64",
    "diag_f64"))
HOST_NEW = ("spmvh_gmres_workspace_create", "spmvh_gmres_workspace_destroy",
            "spmvh_gmres_workspace_reserve_timing",
            "spmvh_gmres_check_arguments", "spmvh_gmres")


def _declared_arity(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_gmres_symbols_declared_exported_prototyped():
    hip_decl = _declared_arity("spmv_hip.h")
    host_decl = _declared_arity("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert len(getattr(_lib.hip, n).argtypes) == hip_decl[n], n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert len(getattr(host.lib, n).argtypes) == host_decl[n], n
    assert hasattr(host, "gmres") and hasattr(host, "GmresWorkspace")


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)
    assert re.search(r"#define\s+SPMV_HIP_GMRES_MAX_RESTART\s+64\b", txt)
    assert re.search(r"#define\s+SPMV_HIP_GMRES_GROUP\s+8\b", txt)
    assert gc.MAX_RESTART == host.GMRES_MAX_RESTART == 64 and gc.GROUP == 8


def test_rules_are_stated_and_the_kernels_are_built():
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    for name in ("struct GmresPreconditioner", "class GmresWorkspace",
                 "int gmres(", '#include "solver_args.h"'):
        assert name in cg_h, name
    args_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host",
                               "solver_args.h")).read()
    assert "constexpr int kGmresMaxRestart = 64" in args_h
    # the plain-C++ rules stand alone: no other header of the mirror, and a
    # program of their own for the sanitizers
    assert re.findall(r'#include "([^"]+)"', args_h) == []
    assert os.path.exists(os.path.join(ROOT, "tools", "solver_args_check.cpp"))
    part = cg_h[cg_h.index("Restarted GMRES(m) from x0 = 0"):
                cg_h.index("int gmres(")]
    assert "poll_every and time_spmv apply" in part
    assert "consumer_reductions, defer_x and\n//          mixed are IGNORED" in part
    mk = open(os.path.join(ROOT, "spmv_amd", "csrc", "Makefile")).read()
    assert "hip/blas1_gmres.hip" in mk
    src = open(os.path.join(ROOT, "spmv_amd", "csrc", "hip",
                            "blas1_gmres.hip")).read()
    assert '#include "blas1_stream.h"' in src and "SPMV_LAUNCH_NT" in src


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    p, n, k = C.c_void_p(), C.c_int64(), C.c_int()
    assert h.spmv_hip_gmres_ws_create(None, 4, C.byref(p)) == EINVAL
    assert h.spmv_hip_gmres_ws_destroy(None) == 0
    assert h.spmv_hip_gmres_ws_reset(None, 0.0, 1, 1, None) == EINVAL
    assert h.spmv_hip_gmres_ws_capacity(None, C.byref(k)) == EINVAL
    assert h.spmv_hip_gmres_ws_done_flag(None, C.byref(p)) == EINVAL
    assert h.spmv_hip_gmres_ws_array(None, 0, C.byref(p), C.byref(n)) == EINVAL
    assert h.spmv_hip_gmres_ws_read_async(None, None, None, 0, None) == EINVAL
    assert h.spmv_hip_gmres_ws_set_state(None, 0, 0, 0, 0, None) == EINVAL
    assert h.spmv_hip_gmres_ws_get_state(None, None, None) == EINVAL
    # a context but no workspace: refused before the context is looked at -- the
    # block of memory standing in for it is never read
    ctx = C.create_string_buffer(4096)
    v = C.addressof(ctx) + 1024
    v -= v % 16
    for c in (None, ctx):
        assert h.spmv_hip_gmres_multi_dot_f64(c, None, 4, v, 4, 1, v,
                                              None) == EINVAL
        assert h.spmv_hip_gmres_reduce(c, None, 0, 1, None) == EINVAL
        assert h.spmv_hip_gmres_multi_axpy_f64(c, None, 0, 4, v, 4, 1, v,
                                               None) == EINVAL
        assert h.spmv_hip_gmres_givens(c, None, 0, 0, None) == EINVAL
        assert h.spmv_hip_gmres_start(c, None, 1, 0, None) == EINVAL
        assert h.spmv_hip_gmres_scale_f64(c, None, 4, v, v, None) == EINVAL
        assert h.spmv_hip_gmres_solve_y(c, None, None) == EINVAL
        assert h.spmv_hip_gmres_combine_f64(c, None, 4, v, 4, v, None) == EINVAL
        assert h.spmv_hip_gmres_add_f64(c, None, 4, v, v, None) == EINVAL
        assert h.spmv_hip_gmres_residual_f64(c, None, 4, v, None, v,
                                             None) == EINVAL
    assert h.spmv_hip_gmres_diag_f64(None, 4, v, v, v, None) == EINVAL
    assert h.spmv_hip_gmres_diag_f64(ctx, 4, None, v, v, None) == EINVAL
    assert h.spmv_hip_gmres_diag_f64(ctx, 4, v + 8, v, v, None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k = C.c_int()
    assert lib.spmvh_gmres(None, None, None, None, None, None, 0, 0.0, 0.0, None,
                           5, 10, 1e-8, C.byref(k), None, None, None, 0, None,
                           None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_gmres_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_gmres_workspace_reserve_timing(None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_gmres_workspace_destroy(None) == 0


@pytest.mark.parametrize("args, word", [
    ((0, 10, 0, 0.0, 0.0), b"restart"), ((65, 10, 0, 0.0, 0.0), b"restart"),
    ((-1, 10, 0, 0.0, 0.0), b"restart"), ((5, -1, 0, 0.0, 0.0), b"kmax"),
    ((5, 10, 17, 1.0, 2.0), b"degree"), ((5, 10, -1, 1.0, 2.0), b"degree"),
    ((5, 10, 4, 0.0, 2.0), b"bounds"), ((5, 10, 4, 2.0, 1.0), b"bounds"),
    ((5, 10, 4, 1.0, float("inf")), b"bounds"),
    ((5, 10, 4, float("nan"), 1.0), b"bounds")])
def test_argument_rules_need_no_device(args, word):
    assert host.lib.spmvh_gmres_check_arguments(*args) != 0
    assert word in host.lib.spmvh_last_error()


def test_argument_rules_accept_the_range():
    for m in (1, 30, 64):
        assert host.lib.spmvh_gmres_check_arguments(m, 0, 0, 0.0, 0.0) == 0
    assert host.lib.spmvh_gmres_check_arguments(5, 400, 16, 0.1, 3.0) == 0


# ---- the restatement -----------------------------------------------------------
def _dense12():
    rng = np.random.default_rng(12)
    A = rng.uniform(-1, 1, (12, 12)) + 4.0 * np.eye(12)
    return A, rng.uniform(-1, 1, 12)


def test_restatement_against_dense_least_squares():
    """Without restart (m >= k) the iterate after k steps minimises ||b - A x||
    over the Krylov space K_k(A, b): compare with lstsq on its power basis
    (orthonormalised), and the history with the true residual norms."""
    A, b = _dense12()
    spmv = lambda q: A @ q
    K = [b / np.linalg.norm(b)]
    for kmax in range(1, 9):
        x, k, hist, status = gc.gmres_ref(spmv, np.dot, None, b, 12, kmax, 0.0)
        assert (k, status, len(hist)) == (kmax, 0, kmax + 1)
        Q, _ = np.linalg.qr(np.array(K).T)
        c, *_ = np.linalg.lstsq(A @ Q, b, rcond=None)
        x_ls = Q @ c
        assert np.linalg.norm(x - x_ls) <= 1e-11 * np.linalg.norm(x_ls), kmax
        assert abs(hist[-1] - np.linalg.norm(b - A @ x)) <= 1e-12 * hist[0]
        K.append(A @ K[-1] / np.linalg.norm(A @ K[-1]))
    # all 12 dimensions: the lucky breakdown or the tolerance, x solves the system
    x, k, hist, status = gc.gmres_ref(spmv, np.dot, None, b, 12, 40, 1e-13)
    assert k <= 12 and np.linalg.norm(b - A @ x) <= 1e-11 * np.linalg.norm(b)
    # restarted, with a right preconditioner: converges, history = true residual
    dinv = 1.0 / np.diag(A)
    x, k, hist, status = gc.gmres_ref(spmv, np.dot, lambda q: dinv * q, b, 3, 200,
                                      1e-12)
    assert status == 0 and 3 < k < 200
    assert np.linalg.norm(b - A @ x) <= 1e-11 * np.linalg.norm(b)
    assert np.all(np.diff(hist) <= 1e-14 * hist[0])  # never grows


def test_restatement_edges():
    A, b = _dense12()
    spmv = lambda q: A @ q
    x, k, hist, st = gc.gmres_ref(spmv, np.dot, None, np.zeros(12), 5, 10, 1e-8)
    assert (k, st) == (0, 0) and np.all(x == 0) and list(hist) == [0.0]
    x, k, hist, st = gc.gmres_ref(spmv, np.dot, None, b, 5, 0, 1e-8)
    assert (k, st) == (0, 0) and np.all(x == 0) and len(hist) == 1
    # A = I: lucky breakdown at k = 1; x == b bit for bit where ||b|| is a power
    # of two and b / ||b|| is exact (16 entries of +-1: v_0.v_0 == 1.0)
    pm = np.where(np.arange(16) % 3 == 0, -1.0, 1.0)
    x, k, hist, st = gc.gmres_ref(lambda q: q.copy(), np.dot, None, pm, 5, 10,
                                  1e-8)
    assert (k, st) == (1, 1) and bc.same_bits(x, pm) and hist[1] == 0.0
    # A = diag(d), 3 distinct values, restart 64
    d = np.array([1.0, 2.0, 4.0] * 4)
    x, k, hist, st = gc.gmres_ref(lambda q: d * q, np.dot, None, b, 64, 50, 1e-12)
    assert k <= 4 and np.linalg.norm(d * x - b) <= 1e-11 * np.linalg.norm(b)
    # skew: converges where b.(A b) = 0 stops bicgstab
    S = gc.skew(12)
    sp = lambda q: gc.csr_spmv(S, q)
    assert np.dot(b, sp(b)) == pytest.approx(0.0, abs=1e-14)
    x, k, hist, st = gc.gmres_ref(sp, np.dot, None, b, 5, 100, 1e-10)
    assert st in (0, 1) and np.linalg.norm(b - sp(x)) <= 1e-9 * np.linalg.norm(b)


def test_givens_and_back_substitution_against_lstsq():
    rng = np.random.default_rng(5)
    for m in (1, 2, 5, 9, 30):
        # random upper Hessenberg with a dominant diagonal: its condition
        # number stays small, so 1e-12 is a bar on the arithmetic and not on
        # lstsq's own error
        H = np.triu(rng.uniform(-1, 1, (m + 1, m)), -1)
        H[np.arange(m), np.arange(m)] += 4.0 * rng.choice([-1.0, 1.0], m)
        beta = 1.7
        cs, sn, g, k = [], [], [beta], 0
        R = [[0.0] * m for _ in range(m)]
        for j in range(m):
            st = gc.gmres_givens(j, H[:j + 1, j], H[j + 1, j] ** 2, cs, sn, g,
                                 beta, k, 10 ** 6, 0.0)
            assert st["col"] is not None and not st["done"]
            assert st["inv"] == 1.0 / abs(H[j + 1, j]) or st["inv"] == \
                pytest.approx(1.0 / abs(H[j + 1, j]), rel=1e-15)
            for i in range(j + 1):
                R[i][j] = st["col"][i]
            cs, sn, g, k = st["cs"], st["sn"], st["g"], st["k"]
        y = np.array(gc.gmres_solve_y(R, g, m))
        # the sign of the subdiagonal does not matter to the kernel (hn = sqrt)
        Ha = H.copy()
        Ha[np.arange(1, m + 1), np.arange(m)] = np.abs(np.diag(H, -1))
        e1 = np.zeros(m + 1)
        e1[0] = beta
        y_ls, *_ = np.linalg.lstsq(Ha, e1, rcond=None)
        assert np.linalg.norm(y - y_ls) <= 1e-12 * max(1.0, np.linalg.norm(y_ls))
        assert abs(abs(g[m]) - np.linalg.norm(e1 - Ha @ y_ls)) <= 1e-12 * beta


def test_rotation_branches_and_stops():
    assert gc.rotation(3.0, 0.0) == (1.0, 0.0)
    c, s = gc.rotation(1.0, 2.0)      # |b| > |a|
    assert s == 1.0 / np.sqrt(1.25) and c == s * 0.5
    c, s = gc.rotation(2.0, 1.0)      # |a| >= |b|
    assert c == 1.0 / np.sqrt(1.25) and s == c * 0.5
    # R_jj == 0: a == b == 0 -> status 2, the column is discarded
    st = gc.gmres_givens(0, [0.0], 0.0, [], [], [1.0], 1.0, 0, 10, 0.0)
    assert st["status"] == 2 and st["done"] and st["jn"] == 0 and st["k"] == 0
    # hn == 0: lucky
    st = gc.gmres_givens(0, [2.0], 0.0, [], [], [1.0], 1.0, 0, 10, 0.0)
    assert (st["status"], st["done"], st["k"], st["res"]) == (1, True, 1, 0.0)
    # rtol, kmax
    st = gc.gmres_givens(0, [2.0], 1.0, [], [], [1.0], 1.0, 0, 10, 0.9)
    assert st["status"] == 0 and st["done"] and st["inv"] is None
    st = gc.gmres_givens(0, [2.0], 1.0, [], [], [1.0], 1.0, 9, 10, 0.0)
    assert st["done"] and st["k"] == 10
    st = gc.gmres_givens(0, [2.0], 1.0, [], [], [1.0], 1.0, 0, 10, 0.0)
    assert not st["done"] and st["inv"] == 1.0


def test_vector_references_and_matrices():
    n = 37
    V = [bc.exact_vec(n, s) for s in range(3)]
    w = bc.exact_vec(n, 9)
    got = gc.gmres_multi_axpy(V, [2.0, -1.0, 4.0], w)
    assert bc.same_bits(got, w - 2 * V[0] + V[1] - 4 * V[2])
    assert bc.same_bits(gc.gmres_combine(V, [2.0, -1.0, 4.0]),
                        2 * V[0] - V[1] + 4 * V[2])
    assert bc.same_bits(gc.gmres_scale(0.5, w), w / 2)
    assert bc.same_bits(gc.gmres_residual(w), w)
    assert bc.same_bits(gc.gmres_residual(w, V[0]), w - V[0])
    for name, rows in (("convdiff11", 1331), ("banded4097", 4097),
                       ("skew1330", 1330), ("poisson11", 1331)):
        rp, ci, va = gc.csr_by_name(name)
        assert len(rp) == rows + 1 and rp[-1] == len(ci) == len(va)
    rp, ci, va = gc.skew(8)
    D = np.zeros((8, 8))
    D[gc.row_of(rp), ci] = va
    assert np.array_equal(D, -D.T) and D[0, 1] == 1.5
    # the Poisson matrix gets two colours, the parity of x + y + z
    P = gc.poisson(4)
    col = gc.sgs_color(P)
    i = np.arange(64)
    assert np.array_equal(col, (i % 4 + i // 4 % 4 + i // 16) % 2)
    # SGS restated: M z = r with M = (D + L) D^-1 (D + U) in the colour order
    M = gc.SgsRef(P)
    r = bc.round_vec(64, 1)
    z = M(r)
    Dm = np.zeros((64, 64))
    Dm[gc.row_of(P[0]), P[1]] = P[2]
    before = col[:, None] > col[None, :]
    Lo, Up, Dg = Dm * before, Dm * before.T, np.diag(np.diag(Dm))
    Mm = (Dg + Lo) @ np.linalg.inv(Dg) @ (Dg + Up)
    assert np.linalg.norm(Mm @ z - r) <= 1e-12 * np.linalg.norm(r)
