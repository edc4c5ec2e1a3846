"""CPU checks of spmv::pcg_block and spmv::sgs_apply_block: the interface is
additive (ABI 5, the new symbols declared, exported and prototyped), every
argument rule raises with its word before anything touches a device, the numpy
restatement of the block recurrence (pcg_block_cases.block_ref) equals
test_gpu_chebyshev._pcg_ref column by column, and the references of every case
test_gpu_pcg_block.py holds to the 1e-6 history bar agree with themselves to a
tenth of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import pcg_block_cases as pc
import test_gpu_chebyshev as tc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_mcgs_apply_block_f64", "spmv_hip_pcgb_ws_create",
           "spmv_hip_pcgb_ws_destroy", "spmv_hip_pcgb_ws_reset",
           "spmv_hip_pcgb_ws_capacity", "spmv_hip_pcgb_ws_rz_rr",
           "spmv_hip_pcgb_ws_pAp", "spmv_hip_pcgb_ws_read_async",
           "spmv_hip_pcgb_init_f64", "spmv_hip_pcgb_dot_pAp_f64",
           "spmv_hip_pcgb_dot_rz_f64", "spmv_hip_pcgb_reduce_pAp",
           "spmv_hip_pcgb_reduce_rz_rr", "spmv_hip_pcgb_update_r_f64",
           "spmv_hip_pcgb_update_xp_f64")
HOST_NEW = ("spmvh_sgs_apply_block", "spmvh_pcg_block",
            "spmvh_pcg_block_workspace_create",
            "spmvh_pcg_block_workspace_destroy",
            "spmvh_pcg_block_check_arguments")
EINVAL = -1


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(\w+)\s*\(", txt))


# ---- 1. the interface ---------------------------------------------------------------
def test_abi_is_still_5_and_the_symbols_are_exported():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)
    hip_decl, host_decl = _declared("spmv_hip.h"), _declared("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert getattr(_lib.hip, n).argtypes is not None, n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert getattr(host.lib, n).argtypes is not None, n
    assert callable(host.sgs_apply_block) and callable(host.pcg_block)
    assert callable(host.PcgBlockWorkspace) and callable(host.PcgBlockWorkspace.close)


def test_null_handles_and_bad_nrhs_refused_without_a_device():
    h, lib = _lib.hip, host.lib
    out = C.c_void_p()
    ctx = C.create_string_buffer(4096)  # stands in for a context: never read
    for nrhs in (0, 9, -1):
        assert h.spmv_hip_pcgb_ws_create(ctx, 10, nrhs, C.byref(out)) == EINVAL
        assert out.value is None
        assert h.spmv_hip_mcgs_apply_block_f64(ctx, ctx, None, None, None, nrhs,
                                               None) == EINVAL
    assert h.spmv_hip_pcgb_ws_create(ctx, -1, 4, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcgb_ws_create(None, 10, 4, C.byref(out)) == EINVAL
    assert h.spmv_hip_pcgb_ws_destroy(None) == 0  # like free(NULL)
    assert h.spmv_hip_pcgb_ws_reset(None, 1e-8, None) == EINVAL
    assert h.spmv_hip_pcgb_ws_read_async(None, None, 0, None, 0, None) == EINVAL
    assert h.spmv_hip_mcgs_apply_block_f64(None, None, None, None, None, 4,
                                           None) == EINVAL
    assert h.spmv_hip_pcgb_dot_rz_f64(ctx, None, 4, None, None, None,
                                      None) == EINVAL
    assert h.spmv_hip_pcgb_reduce_pAp(ctx, None, 1, None) == EINVAL
    k = C.c_int()
    its = (C.c_int * 8)()
    assert lib.spmvh_pcg_block(None, None, None, None, None, 4, None, None, 10,
                               1e-8, C.byref(k), its, None, None, 0, None,
                               None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_apply_block(None, None, None, None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_pcg_block_workspace_create(None, None) != 0
    assert lib.spmvh_pcg_block_workspace_destroy(None) == 0


# ---- 2. the argument rules ------------------------------------------------------------
ROWS = 100
_BUF = np.zeros(ROWS * 8 * 3 + ROWS)  # host memory: the rules compare addresses only
_B = _BUF.ctypes.data
_X = _B + 8 * ROWS * 8
_DINV = _B + 8 * ROWS * 16


def _check(nrhs=4, kmax=10, has_dinv=1, has_sgs=0, sgs_rows=ROWS, negative=0,
           rows=ROWS, B=_B, X=_X, dinv=_DINV):
    rc = host.lib.spmvh_pcg_block_check_arguments(nrhs, kmax, has_dinv, has_sgs,
                                                  sgs_rows, negative, rows, B, X,
                                                  dinv)
    return rc, host.lib.spmvh_last_error().decode()


@pytest.mark.parametrize("word,kw", [
    ("nrhs", dict(nrhs=0)), ("nrhs", dict(nrhs=9)), ("nrhs", dict(nrhs=-3)),
    ("kmax", dict(kmax=-1)),
    ("preconditioner", dict(has_dinv=1, has_sgs=1)),
    ("preconditioner", dict(has_dinv=0, has_sgs=0)),
    ("rows", dict(has_dinv=0, has_sgs=1, sgs_rows=ROWS + 1)),
    ("pivot", dict(has_dinv=0, has_sgs=1, negative=2)),
    ("overlaps", dict(X=_B)),
    ("overlaps", dict(X=_B + 8 * (ROWS * 4 - 1))),   # the last double of B
    ("overlaps", dict(X=_B - 8 * (ROWS * 4 - 1))),   # the first double of B
    ("overlaps", dict(X=_DINV)),
    ("overlaps", dict(X=_DINV + 8 * (ROWS - 1))),
    ("overlaps", dict(X=_DINV - 8 * (ROWS * 4 - 1))),
])
def test_every_rule_raises_with_its_word(word, kw):
    rc, msg = _check(**kw)
    assert rc != 0 and word in msg, (kw, msg)


def test_the_rules_accept_what_they_should():
    for nrhs in (1, 2, 3, 8):
        assert _check(nrhs=nrhs)[0] == 0
    assert _check(kmax=0)[0] == 0
    assert _check(has_dinv=0, has_sgs=1)[0] == 0
    # X next to B and next to dinv, not sharing a byte
    assert _check(X=_B + 8 * ROWS * 4)[0] == 0
    assert _check(X=_DINV + 8 * ROWS)[0] == 0
    assert _check(X=_DINV - 8 * ROWS * 4)[0] == 0
    # an SGS preconditioner: what dinv points at does not matter
    assert _check(has_dinv=0, has_sgs=1, X=_DINV)[0] == 0
    # the rules come in the stated order
    assert "nrhs" in _check(nrhs=0, kmax=-1)[1]
    assert "kmax" in _check(kmax=-1, has_dinv=0)[1]


# ---- 3. the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_block_ref_equals_pcg_ref_per_column(shape, kind):
    """Columns that stop at different k (the zero column at 0), in lockstep:
    each equals _pcg_ref on that column alone -- same k, same bits."""
    P = pc.case(shape)
    names = ["rand0", "zero", "eig" if P.n_grid else "rand1", "ones"]
    M = P.precond(kind)
    its, hist, X = pc.block_ref(P.spmv, oracle.ddot, P.block(names), M, pc.KMAX,
                                pc.RTOL)
    # (the banded matrix takes every non-zero column to the same k)
    assert len(set(its.tolist())) >= (3 if P.n_grid else 2), its
    for c, col in enumerate(names):
        x, k, h = tc._pcg_ref(P.spmv, oracle.ddot, P.cols[col], M, pc.KMAX,
                              pc.RTOL)
        assert its[c] == k, (shape, kind, col)
        assert np.array_equal(hist[c, :k + 1], h), (shape, kind, col)
        assert np.all(hist[c, k + 1:] == -1.0), (shape, kind, col)
        assert np.array_equal(X[:, c], x), (shape, kind, col)
    assert its[1] == 0 and hist[1, 0] == 0.0 and np.all(X[:, 1] == 0.0)
    # cut at kmax = 3, rtol = 0: three steps of every column but the zero one
    its, hist, X = pc.block_ref(P.spmv, oracle.ddot, P.block(names), M, 3, 0.0)
    assert its.tolist() == [3, 0, 3, 3]
    x, k, h = tc._pcg_ref(P.spmv, oracle.ddot, P.cols["ones"], M, 3, 0.0)
    assert np.array_equal(X[:, 3], x) and np.array_equal(hist[3], h)


# ---- 4. the references agree with themselves ------------------------------------------------
def test_dev_ref_of_every_gpu_case_is_a_tenth_of_the_bar():
    """dev_ref: the deviation of the restatement between oracle.ddot and the
    chunked pairwise sum over the history entries _vs_ref compares.  Above 1e-7
    _vs_ref would widen its 1e-6 bar; no case of the GPU tests may be there."""
    worst, at = 0.0, None
    for shape, kind, col in pc.gpu_cases():
        d = pc.case(shape).dev_ref(kind, col)
        if d > worst:
            worst, at = d, (shape, kind, col)
    for world in (2, 3):  # the references of the test with ranks as threads
        d = max(pc.slab_case(world).dev_refs())
        if d > worst:
            worst, at = d, ("slabs", world)
    print("largest dev_ref", worst, at)
    assert worst <= 1e-7, (worst, at)
