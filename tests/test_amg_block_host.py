"""CPU checks of spmv::amg_apply_block and of pcg_block with an
AmgPreconditioner: the interface is additive (ABI 5, the new symbols declared,
exported and prototyped), every argument rule raises with its word before
anything touches a device, the block restatement (pcg_block_cases.block_ref
with amg_cases.AmgRef.apply per column) equals the single-vector PCG
restatement column by column, and the references of every column
test_gpu_pcg_block_amg.py holds to the 1e-6 history bar agree with themselves
between two summation orders to a tenth of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_block_cases as abc
import oracle
import pcg_block_cases as pc
import test_gpu_chebyshev as tc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_cheb_apply0_block_f64", "spmv_hip_cheb_step_block_f64",
           "spmv_hip_amg_post0_block_f64", "spmv_hip_amg_restrict_block_f64",
           "spmv_hip_amg_prolong_block_f64")
HOST_NEW = ("spmvh_amg_apply_block", "spmvh_amg_apply_block_check_arguments",
            "spmvh_amg_release_block_scratch", "spmvh_pcg_block_amg",
            "spmvh_pcg_block_amg_check_arguments")
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
    assert callable(host.amg_apply_block)
    assert callable(host.AmgPreconditioner.release_block_scratch)
    import inspect
    assert "amg" in inspect.signature(host.pcg_block).parameters


def test_the_existing_entry_points_keep_their_signatures():
    """additive: spmvh_pcg_block and its rule function as they were"""
    assert len(host.lib.spmvh_pcg_block.argtypes) == 17
    assert len(host.lib.spmvh_pcg_block_check_arguments.argtypes) == 10
    assert len(host.lib.spmvh_pcg_block_amg.argtypes) == 16


def test_null_handles_and_bad_nrhs_refused_without_a_device():
    h, lib = _lib.hip, host.lib
    ctx = C.create_string_buffer(4096)  # stands in for a context: never read
    for nrhs in (0, 9, -1):
        assert h.spmv_hip_cheb_apply0_block_f64(ctx, 4, nrhs, 1.0, ctx, ctx, ctx,
                                                ctx, None) == EINVAL
        assert h.spmv_hip_cheb_step_block_f64(ctx, 4, nrhs, 1.0, 1.0, 0, ctx, ctx,
                                              ctx, ctx, ctx, None) == EINVAL
        assert h.spmv_hip_amg_post0_block_f64(ctx, 4, nrhs, 1.0, ctx, ctx, ctx,
                                              ctx, ctx, None) == EINVAL
    assert h.spmv_hip_cheb_apply0_block_f64(None, 4, 4, 1.0, ctx, ctx, ctx, ctx,
                                            None) == EINVAL
    assert h.spmv_hip_amg_restrict_block_f64(ctx, None, 4, ctx, ctx, ctx,
                                             None) == EINVAL
    assert h.spmv_hip_amg_prolong_block_f64(ctx, None, 4, 1.0, ctx, ctx,
                                            None) == EINVAL
    assert lib.spmvh_amg_apply_block(None, None, None, None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_amg_release_block_scratch(None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    k = C.c_int()
    its = (C.c_int * 8)()
    assert lib.spmvh_pcg_block_amg(None, None, None, None, None, 4, None, 10,
                                   1e-8, C.byref(k), its, None, None, 0, None,
                                   None) != 0
    assert b"NULL" in lib.spmvh_last_error()


# ---- 2. the argument rules ------------------------------------------------------------
ROWS = 100
_BUF = np.zeros(ROWS * 8 * 3 + ROWS)  # host memory: the rules compare addresses only
_B = _BUF.ctypes.data
_X = _B + 8 * ROWS * 8
_DINV = _B + 8 * ROWS * 16


def _apply_check(nrhs=4, rows=ROWS, R=_B, Z=_X):
    rc = host.lib.spmvh_amg_apply_block_check_arguments(nrhs, rows, R, Z)
    return rc, host.lib.spmvh_last_error().decode()


@pytest.mark.parametrize("word,kw", [
    ("nrhs", dict(nrhs=0)), ("nrhs", dict(nrhs=9)), ("nrhs", dict(nrhs=-3)),
    ("overlaps", dict(Z=_B)),
    ("overlaps", dict(Z=_B + 8 * (ROWS * 4 - 1))),   # the last double of R
    ("overlaps", dict(Z=_B - 8 * (ROWS * 4 - 1))),   # the first double of R
])
def test_amg_apply_block_rules(word, kw):
    rc, msg = _apply_check(**kw)
    assert rc != 0 and word in msg, (kw, msg)


def test_amg_apply_block_accepts_what_it_should():
    for nrhs in range(1, 9):
        assert _apply_check(nrhs=nrhs)[0] == 0
    assert _apply_check(Z=_B + 8 * ROWS * 4)[0] == 0      # side by side
    assert _apply_check(Z=_B - 8 * ROWS * 4)[0] == 0
    assert _apply_check(Z=_B + 8, rows=0)[0] == 0         # nothing to share
    assert "nrhs" in _apply_check(nrhs=0, Z=_B)[1]        # the stated order


def _check(nrhs=4, kmax=10, has_dinv=0, has_sgs=0, has_amg=1, sgs_rows=ROWS,
           negative=0, amg_rows=ROWS, rows=ROWS, B=_B, X=_X, dinv=_DINV):
    rc = host.lib.spmvh_pcg_block_amg_check_arguments(
        nrhs, kmax, has_dinv, has_sgs, has_amg, sgs_rows, negative, amg_rows,
        rows, B, X, dinv)
    return rc, host.lib.spmvh_last_error().decode()


@pytest.mark.parametrize("word,kw", [
    ("nrhs", dict(nrhs=0)), ("nrhs", dict(nrhs=9)),
    ("kmax", dict(kmax=-1)),
    ("preconditioner", dict(has_dinv=1, has_sgs=1, has_amg=0)),
    ("preconditioner", dict(has_dinv=1, has_sgs=0, has_amg=1)),
    ("preconditioner", dict(has_dinv=0, has_sgs=1, has_amg=1)),
    ("preconditioner", dict(has_dinv=1, has_sgs=1, has_amg=1)),
    ("preconditioner", dict(has_dinv=0, has_sgs=0, has_amg=0)),
    ("rows", dict(amg_rows=ROWS + 1)),
    ("rows", dict(amg_rows=ROWS - 1)),
    ("rows", dict(has_amg=0, has_sgs=1, sgs_rows=ROWS + 1)),
    ("pivot", dict(has_amg=0, has_sgs=1, negative=2)),
    ("overlaps", dict(X=_B)),
    ("overlaps", dict(X=_B + 8 * (ROWS * 4 - 1))),
    ("overlaps", dict(has_amg=0, has_dinv=1, X=_DINV)),
])
def test_every_pcg_block_rule_raises_with_its_word(word, kw):
    rc, msg = _check(**kw)
    assert rc != 0 and word in msg, (kw, msg)


def test_the_pcg_block_rules_accept_what_they_should():
    for nrhs in (1, 2, 3, 8):
        assert _check(nrhs=nrhs)[0] == 0
    assert _check(kmax=0)[0] == 0
    assert _check(has_amg=0, has_dinv=1)[0] == 0
    assert _check(has_amg=0, has_sgs=1)[0] == 0
    assert _check(X=_DINV)[0] == 0  # amg: what dinv points at does not matter
    assert _check(sgs_rows=ROWS + 1)[0] == 0  # ... nor the SGS fields
    assert "nrhs" in _check(nrhs=0, kmax=-1)[1]
    assert "kmax" in _check(kmax=-1, has_amg=0)[1]
    assert "preconditioner" in _check(has_dinv=1, amg_rows=ROWS + 1)[1]
    # the existing entry point is the overload without the third one
    lib = host.lib
    assert lib.spmvh_pcg_block_check_arguments(4, 10, 1, 0, ROWS, 0, ROWS, _B, _X,
                                               _DINV) == 0
    assert lib.spmvh_pcg_block_check_arguments(4, 10, 0, 0, ROWS, 0, ROWS, _B, _X,
                                               _DINV) != 0
    assert b"preconditioner" in lib.spmvh_last_error()


def test_python_refuses_two_preconditioners_without_a_device():
    class Handle:
        h = None
    with pytest.raises(host.SpmvHostError, match="preconditioner"):
        host.pcg_block(Handle, Handle, Handle, None, None, 4, 10, 1e-8,
                       dinv=_DINV, amg=Handle)
    with pytest.raises(host.SpmvHostError, match="preconditioner"):
        host.pcg_block(Handle, Handle, Handle, None, None, 4, 10, 1e-8,
                       sgs=Handle, amg=Handle)


# ---- 3. the restatement -----------------------------------------------------------------
def test_block_ref_with_amg_equals_pcg_ref_per_column():
    """Columns that stop at different k (the zero column at 0), in lockstep,
    the V-cycle restated per column: each equals _pcg_ref with AmgRef.apply on
    that column alone -- same k, same bits."""
    P = abc.case("poisson11")
    names = ["rand0", "zero", "eig", "ones"]
    its, hist, X = pc.block_ref(P.spmv, oracle.ddot, P.block(names), P.precond,
                                abc.KMAX, abc.RTOL)
    assert len(set(its.tolist())) >= 3, its
    for c, col in enumerate(names):
        x, k, h = tc._pcg_ref(P.spmv, oracle.ddot, P.cols[col], P.precond,
                              abc.KMAX, abc.RTOL)
        assert its[c] == k, col
        assert np.array_equal(hist[c, :k + 1], h), col
        assert np.all(hist[c, k + 1:] == -1.0), col
        assert np.array_equal(X[:, c], x), col
    assert its[1] == 0 and hist[1, 0] == 0.0 and np.all(X[:, 1] == 0.0)
    # the cycle of a block is the cycle of its columns: AmgRef.apply per column
    R = P.block(["rand0", "ones", "rand1"])
    Z = np.stack([P.precond(R[:, c]) for c in range(3)], axis=1)
    assert np.array_equal(Z[:, 1], P.amg.apply(P.cols["ones"]))


# ---- 4. the references agree with themselves ------------------------------------------------
def test_dev_ref_of_every_gpu_column_is_a_tenth_of_the_bar():
    """dev_ref: the deviation of the restatement between oracle.ddot and the
    chunked pairwise sum over the history entries _vs_ref compares.  Above 1e-7
    _vs_ref would widen its 1e-6 bar; no column of the GPU tests may be there
    (a column that is gets replaced in amg_block_cases.POOL, never kept under a
    wider bar)."""
    worst, at = 0.0, None
    for shape in abc.SHAPES:
        for col in abc.POOL[shape]:
            d = abc.case(shape).dev_ref(col)
            print(shape, col, "k", abc.case(shape).ref(col).k, "dev_ref", d)
            if d > worst:
                worst, at = d, (shape, col)
    for world in (2, 3):
        d = max(abc.slab_case(world).dev_refs())
        print("slabs", world, "dev_ref", d)
        if d > worst:
            worst, at = d, ("slabs", world)
    print("largest dev_ref", worst, at)
    assert worst <= 1e-7, (worst, at)
