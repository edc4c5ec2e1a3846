"""The device setup of AmgPreconditioner, the part that needs no device: the
numpy restatement of its definition (amg_device_cases.aggregate_by_priority)
against the host builder, the round-by-round simulation of the device scheme
against the definition, and the interface.

With natural priorities the definition must BE host.amg_symbolic (agg, member
lists, coarse pattern, source lists) on every matrix, both storages, theta 0,
0.25 and 1.  With either order the rounds must give the definition's
aggregates: that is what makes the launches of spmv_amg_build.hip correct."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_cases as ac
import amg_device_cases as dc
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_amg_aggregate", "spmv_hip_amg_plan_build",
           "spmv_hip_amg_plan_sizes", "spmv_hip_amg_plan_export")
HOST_NEW = ("spmvh_amg_create_ex", "spmvh_amg_setup_info",
            "spmvh_amg_level_rounds", "spmvh_amg_step_sizes",
            "spmvh_amg_step_export")
KEYS = ("agg", "member_ptr", "member", "rowptr", "colind", "src_ptr", "src")

GENERAL = ("poisson11", "poisson24", "banded4097", "ragged3001", "convdiff8",
           "arrow130", "diag200", "diag1", "empty7", "duplicates", "weak_row")
# (symmetric storage of a nonsymmetric matrix stands for another matrix; the
# empty block has no diagonal to split off)
BOTH = tuple(n for n in GENERAL if n not in ("convdiff8", "empty7"))


def _cases():
    out = []
    for name in GENERAL:
        for sym in ((False, True) if name in BOTH else (False,)):
            for theta in (0.0, 0.25, 1.0):
                out.append((name, sym, theta))
    return out


_made = {}


def expanded(name, sym):
    """-> (csr of the storage, diagonal, n, ptr, col, src, val), made once"""
    if (name, sym) not in _made:
        csr = dc.matrix(name)
        n = len(csr[0]) - 1
        st, diag = dc.storages(csr, n, sym)
        ptr, col, src = ac.expand(st[0], st[1], n, sym)
        _made[name, sym] = (st, diag, n, ptr, col, src,
                            ac.values_of(src, st[2], diag))
    return _made[name, sym]


# ---- 1. the interface ----------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped():
    hip_h = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    host_h = open(os.path.join(ROOT, "include", "spmv_host_c.h")).read()
    for name in HIP_NEW:
        assert re.search(r"\b%s\(" % name, hip_h), name
        assert getattr(_lib.hip, name).argtypes is not None, name
    for name in HOST_NEW:
        assert re.search(r"\b%s\(" % name, host_h), name
        assert hasattr(host.lib, name), name


def test_null_arguments_are_refused_without_a_device():
    info = (C.c_int64 * 4)()
    n_agg, rounds = C.c_int32(), (C.c_int * 2)()
    assert _lib.hip.spmv_hip_amg_aggregate(
        None, 0, 0, 0, None, None, None, None, 0, 0.25, 0, None, C.byref(n_agg),
        rounds, info, None) != 0
    assert _lib.hip.spmv_hip_amg_plan_sizes(None, None) != 0
    assert _lib.hip.spmv_hip_amg_plan_export(None, None) != 0


def test_python_layer_takes_setup_and_order():
    import inspect
    sig = inspect.signature(host.AmgPreconditioner.__init__)
    assert sig.parameters["setup"].default == "host"
    assert sig.parameters["order"].default is None
    for name in ("setup_detail", "rounds", "step_arrays"):
        assert callable(getattr(host.AmgPreconditioner, name))


# ---- 2. natural priorities: the host builder, entry for entry ------------------------
@pytest.mark.parametrize("name,sym,theta", _cases())
def test_natural_definition_is_the_host_builder(name, sym, theta):
    st, diag, n, ptr, col, src, val = expanded(name, sym)
    want = host.amg_symbolic(*st, n, n, sym, diag, theta)
    got = dc.coarsen(st, n, sym, diag, theta, "natural")
    assert got["n_agg"] == want["n_agg"], (name, sym, theta)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (name, sym, theta, k)
    assert np.array_equal(got["xrow_ptr"], want["xrow_ptr"])
    assert np.array_equal(got["xrow_src"], want["xrow_src"])


# ---- 3. the rounds give the definition, both orders ------------------------------------
@pytest.mark.parametrize("order", dc.ORDERS)
@pytest.mark.parametrize("name,sym,theta", _cases())
def test_rounds_give_the_definition(name, sym, theta, order):
    st, diag, n, ptr, col, src, val = expanded(name, sym)
    agg, n_agg = dc.aggregate_by_priority(ptr, col, val, n, theta, order)
    got, got_n, rounds = dc.aggregate_in_rounds(ptr, col, val, n, theta, order)
    print(name, sym, theta, order, "aggregates", n_agg, "rounds", rounds)
    assert got_n == n_agg
    assert np.array_equal(got, agg), (name, sym, theta, order)
    assert 1 <= rounds[0] <= n + 1 and 1 <= rounds[1] <= n + 1 or n == 0
    # a partition into non-empty aggregates
    assert np.array_equal(np.unique(agg), np.arange(n_agg))


def test_hashed_differs_and_needs_fewer_rounds_on_a_lattice():
    st, diag, n, ptr, col, src, val = expanded("poisson11", False)
    nat = dc.aggregate_in_rounds(ptr, col, val, n, 0.25, "natural")
    has = dc.aggregate_in_rounds(ptr, col, val, n, 0.25, "hashed")
    assert not np.array_equal(nat[0], has[0])
    assert has[2][0] < nat[2][0], (has[2], nat[2])


def test_the_weak_row_is_a_singleton_and_nobody_elses_first_choice():
    st, diag, n, ptr, col, src, val = expanded("weak_row", False)
    strong = dc.strong_lists(ptr, col, val, n, 0.25)
    assert strong[3] == []
    for order in dc.ORDERS:
        agg, _ = dc.aggregate_by_priority(ptr, col, val, n, 0.25, order)
        assert 0 <= agg[3]


def test_priorities_are_unique_and_positive():
    for order in dc.ORDERS:
        p = dc.priorities(5000, order)
        assert len(set(p)) == len(p) and min(p) > 0 and max(p) < 1 << 64
