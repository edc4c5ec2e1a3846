"""CPU checks of the device setup of spmv::Ilu0Preconditioner (SgsOptions,
spmv_hip_ilu0_plan_build, the export).  The numpy restatement of
ilu0_device_cases.py is what test_gpu_ilu0_device.py holds the device against,
so it is proved here first: given host.sgs_color's colours it equals
host.ilu0_symbolic (host/ilu0_build.cpp) array for array, on every shape of the
GPU tests and in both storages.  Then the new symbols, the ABI version and the
rules of the options, which need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilu0_cases as ic
import ilu0_device_cases as idc
import sgs_device_cases as dc
from spmv_amd import _lib, host
from test_sgs_device_host import matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMMETRIC = ("poisson11", "poisson24", "banded4097", "ragged3001", "clique70",
             "hand320", "lonely130", "diag200", "diag1")
GENERAL_ONLY = ("arrow300", "oneway97")
HIP_NEW = {"spmv_hip_ilu0_plan_build": 13, "spmv_hip_ilu0_plan_sizes": 2,
           "spmv_hip_ilu0_plan_export": 3}
HOST_NEW = {"spmvh_ilu0_create_ex": 6, "spmvh_ilu0_export_sizes": 2,
            "spmvh_ilu0_export": 3}


def ilu_matrix(name):
    return ic.arrow(300) if name == "arrow300" else matrix(name)


def _cases():
    out = [pytest.param(n, s, id=f"{n}-{'symmetric' if s else 'general'}")
           for n in SYMMETRIC for s in (False, True)]
    return out + [pytest.param(n, False, id=f"{n}-general") for n in GENERAL_ONLY]


@pytest.mark.parametrize("name,symmetric", _cases())
def test_restatement_is_the_host_symbolic(name, symmetric):
    csr = ilu_matrix(name)
    n = len(csr[0]) - 1
    want = host.ilu0_symbolic(csr[0], csr[1], n, symmetric=symmetric)
    colours, nc = host.sgs_color(csr[0], csr[1], n, n, symmetric)
    assert np.array_equal(want["colors"], colours) and want["num_colors"] == nc
    plan, ilu, ref = idc.ilu_ref(csr, n, symmetric, colours)
    assert np.array_equal(plan["perm"], want["perm"])
    assert np.array_equal(plan["color_start"], want["color_start"])
    assert np.array_equal(ref.pos, want["pos"])
    assert idc.same_ilu(ilu, want) is None
    for h in ("before", "after"):
        assert np.array_equal(plan[h]["col"], want[h]["sliced_col"]), h
        assert np.array_equal(plan[h]["long_col"], want[h]["long_col"]), h
        assert not np.any(plan[h]["val"]) and not np.any(plan[h]["long_val"])
        assert not np.any(np.signbit(plan[h]["val"]))
        slot = ilu[h]["slot"]  # every slot once, inside its array
        assert len(np.unique(slot)) == len(slot)
        assert np.all(slot[slot >= 0] < len(plan[h]["col"]))
        assert np.all(~slot[slot < 0] < len(plan[h]["long_col"]))
    assert not np.any(plan["dinv"])
    if name == "arrow300":  # one row of 299 entries in `before`: a long row
        assert np.diff(ilu["before"]["ptr"]).max() == 299
        assert len(plan["before"]["long_pos"]) == 1
    if name == "clique70":
        assert nc == 70 and len(plan["before"]["long_pos"]) > 0
    if name == "hand320" and not symmetric:
        hand = dc.hand_coloured()[1]
        p2 = idc.ilu_ref(csr, n, False, hand)[0]
        assert np.diff(p2["color_start"]).tolist() == [63, 64, 65, 128]


def test_restatement_of_the_empty_block():
    plan, ilu, ref = idc.ilu_ref((np.zeros(1, np.int32), np.zeros(0, np.int32),
                                  np.zeros(0)), 0, False, np.zeros(0, np.int32))
    assert ref is None and len(plan["perm"]) == 0
    assert plan["color_start"].tolist() == [0]
    assert all(len(ilu[h][k]) == 0 for h in ("before", "after")
               for k, _ in idc.ILU_KEYS)


def test_restatement_refuses_what_the_host_refuses():
    for make, sym in ((idc.duplicate_general, False), (idc.duplicate_mirrored, True)):
        csr, _ = make()
        n = len(csr[0]) - 1
        with pytest.raises(host.SpmvHostError, match="duplicate"):
            host.ilu0_symbolic(csr[0], csr[1], n, symmetric=sym)
        colours, _ = host.sgs_color(csr[0], csr[1], n, n, sym)
        with pytest.raises(ValueError, match="duplicate"):
            idc.ilu_ref(csr, n, sym, colours)


def test_long_threshold_of_the_restatement_moves_rows_to_the_long_lists():
    csr = matrix("ragged3001")
    n = len(csr[0]) - 1
    colours, _ = host.sgs_color(csr[0], csr[1], n, n, False)
    p64, i64_, _ = idc.ilu_ref(csr, n, False, colours)
    p4, i4, _ = idc.ilu_ref(csr, n, False, colours, 4)
    assert len(p4["before"]["long_pos"]) > len(p64["before"]["long_pos"])
    for h in ("before", "after"):  # the parts do not depend on the threshold
        for k in ("ptr", "cpos", "src"):
            assert np.array_equal(i4[h][k], i64_[h][k])
        assert np.sum(i4[h]["slot"] < 0) == len(p4[h]["long_col"])


# ---- the symbols and the options ----------------------------------------------------
def _arity(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_exist_with_their_arities():
    for name, arity in HIP_NEW.items():
        assert getattr(_lib.hip, name) is not None
        assert _arity("spmv_hip.h", name) == arity, name
    hostlib = C.CDLL(os.path.join(ROOT, "spmv_amd", "lib", "libspmv_host.so"))
    for name, arity in HOST_NEW.items():
        assert getattr(hostlib, name) is not None
        assert _arity("spmv_host_c.h", name) == arity, name
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ILU0_DUPLICATE\s+6\b", text)


def test_abi_version_is_still_5():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    m = re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 5
    assert _lib.hip.spmv_hip_abi_version() == 5


class _Handle:
    h = None


def test_host_setup_takes_neither_colours_nor_an_order():
    """the rules of the options are checked before any handle is looked at"""
    for kw in (dict(colors=np.zeros(4, np.int32)), dict(order="natural"),
               dict(order="hashed")):
        with pytest.raises(host.SpmvHostError, match="neither colors nor an order"):
            host.Ilu0Preconditioner(_Handle(), _Handle(), setup="host", **kw)
    with pytest.raises(ValueError):
        host.Ilu0Preconditioner(_Handle(), _Handle(), setup="gpu")
    with pytest.raises(ValueError):
        host.Ilu0Preconditioner(_Handle(), _Handle(), setup="device", order="x")
    with pytest.raises(host.SpmvHostError, match="NULL"):
        host.Ilu0Preconditioner(_Handle(), _Handle(), setup="device")
