"""CPU checks of the device setup of spmv::SgsPreconditioner (SgsOptions,
spmv_hip_mcgs_color, spmv_hip_mcgs_plan_build, the export): the restatements of
sgs_device_cases.py against the host builder, the new symbols, the NULL checks
and the rules of the options.  The restatements are what test_gpu_sgs_device.py
holds the device against, so they are proved here first:

  colour_ref(natural) == host.sgs_color, entry for entry, on every matrix;
  colour_ref(hashed) is proper on B + B^T and wears every colour;
  plan_ref(greedy colours) == host.sgs_build + sgs_layout.slice_part,
  np.array_equal on every array, both storages.

The last test prints the table of DESIGN 7y: iterations of the CPU reference
pcg_sgs with the greedy and with the hashed colours."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import sgs_device_cases as dc
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from sgs_layout import slice_part
from spmv_amd import _lib, host
from test_gpu_sgs import Sweeps, _make_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

HIP_NEW = ("spmv_hip_mcgs_color", "spmv_hip_mcgs_plan_build",
           "spmv_hip_mcgs_plan_sizes", "spmv_hip_mcgs_plan_export")
HOST_NEW = ("spmvh_sgs_create_ex", "spmvh_sgs_setup_info",
            "spmvh_sgs_setup_detail", "spmvh_sgs_export_sizes",
            "spmvh_sgs_export")

NAMES = ("poisson11", "poisson24", "banded4097", "ragged3001", "diag200",
         "diag1", "clique70", "lonely130", "oneway97", "unsorted150", "hand320")
_cache = {}


def matrix(name):
    if name not in _cache:
        make = {"clique70": dc.clique, "lonely130": dc.lonely_row,
                "oneway97": dc.one_way, "unsorted150": dc.unsorted_duplicates,
                "hand320": lambda: dc.hand_coloured()[0]}
        _cache[name] = make[name]() if name in make else _make_csr(name)
    return _cache[name]


# ---- 1. the restatements ------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_natural_restatement_is_the_host_colouring(name, symmetric):
    csr = matrix(name)
    n = len(csr[0]) - 1
    got, nc = dc.colour_ref(csr, n, symmetric, "natural")
    want, nc_want = host.sgs_color(csr[0], csr[1], n, n, symmetric)
    assert nc == nc_want and np.array_equal(got, want)
    if name == "clique70":
        assert nc == 70
    if name == "ragged3001":
        assert nc == 24


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_hashed_restatement_is_proper_and_wears_every_colour(name, symmetric):
    csr = matrix(name)
    n = len(csr[0]) - 1
    colours, nc = dc.colour_ref(csr, n, symmetric, "hashed")
    assert colours.min() == 0 and len(np.unique(colours)) == nc
    assert dc.is_proper(csr, n, symmetric, colours)


def test_hashed_colours_of_poisson():
    """7-point Poisson: 6 colours against the greedy's 2"""
    for n3, sizes in ((11, None), (24, [4259, 4304, 3006, 1790, 453, 12])):
        csr = matrix(f"poisson{n3}")
        n = n3 ** 3
        colours, nc = dc.colour_ref(csr, n, False, "hashed")
        assert nc == 6
        assert host.sgs_color(csr[0], csr[1], n, n, False)[1] == 2
        if sizes:
            assert np.bincount(colours).tolist() == sizes


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_plan_restatement_is_the_host_builder(name, symmetric):
    csr = matrix(name)
    n = len(csr[0]) - 1
    b = host.sgs_build(*csr, n, n, symmetric)
    want = dict(perm=b["perm"], color_start=b["color_start"], dinv=1.0 / b["d"])
    for h in ("before", "after"):
        want[h] = slice_part(b["color_start"], *b[h])[0]
    got = dc.plan_ref(csr, n, symmetric, b["colors"])
    assert dc.same_plan(got, want) is None
    if name == "ragged3001":  # long rows in both parts
        assert len(got["before"]["long_pos"]) and len(got["after"]["long_pos"])
    if name == "clique70":  # 64 entries stay in the slice, 65 go to the list
        pos = got["perm"].tolist()
        assert got["before"]["len"][pos.index(64)] == 64
        assert got["before"]["len"][pos.index(65)] == -1
        assert got["after"]["len"][pos.index(5)] == 64
        assert got["after"]["len"][pos.index(4)] == -1


def test_hand_coloured_matrix_has_the_slice_edges():
    csr, colours = dc.hand_coloured()
    n = len(csr[0]) - 1
    assert np.bincount(colours).tolist() == [63, 64, 65, 128]
    assert dc.is_proper(csr, n, False, colours)
    p = dc.plan_ref(csr, n, False, colours)
    assert p["before"]["color_slice"].tolist() == [0, 1, 2, 4, 6]


# ---- 2. the interface ---------------------------------------------------------------
def _declared_arity(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_symbols_declared_exported_prototyped():
    hip_decl = _declared_arity("spmv_hip.h")
    host_decl = _declared_arity("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert len(getattr(_lib.hip, n).argtypes) == hip_decl[n], n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert len(getattr(host.lib, n).argtypes) == host_decl[n], n
    assert _lib.hip.spmv_hip_abi_version() == 5
    mk = open(os.path.join(ROOT, "spmv_amd", "csrc", "Makefile")).read()
    assert "hip/spmv_mcgs_build.hip" in mk
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    for text in ("struct SgsOptions", "SgsSetup setup = SgsSetup::host",
                 "SgsOrder order = SgsOrder::hashed",
                 "const int32_t* colors = nullptr", "int rounds() const",
                 "double setup_ms() const", "slow on long"):
        assert text in cg_h, text


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    plan, nc, rounds = C.c_void_p(), C.c_int(), C.c_int()
    info = np.zeros(4, np.int64)
    sizes = np.zeros(10, np.int64)
    assert h.spmv_hip_mcgs_color(None, 4, 4, 0, None, None, 0, 0, None,
                                 C.byref(nc), C.byref(rounds), None) == EINVAL
    assert h.spmv_hip_mcgs_plan_build(None, 4, 4, 0, None, None, None, None, 0,
                                      None, 1, 64, C.byref(plan),
                                      info.ctypes.data, None) == EINVAL
    assert h.spmv_hip_mcgs_plan_sizes(None, sizes.ctypes.data) == EINVAL
    assert h.spmv_hip_mcgs_plan_export(None, None, None, None, None,
                                       None) == EINVAL
    # a context but arguments that cannot be: refused before the context is read
    ctx = C.create_string_buffer(4096)
    v = C.addressof(ctx) + 1024
    assert h.spmv_hip_mcgs_color(ctx, 4, 4, 0, None, None, 0, 0, v, None,
                                 C.byref(rounds), None) == EINVAL
    assert h.spmv_hip_mcgs_color(ctx, 4, 3, 0, None, None, 0, 0, v, C.byref(nc),
                                 C.byref(rounds), None) == EINVAL  # cols < rows
    assert h.spmv_hip_mcgs_color(ctx, 4, 4, 0, None, None, 0, 2, v, C.byref(nc),
                                 C.byref(rounds), None) == EINVAL  # order
    assert h.spmv_hip_mcgs_color(ctx, 4, 4, 5, None, None, 0, 0, v, C.byref(nc),
                                 C.byref(rounds), None) == EINVAL  # no arrays
    assert h.spmv_hip_mcgs_plan_build(ctx, 4, 4, 0, None, None, None, None, 0, v,
                                      1, 64, None, info.ctypes.data,
                                      None) == EINVAL
    assert h.spmv_hip_mcgs_plan_build(ctx, 4, 4, 0, None, None, None, None, 0,
                                      None, 1, 64, C.byref(plan),
                                      info.ctypes.data, None) == EINVAL
    assert h.spmv_hip_mcgs_plan_build(ctx, 4, 4, 0, None, None, None, None, 1, v,
                                      1, 64, C.byref(plan), info.ctypes.data,
                                      None) == EINVAL  # symmetric, no diagonal
    assert not plan.value
    lib = host.lib
    M = C.c_void_p()
    assert lib.spmvh_sgs_create_ex(None, None, 1, 0, None, C.byref(M)) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_setup_info(None, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_setup_detail(None, None, None, None) != 0
    assert lib.spmvh_sgs_export_sizes(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_export(None, None, None, None, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()


def test_host_setup_takes_neither_colours_nor_an_order():
    """the rule is checked before any handle is looked at"""
    lib = host.lib
    M = C.c_void_p()
    colours = np.zeros(4, np.int32)
    for order, col in ((0, None), (1, None), (-1, colours.ctypes.data)):
        assert lib.spmvh_sgs_create_ex(None, None, 0, order, col, C.byref(M)) != 0
        assert b"setup = host" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_create_ex(None, None, 2, -1, None, C.byref(M)) != 0
    assert b"setup" in lib.spmvh_last_error()
    nobody = SimpleNamespace(h=None)
    for kw in (dict(order="natural"), dict(order="hashed"), dict(colors=colours)):
        with pytest.raises(host.SpmvHostError, match="setup = host"):
            host.SgsPreconditioner(nobody, nobody, setup="host", **kw)
    with pytest.raises(ValueError):
        host.SgsPreconditioner(nobody, nobody, setup="gpu")


# ---- 3. for DESIGN 7y ---------------------------------------------------------------
def test_reference_iterations_greedy_against_hashed():
    """pcg_sgs of the CPU reference to 1e-10, b = A * uniform(-1, 1): printed
    for DESIGN 7y, asserted only to converge"""
    for name in ("poisson24", "banded4097", "ragged3001"):
        for scaled in (False, True):
            csr = tp._scaled(matrix(name)) if scaled else matrix(name)
            n = len(csr[0]) - 1
            dinv = 1.0 / tp._diag_of(csr)
            b = oracle.csr_spmv(*csr, np.random.default_rng(n + 1).uniform(-1, 1, n))
            ks = {}
            for order in ("natural", "hashed"):
                colours, nc = dc.colour_ref(csr, n, False, order)
                sw = Sweeps(csr, n, colours, False)
                _, k, _ = tc._pcg_ref(lambda p: oracle.csr_spmv(*csr, p),
                                      oracle.ddot, b,
                                      lambda r: sw.apply(dinv, r), 200, 1e-10)
                ks[order] = (nc, k)
                assert k < 200
            print(f"{name} {'scaled' if scaled else 'plain'}: greedy "
                  f"{ks['natural'][0]} colours k = {ks['natural'][1]}, hashed "
                  f"{ks['hashed'][0]} colours k = {ks['hashed'][1]}")
