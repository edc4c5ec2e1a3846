"""The fused AMG tail without a GPU: the tail_rows rule, the selection of the
tail restated (amg_tail_cases.first_tail_level) and held against the level sizes
amg_cases.AmgRef gives for every object case of test_gpu_amg_tail.py, the
restatement of the kernel's walk (amg_tail_cases.tail_ref) held bit for bit
against AmgRef's own cycle, the launch arithmetic, the entry points, and
tools/amg_tail_check.cpp built with the sanitizers and run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import amg_cases as ac
import amg_tail_cases as tc
import gmres_cases as gc
import test_gpu_amg as ta
from spmv_amd import _lib, hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

HIP_NEW = ("spmv_hip_amg_tail_create", "spmv_hip_amg_tail_destroy",
           "spmv_hip_amg_tail_set_coefficients", "spmv_hip_amg_tail_bytes",
           "spmv_hip_amg_tail_run_f64")
HOST_NEW = ("spmvh_amg_set_tail_rows", "spmvh_amg_tail_levels",
            "spmvh_amg_check_tail_rows", "spmvh_amg_tail_lanes")


def test_entry_points_exist():
    for name in HIP_NEW:
        assert hasattr(_lib.hip, name), name
    for name in HOST_NEW:
        assert hasattr(host.lib, name), name
    for name in ("set_tail_rows", "tail_levels", "tail_lanes"):
        assert callable(getattr(host.AmgPreconditioner, name)), name
    assert callable(hip.AmgTail)
    with open(os.path.join(ROOT, "include", "spmv_hip.h")) as f:
        text = f.read()
    for name in HIP_NEW:
        assert name + "(" in text, name
    with open(os.path.join(ROOT, "include", "spmv_host_c.h")) as f:
        text = f.read()
    for name in HOST_NEW:
        assert name + "(" in text, name


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5


def test_amg_options_keep_their_seven_fields():
    assert len(host.AMG_DEFAULTS) == 7 and "tail_rows" not in host.AMG_DEFAULTS


def test_tail_rows_rule():
    for ok in (0, 1, 150, 10 ** 9, 2 ** 62):
        host.amg_check_tail_rows(ok)
    for bad in (-1, -(2 ** 40)):
        with pytest.raises(host.SpmvHostError, match="tail_rows"):
            host.amg_check_tail_rows(bad)
    # the rule comes before the handle: no device, no object
    assert host.lib.spmvh_amg_set_tail_rows(None, -1) != 0
    assert b"tail_rows" in host.lib.spmvh_last_error()


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    out, n64 = C.c_void_p(), C.c_int64()
    assert h.spmv_hip_amg_tail_create(None, None, C.byref(out)) == EINVAL
    assert h.spmv_hip_amg_tail_destroy(None) == 0
    assert h.spmv_hip_amg_tail_bytes(None, C.byref(n64)) == EINVAL
    assert h.spmv_hip_amg_tail_set_coefficients(None, 0, None, None) == EINVAL
    assert h.spmv_hip_amg_tail_run_f64(None, None, None) == EINVAL


def test_first_tail_level_rule():
    f = tc.first_tail_level
    assert f([13824, 1685, 150], 0) == 3
    assert f([13824, 1685, 150], 149) == 3
    assert f([13824, 1685, 150], 150) == 2
    assert f([13824, 1685, 150], 1684) == 2
    assert f([13824, 1685, 150], 1685) == 1
    assert f([13824, 1685, 150], 10 ** 9) == 1  # level 0 is never in it
    assert f([200], 10 ** 9) == 1 and tc.tail_levels([200], 10 ** 9) == 0
    assert f([900, 50, 400, 60], 100) == 3  # a suffix: 50 is above 400
    assert f([900, 50, 400, 60], 400) == 1


@pytest.mark.parametrize("case", tc.OBJECT_CASES, ids=lambda c: c[0])
def test_expected_tail_levels_follow_from_the_reference_sizes(case):
    name, options, sizes, expect = case
    csr = ta._make_csr(name)
    n = len(csr[0]) - 1
    ref = ac.AmgRef(csr, n, **options)
    assert tuple(L["n"] for L in ref.levels) == sizes
    for tail_rows, levels in expect.items():
        assert tc.tail_levels(sizes, tail_rows) == levels, (name, tail_rows)
    if len(sizes) > 1:  # a case with levels to fuse does fuse some
        assert max(expect.values()) >= 1, name
    else:
        assert set(expect.values()) == {0}, name


def test_the_listed_poisson24_expectations():
    assert tc.POISSON24[2] == (13824, 1685, 150)
    assert tc.POISSON24[3] == {149: 0, 150: 1, 1685: 2, 10 ** 9: 2}
    # ragged3001: its level 1 is the whole tail and runs the vector order
    csr = ta._make_csr("ragged3001")
    ref = ac.AmgRef(csr, len(csr[0]) - 1)
    assert ac.vector_lanes(ref.levels[1]["csr"]) == 64


def test_launch_arithmetic():
    for nl in (2, 3, 5):
        for s in (1, 2, 3):
            for c in (1, 8):
                full = tc.launches(nl, s, c)
                assert full == (nl - 1) * ((2 * s + 1) + 2 * s + 2) + 2 * c
                for tail in range(1, nl):
                    t = nl - tail
                    saved = (nl - 1 - t) * (4 * s + 3) + (2 * c - 1) - 1
                    assert tc.launches(nl, s, c, tail) == full - saved
    assert tc.launches(3, 2, 8) == 38 and tc.launches(3, 2, 8, 2) == 13


@pytest.mark.parametrize("options", [
    {"min_coarse_rows": 20},
    {"min_coarse_rows": 20, "smooth_degree": 3, "coarse_degree": 1,
     "coarse_scale": 1.6},
    {"min_coarse_rows": 20, "smooth_degree": 1}], ids=["defaults", "s3c1", "s1"])
def test_tail_ref_is_the_cycle_of_amg_ref(options):
    """the restated walk over levels 1 .. last of Poisson 11^3 = AmgRef's own
    recursion from level 1, and the tail of the coarsest level alone"""
    csr = ta._make_csr("poisson11")
    ref = ac.AmgRef(csr, len(csr[0]) - 1, **options)
    o = ref.opt
    assert len(ref.levels) == 3
    for first in (1, 2):
        levels = []
        for l in range(first, 3):
            L = ref.levels[l]
            last = l == 2
            a, b = gc.chebyshev_coefficients(
                o["coarse_degree"] if last else o["smooth_degree"], L["lmin"],
                L["lmax"])
            levels.append(tc.Level(L["csr"], L["dinv"], a, b, L.get("step")))
        r = np.random.default_rng(first).uniform(-1, 1, ref.levels[first]["n"])
        _, zs = tc.tail_ref(levels, o["smooth_degree"], o["coarse_degree"],
                            o["coarse_scale"], r)
        assert np.array_equal(zs[0], ref.cycle(first, r)), (options, first)


def test_hand_built_cases_cover_what_they_claim():
    assert tc.SIZES == (1, 2, 1023, 1024, 1025, 2049)
    t = tc.aggregate_case()
    assert sorted(np.diff(t.levels[0].step["member_ptr"])) == [1, 2, 3, 700]
    mem = t.levels[0].step["member"][-700:]
    assert np.any(np.diff(mem) > 1)  # scattered
    assert tc.one_coarse_row_case().levels[1].n == 1
    lens = np.diff(tc.sequential_lens_case().levels[0].csr[0])
    assert {0, 1, tc.LONG} <= set(lens.tolist())
    for lanes in (4, 64):
        v = tc.vector_case(lanes)
        lens = np.diff(v.levels[0].csr[0])
        assert {0, 1, lanes - 1, lanes, lanes + 1, tc.LONG} <= set(lens.tolist())
        assert v.levels[0].n > 2 * (tc.BLOCK // lanes)  # a third trip
        assert all(L.lanes == lanes for L in v.levels)
    assert len(tc.depth_case().levels) == 3
    for t in tc.special_cases():
        rs, zs = t.ref()
        if "nan" in t.name or "inf" in t.name:
            assert np.any(np.isnan(zs[0])), t.name
    t = tc.special_cases()[0]
    rp, ci, va = t.levels[0].csr
    assert rp[2] - rp[1] == 1 and np.signbit(va[rp[1]]) and va[rp[1]] == 0.0


def test_amg_tail_check_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host compiler (the one that builds the library)"
    exe = str(tmp_path / "amg_tail_check")
    src = os.path.join(ROOT, "spmv_amd", "csrc", "hip")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-I" + src,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "amg_tail_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
