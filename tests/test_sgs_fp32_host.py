"""CPU checks of SgsOptions::values = fp32 (fp32 values in the sweep plans of
SgsPreconditioner and Ilu0Preconditioner): the range rule pinned against numpy,
the new symbols, the rules of the option, and the iteration counts of the
numpy restatement with fp64 and with rounded values that test_gpu_sgs_fp32.py's
cap rests on (printed for DESIGN)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from spmv_amd import _lib, host
from test_gpu_sgs import Sweeps, ragged_spd
from test_sgs_device_host import _declared_arity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

HIP_NEW = ("spmv_hip_mcgs_plan_create_ex", "spmv_hip_mcgs_plan_build_ex",
           "spmv_hip_mcgs_plan_value_bits", "spmv_hip_ilu0_plan_create_ex",
           "spmv_hip_ilu0_plan_build_ex", "spmv_hip_ilu0_counts")
HOST_NEW = ("spmvh_sgs_create_ex2", "spmvh_ilu0_create_ex2",
            "spmvh_sgs_value_bits", "spmvh_fp32_range_count")


def rounded(v):
    """fp64 -> fp32 (nearest-even) -> fp64, as numpy does it"""
    with np.errstate(all="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def range_count_ref(v):
    """the rule restated: finite, non-zero, and the rounding is +-Inf, zero or
    an fp32 subnormal"""
    v = np.asarray(v, np.float64)
    f = np.abs(rounded(v))
    tiny = float(np.finfo(np.float32).tiny)  # 2^-126
    return int(np.sum(np.isfinite(v) & (v != 0.0) & (np.isinf(f) | (f < tiny))))


# ---- 1. the range rule ---------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
LAST_TO_FLT_MAX = float(np.nextafter(2.0 ** 128 - 2.0 ** 103, 0.0))
FIRST_TO_INF = 2.0 ** 128 - 2.0 ** 103
FLT_MIN = 2.0 ** -126
ROUNDS_UP_TO_FLT_MIN = 2.0 ** -126 - 2.0 ** -150   # the tie: to the even 2^-126
FIRST_TO_SUBNORMAL = float(np.nextafter(ROUNDS_UP_TO_FLT_MIN, 0.0))
HAND = [
    (0.0, 0), (-0.0, 0), (np.inf, 0), (-np.inf, 0), (np.nan, 0),
    (FLT_MAX, 0), (-FLT_MAX, 0), (LAST_TO_FLT_MAX, 0), (FIRST_TO_INF, 1),
    (-FIRST_TO_INF, 1), (1e300, 1), (FLT_MIN, 0), (-FLT_MIN, 0),
    (ROUNDS_UP_TO_FLT_MIN, 0), (FIRST_TO_SUBNORMAL, 1), (3.0 * 2.0 ** -140, 1),
    (-(2.0 ** -149), 1), (2.0 ** -150, 1), (2.0 ** -1060, 1), (1.0, 0),
    (1.0 + 2.0 ** -30, 0), (-3.5e-30, 0)]


def test_the_hand_made_vector_is_what_it_says():
    """the roundings the cases are named after, by numpy"""
    tiny = np.float32(FLT_MIN)
    assert np.float32(LAST_TO_FLT_MAX) == np.float32(FLT_MAX)
    assert np.isinf(rounded(FIRST_TO_INF))
    assert np.float32(ROUNDS_UP_TO_FLT_MIN) == tiny
    assert ROUNDS_UP_TO_FLT_MIN < FLT_MIN
    assert 0 < np.float32(FIRST_TO_SUBNORMAL) < tiny
    assert 0 < np.float32(3.0 * 2.0 ** -140) < tiny
    assert np.float32(2.0 ** -150) == 0.0


def test_fp32_range_count_against_numpy():
    v = np.array([x for x, _ in HAND])
    want = np.array([c for _, c in HAND])
    for x, c in HAND:  # one by one: which value, not only how many
        assert host.fp32_range_count([x]) == c == range_count_ref([x]), x
    assert host.fp32_range_count(v) == want.sum() == range_count_ref(v)
    assert host.fp32_range_count(np.zeros(0)) == 0
    # a seeded sweep over every binade near the two edges
    rng = np.random.default_rng(32)
    for centre in (-126, -149, 128):
        w = rng.uniform(1, 2, 4000) * 2.0 ** rng.integers(centre - 3, centre + 3, 4000)
        w = w[np.isfinite(w)] * rng.choice([-1.0, 1.0], len(w))
        assert host.fp32_range_count(w) == range_count_ref(w)
        if centre != -149:  # (there every value is below FLT_MIN: all count)
            assert 0 < range_count_ref(w) < len(w)


# ---- 2. the interface ---------------------------------------------------------------
def test_symbols_declared_exported_prototyped():
    hip_decl = _declared_arity("spmv_hip.h")
    host_decl = _declared_arity("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert len(getattr(_lib.hip, n).argtypes) == hip_decl[n], n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert len(getattr(host.lib, n).argtypes) == host_decl[n], n
    assert _lib.hip.spmv_hip_abi_version() == 5  # additive
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    for text in ("enum class SgsValues { fp64, fp32 }",
                 "SgsValues values = SgsValues::fp64", "int value_bits() const"):
        assert text in cg_h, text


def test_null_handles_and_bad_widths_refused_without_a_device():
    h = _lib.hip
    plan, bits = C.c_void_p(), C.c_int()
    count = C.c_int64()
    info = np.zeros(4, np.int64)
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert h.spmv_hip_mcgs_plan_create_ex(None, None, 32, C.byref(plan),
                                          C.byref(count)) == EINVAL
    assert h.spmv_hip_mcgs_plan_value_bits(None, C.byref(bits)) == EINVAL
    assert h.spmv_hip_ilu0_plan_create_ex(None, None, 32, C.byref(plan)) == EINVAL
    assert h.spmv_hip_ilu0_counts(None, None, C.byref(a), C.byref(b), C.byref(c),
                                  None) == EINVAL
    ctx = C.create_string_buffer(4096)
    v = C.addressof(ctx) + 1024
    for width in (0, 16, 33, -32):  # refused before the context is read
        assert h.spmv_hip_mcgs_plan_create_ex(ctx, v, width, C.byref(plan),
                                              C.byref(count)) == EINVAL
        assert h.spmv_hip_ilu0_plan_create_ex(ctx, v, width,
                                              C.byref(plan)) == EINVAL
        assert h.spmv_hip_mcgs_plan_build_ex(
            ctx, 4, 4, 0, None, None, None, None, 0, v, 1, 64, width,
            C.byref(plan), info.ctypes.data, C.byref(count), None) == EINVAL
        assert h.spmv_hip_ilu0_plan_build_ex(
            ctx, 4, 4, 0, None, None, 0, v, 1, 64, width, C.byref(plan),
            info.ctypes.data, None) == EINVAL
    assert h.spmv_hip_mcgs_plan_create_ex(ctx, v, 32, C.byref(plan),
                                          None) == EINVAL
    assert not plan.value


def test_the_rules_of_values():
    lib = host.lib
    M = C.c_void_p()
    for fn in (lib.spmvh_sgs_create_ex2, lib.spmvh_ilu0_create_ex2):
        for values in (2, -1, 32):  # the enum, before any handle is looked at
            assert fn(None, None, 1, 0, None, values, C.byref(M)) != 0
            assert b"values" in lib.spmvh_last_error()
        assert fn(None, None, 0, 1, None, 1, C.byref(M)) != 0
        assert b"setup = host" in lib.spmvh_last_error()
        assert fn(None, None, 0, -1, None, 1, C.byref(M)) != 0
        assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_value_bits(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    nobody = SimpleNamespace(h=None)
    for cls in (host.SgsPreconditioner, host.Ilu0Preconditioner):
        for bad in ("bf16", "fp16", 32, None):
            with pytest.raises(ValueError, match="values"):
                cls(nobody, nobody, values=bad)
            with pytest.raises(ValueError, match="values"):
                cls(nobody, nobody, setup="device", values=bad)
        # a good width reaches the library (which misses its handles)
        with pytest.raises(host.SpmvHostError, match="NULL"):
            cls(nobody, nobody, values="fp32")
        with pytest.raises(host.SpmvHostError, match="setup = host"):
            cls(nobody, nobody, setup="host", order="natural", values="fp32")


# ---- 3. the cap of the whole solves, on the CPU first ------------------------------------
def round_offdiagonal(csr):
    rp, ci, va = csr
    on = ci == tp._row_of(rp)
    return rp, ci, np.where(on, va, rounded(va))


def nonsymmetric(csr):
    """a nonsymmetric variant: the strictly upper entries shrunk, row by row
    still diagonally dominant"""
    rp, ci, va = csr
    rows = tp._row_of(rp)
    k = np.arange(len(va))
    return rp, ci, np.where(ci > rows, va * (0.55 + 0.4 * np.sin(k) ** 2), va)


def test_reference_iterations_fp64_against_rounded():
    """pcg_sgs of the CPU reference to 1e-10 with the sweeps on the fp64 values
    and on the rounded ones (dinv of the fp64 matrix): inside the cap of the
    GPU test, k32 <= 2 k64, and printed for DESIGN"""
    for name, csr in (("poisson12", tp._csr("poisson12")),
                      ("ragged2001", ragged_spd(2001, 11))):
        n = len(csr[0]) - 1
        dinv = 1.0 / tp._diag_of(csr)
        b = oracle.csr_spmv(*csr, np.random.default_rng(n + 1).uniform(-1, 1, n))
        colours, _ = host.sgs_color(csr[0], csr[1], n, n, False)
        ks = {}
        for width, mat in ((64, csr), (32, round_offdiagonal(csr))):
            sw = Sweeps(mat, n, colours, False)
            _, k, _ = tc._pcg_ref(lambda p: oracle.csr_spmv(*csr, p), oracle.ddot,
                                  b, lambda r: sw.apply(dinv, r), 200, 1e-10)
            ks[width] = k
        print(f"{name}: pcg_sgs reference k = {ks[64]} (fp64 values), "
              f"{ks[32]} (rounded values)")
        assert ks[64] < 200 and ks[32] <= 2 * ks[64]
        if name == "poisson12":  # 6 and -1 are exact: the same operator
            assert ks[32] == ks[64]
        else:
            assert not np.array_equal(round_offdiagonal(csr)[2], csr[2])
