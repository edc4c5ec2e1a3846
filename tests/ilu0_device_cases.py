"""The device setup of spmv::Ilu0Preconditioner (spmv_hip_ilu0_plan_build)
restated in numpy from GIVEN colours.  No GPU and no library are needed to
import this.

ilu_ref      the symbolic half: ilu0_cases.Ilu0Ref for perm, color_start and
             the parts' ptr / cpos / src (entries ascending by the POSITION of
             the column, a duplicate raises ValueError), sgs_layout.slice_part
             for the sliced arrays and, by fill_slots' rule, slot.  Returns the
             dicts host.Ilu0Preconditioner.plan_arrays() and .ilu_arrays()
             return: the sweep plan with every value, padding and dinv +0.0 --
             the placeholders the factorisation writes -- and the part arrays.
             src counts in the arrays GIVEN: for symmetric storage hand it the
             arrays the matrix keeps (sgs_device_cases.lower_of).
with_factor  the plan after a factorisation: l~ / u~ scattered by slot, dinv~
             by row.
raw_ilu_build  the C entry on raw device arrays."""
import ctypes as C

import numpy as np

import ilu0_cases as ic
import sgs_device_cases as dc
from sgs_layout import LONG_THRESHOLD, SLICED_KEYS, _McgsPart, layout, scatter

ILU_KEYS = (("ptr", np.int64), ("cpos", np.int32), ("src", np.int32),
            ("slot", np.int64))
DUPLICATE = 6  # SPMV_HIP_ILU0_DUPLICATE


class _Ilu0Export(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in ILU_KEYS]


def ilu_ref(csr, n, symmetric, colours, long_threshold=LONG_THRESHOLD):
    """-> (plan, ilu, ref): plan as plan_arrays(), ilu as ilu_arrays(), ref the
    Ilu0Ref (factor, apply)"""
    rp, ci, va = (np.asarray(a) for a in csr)
    rp, ci, va = rp[:n + 1], ci[:int(rp[n]) if n else 0], va[:int(rp[n]) if n else 0]
    if n == 0:
        empty = {k: np.zeros(1 if k in ("color_slice", "color_long", "slice_ptr",
                                        "long_ptr") else 0, dc.PART_TYPES[k])
                 for k in SLICED_KEYS}
        plan = dict(perm=np.zeros(0, np.int32), color_start=np.zeros(1, np.int32),
                    dinv=np.zeros(0), before=empty, after=dict(empty))
        part = {k: np.zeros(0, t) for k, t in ILU_KEYS}
        return plan, dict(before=part, after=dict(part)), None
    ref = ic.Ilu0Ref((rp, ci, va), n, colours, symmetric)
    lay = layout(ref, long_threshold)
    plan = dict(perm=lay["perm"], color_start=lay["color_start"], dinv=np.zeros(n))
    ilu = {}
    for h in ("before", "after"):
        plan[h] = lay[h]["sliced"]
        ilu[h] = {k: np.asarray(lay[h][k]).astype(t) for k, t in ILU_KEYS}
    return plan, ilu, ref


def with_factor(plan, ilu, ref, fac):
    """the plan after ilu0_factor wrote fac = (l, u, d by position) into it"""
    l, u, d = fac
    with np.errstate(all="ignore"):
        dinv = np.zeros(ref.n)
        dinv[ref.perm] = 1.0 / d
    out = dict(plan, dinv=dinv)
    for h, w in (("before", l), ("after", u)):
        out[h] = scatter(plan[h], ilu[h]["slot"], w)
    return out


def same_ilu(got, want):
    """None, or the name of the first part array that differs"""
    for h in ("before", "after"):
        for k, t in ILU_KEYS:
            a, b = np.asarray(got[h][k]), np.asarray(want[h][k]).astype(t)
            if a.dtype != t or a.shape != b.shape or not np.array_equal(a, b):
                return f"{h}.{k}"
    return None


def export_ilu(hip, plan):
    """a device plan of either builder -> (plan_arrays dict with bytes,
    ilu_arrays dict with bytes)"""
    sizes = np.zeros(4, np.int64)
    assert hip.spmv_hip_ilu0_plan_sizes(plan, sizes.ctypes.data) == 0
    n = int(sizes[0])
    ilu, structs = dict(bytes=int(sizes[3])), []
    for h, m in (("before", int(sizes[1])), ("after", int(sizes[2]))):
        count = dict(ptr=n + 1 if n > 0 else 0, cpos=m, src=m, slot=m)
        ilu[h] = {k: np.zeros(count[k], t) for k, t in ILU_KEYS}
        s = _Ilu0Export()
        for k, _ in ILU_KEYS:
            setattr(s, k, ilu[h][k].ctypes.data)
        structs.append(s)
    assert hip.spmv_hip_ilu0_plan_export(plan, C.byref(structs[0]),
                                         C.byref(structs[1])) == 0
    inner = C.c_void_p()
    assert hip.spmv_hip_ilu0_mcgs_plan(plan, C.byref(inner)) == 0
    total = C.c_int64()
    assert hip.spmv_hip_ilu0_plan_bytes(plan, C.byref(total)) == 0
    ilu["total_bytes"] = total.value
    return dc.export_plan(hip, inner), ilu


def raw_ilu_build(hip, exec_, csr, n, num_cols, symmetric, colours,
                  num_colors=None, threshold=LONG_THRESHOLD):
    """spmv_hip_ilu0_plan_build -> (return code, info[4], plan arrays, part
    arrays); no value array is handed over"""
    rp, ci, _ = csr
    dev = dc._Dev(exec_)
    try:
        d_rp, d_ci = dev.put(rp, np.int32), dev.put(ci, np.int32)
        d_col = dev.put(colours, np.int32)
        nc = int(np.max(colours)) + 1 if num_colors is None else num_colors
        plan, info = C.c_void_p(), np.full(4, -1, np.int64)
        rc = hip.spmv_hip_ilu0_plan_build(
            exec_.context, n, num_cols, len(ci), d_rp, d_ci, int(symmetric),
            d_col, nc, threshold, C.byref(plan), info.ctypes.data, None)
        if rc != 0:
            assert not plan.value
            return rc, info, None, None
        try:
            return (rc, info) + export_ilu(hip, plan)
        finally:
            assert hip.spmv_hip_ilu0_plan_destroy(plan) == 0
    finally:
        dev.close()


def duplicate_general(n=40):
    """general storage: column 7 stored twice in row 20 (not adjacent, columns
    otherwise ascending) -> (csr, the row)"""
    rp, ci, va = dc.lonely_row(n)
    rows = dc._row_of(rp)
    return dc.from_triplets(n, np.concatenate([rows, [20, 20]]),
                            np.concatenate([ci, [7, 7]]),
                            np.concatenate([va, [-0.1, -0.2]])), 20


def duplicate_mirrored(n=40):
    """symmetric storage: the stored lower entry (20, 7) twice -- row 20 sees two
    stored entries, row 7 two mirror images -> (csr, the smaller row)"""
    csr, _ = duplicate_general(n)
    return csr, 7
