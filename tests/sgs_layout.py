"""host/sgs_build.h's sliced layout (long lists included) and host/ilu0_build.h's
ptr / cpos / src / slot restated in numpy, from an ilu0_cases.Ilu0Ref.  No GPU,
no library: the colours are the Ilu0Ref's, so the caller's -- any proper
colouring, not the greedy one.

layout(ref) returns what spmv_hip_mcgs_host and spmv_hip_ilu0_host point to;
McgsHost / Ilu0Host turn it into the ctypes structs of include/spmv_hip.h.
sweep() reads the layout arrays the way mcgs_sweep_kernel does -- slices
column-major lane by lane, long rows in chunks of 64 added in their order --
and is the restatement the three mutants of test_sgs_kernel_cases_host.py are
made of."""
import ctypes as C

import numpy as np

LONG_THRESHOLD = 64  # kSgsLongThreshold


# ---- the structs of include/spmv_hip.h ----------------------------------------------
class _McgsPart(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        "color_slice", "slice_pos0", "slice_ptr", "len", "col", "val",
        "color_long", "long_pos", "long_ptr", "long_col", "long_val")]


class _McgsHost(C.Structure):
    _fields_ = [("num_rows", C.c_int32), ("num_colors", C.c_int32),
                ("perm", C.c_void_p), ("color_start", C.c_void_p),
                ("dinv", C.c_void_p), ("before", _McgsPart), ("after", _McgsPart)]


class _Ilu0Part(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("ptr", "cpos", "src", "slot")]


class _Ilu0Host(C.Structure):
    _fields_ = [("mcgs", _McgsHost), ("num_values", C.c_int64),
                ("before", _Ilu0Part), ("after", _Ilu0Part)]


SLICED_KEYS = tuple(k for k, _ in _McgsPart._fields_)


# ---- sgs_slice and fill_slots ---------------------------------------------------------
def slice_part(color_start, ptr, col, val=None, long_threshold=LONG_THRESHOLD):
    """sgs_slice of a part in CSR over positions -> (sliced, slot): the arrays of
    SgsSlicedPart and, per entry of the part, ilu0_build's slot (>= 0: index
    into val; < 0: ~index into long_val)."""
    ptr = np.asarray(ptr, np.int64)
    col = np.asarray(col, np.int32)
    val = np.zeros(len(col)) if val is None else np.asarray(val, np.float64)
    lens = np.diff(ptr)
    ln = np.where(lens > long_threshold, -1, lens).astype(np.int32)
    slot = np.zeros(len(col), np.int64)
    color_slice, color_long, pos0, slice_ptr = [0], [0], [], [0]
    cols, vals, long_pos, long_ptr = [], [], [], [0]
    for c in range(len(color_start) - 1):
        for p0 in range(int(color_start[c]), int(color_start[c + 1]), 64):
            p1 = min(p0 + 64, int(color_start[c + 1]))
            width = max(int(ln[p0:p1].max()), 0)
            bc, bv = np.zeros((width, 64), np.int32), np.zeros((width, 64))
            for pos in range(p0, p1):
                e0, e1 = int(ptr[pos]), int(ptr[pos + 1])
                if ln[pos] < 0:
                    slot[e0:e1] = ~(long_ptr[-1] + np.arange(e1 - e0))
                    long_pos.append(pos)
                    long_ptr.append(long_ptr[-1] + e1 - e0)
                    continue
                m = e1 - e0
                bc[:m, pos - p0], bv[:m, pos - p0] = col[e0:e1], val[e0:e1]
                slot[e0:e1] = slice_ptr[-1] + 64 * np.arange(m) + (pos - p0)
            cols.append(bc.ravel())
            vals.append(bv.ravel())
            pos0.append(p0)
            slice_ptr.append(slice_ptr[-1] + 64 * width)
        color_slice.append(len(pos0))
        color_long.append(len(long_pos))
    in_long = np.repeat(ln < 0, lens)
    sliced = dict(
        color_slice=np.array(color_slice, np.int32),
        slice_pos0=np.array(pos0, np.int32),
        slice_ptr=np.array(slice_ptr, np.int64), len=ln,
        col=np.concatenate(cols + [np.zeros(0, np.int32)]).astype(np.int32),
        val=np.concatenate(vals + [np.zeros(0)]),
        color_long=np.array(color_long, np.int32),
        long_pos=np.array(long_pos, np.int32),
        long_ptr=np.array(long_ptr, np.int64),
        long_col=col[in_long].copy(), long_val=val[in_long].copy())
    return sliced, slot


def scatter(sliced, slot, w):
    """ilu0_scatter: the part's values `w` (part-CSR order) into a copy of the
    sliced layout"""
    out = dict(sliced, val=sliced["val"].copy(), long_val=sliced["long_val"].copy())
    out["val"][slot[slot >= 0]] = np.asarray(w)[slot >= 0]
    out["long_val"][~slot[slot < 0]] = np.asarray(w)[slot < 0]
    return out


def layout(ref, long_threshold=LONG_THRESHOLD):
    """-> dict(n, num_colors, perm, color_start, before, after); a part is
    dict(ptr, cpos, src, slot, sliced): ilu0_symbolic's output for ref's matrix
    and colours, the sliced values 0.0"""
    out = dict(n=ref.n, num_colors=ref.nc, perm=ref.perm.astype(np.int32),
               color_start=ref.color_start.astype(np.int32))
    for name, part in zip(("before", "after"), ref.parts):
        sliced, slot = slice_part(ref.color_start, part["ptr"], part["col"],
                                  None, long_threshold)
        out[name] = dict(ptr=part["ptr"].astype(np.int64),
                         cpos=part["cpos"].astype(np.int32),
                         src=part["src"].astype(np.int32), slot=slot,
                         sliced=sliced)
    return out


def with_values(lay, l, u):
    """the layout with l and u (part-CSR order) scattered into its slices"""
    out = dict(lay)
    for name, w in (("before", l), ("after", u)):
        out[name] = dict(lay[name], sliced=scatter(lay[name]["sliced"],
                                                   lay[name]["slot"], w))
    return out


# ---- the ctypes structs ---------------------------------------------------------------
def _ptr_of(a, keep):
    if a is None or len(a) == 0:
        return None
    keep.append(a)
    return a.ctypes.data_as(C.c_void_p)


def fill_mcgs(s, lay, dinv, keep):
    """fill a _McgsHost from a layout; every array it points to goes to `keep`"""
    s.num_rows, s.num_colors = lay["n"], lay["num_colors"]
    s.perm = _ptr_of(np.ascontiguousarray(lay["perm"], np.int32), keep)
    # (color_start has num_colors + 1 >= 1 entries: never NULL)
    cs = np.ascontiguousarray(lay["color_start"], np.int32)
    keep.append(cs)
    s.color_start = cs.ctypes.data_as(C.c_void_p)
    s.dinv = _ptr_of(np.ascontiguousarray(dinv, np.float64), keep)
    for h in ("before", "after"):
        for k in SLICED_KEYS:
            a = lay[h]["sliced"][k]
            if k in ("color_slice", "color_long", "slice_ptr", "long_ptr"):
                a = np.ascontiguousarray(a)
                keep.append(a)
                setattr(getattr(s, h), k, a.ctypes.data_as(C.c_void_p))
            else:
                setattr(getattr(s, h), k, _ptr_of(a, keep))
    return s


def mcgs_host(lay, dinv):
    """-> (_McgsHost, keep): `keep` owns the arrays, hold it while the struct lives"""
    keep = []
    return fill_mcgs(_McgsHost(), lay, dinv, keep), keep


def ilu0_host(lay, num_values):
    """-> (_Ilu0Host, keep); the sweep plan's values and dinv are placeholders"""
    keep = []
    s = _Ilu0Host()
    fill_mcgs(s.mcgs, lay, np.zeros(lay["n"]), keep)
    s.num_values = num_values
    for h in ("before", "after"):
        for k in ("ptr", "cpos", "src", "slot"):
            a = np.ascontiguousarray(lay[h][k])
            if k == "ptr":
                keep.append(a)
                setattr(getattr(s, h), k, a.ctypes.data_as(C.c_void_p))
            else:
                setattr(getattr(s, h), k, _ptr_of(a, keep))
    return s, keep


def _sliced(sym, part):
    """sgs_build.h's layout of a part of host.ilu0_symbolic's output, restated;
    the columns must be the builder's own"""
    cols = sym["perm"][part["cpos"]]
    sliced, slot = slice_part(sym["color_start"], part["ptr"], cols)
    assert np.array_equal(sliced["col"], part["sliced_col"])  # the builder's own
    assert np.array_equal(sliced["long_col"], part["long_col"])
    assert np.array_equal(slot, part["slot"])
    for k in ("long_pos", "long_col", "long_val"):  # absent: NULL, as the builder's
        if len(sliced[k]) == 0:
            sliced[k] = None
    return sliced


# ---- the sweeps as mcgs_sweep_kernel reads the layout -------------------------------
def _tree64(prod):
    """a chunk's products added by halving strides (32, 16, .. 1), missing lanes
    0.0: the order of a shuffle-down reduction, NOT the kernel's"""
    v = np.zeros(64)
    v[:len(prod)] = prod
    off = 32
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return v[0]


def _colour_sums(lay, part, c, z, mutant):
    """position -> sum of the part's row, for the positions of colour c"""
    s = lay[part]["sliced"]
    c1 = int(lay["color_start"][c + 1])
    sums = {}
    for sl in range(s["color_slice"][c], s["color_slice"][c + 1]):
        p0 = int(s["slice_pos0"][sl])
        lanes = np.arange(min(64, c1 - p0))
        m = s["len"][p0 + lanes]
        base = int(s["slice_ptr"][sl])
        width = int(s["slice_ptr"][sl + 1] - base) // 64
        acc = np.zeros(len(lanes))
        for k in range(width):
            e = base + 64 * k + lanes
            prod = s["val"][e] * z[s["col"][e]]
            live = (m >= 0) if mutant == "pad" else (m > k)
            if mutant == "first" and k == 0:
                acc = np.where(live, prod, acc)
            else:
                acc = np.where(live, acc + prod, acc)
        for lane in lanes[m >= 0]:
            sums[p0 + int(lane)] = acc[lane]
    for l in range(s["color_long"][c], s["color_long"][c + 1]):
        e0, e1 = int(s["long_ptr"][l]), int(s["long_ptr"][l + 1])
        prod = s["long_val"][e0:e1] * z[s["long_col"][e0:e1]]
        acc = np.float64(0.0)
        for e in range(0, e1 - e0, 64):
            if mutant == "pairwise":
                acc = acc + _tree64(prod[e:e + 64])
                continue
            for j, p in enumerate(prod[e:e + 64]):
                acc = p if (mutant == "first" and e + j == 0) else acc + p
        sums[int(s["long_pos"][l])] = acc
    return sums


def sweep(lay, dinv, r, z0, mutant=None):
    """z = M^-1 r on a layout with values (with_values), dinv by ROW, z prefilled
    with z0.  mutant: None, or one deliberately wrong kernel -- "pad" (the
    padding of a slice is multiplied, not skipped), "first" (the sum starts at
    the first product, not at 0.0), "pairwise" (a long row's chunk is added by
    halving strides)."""
    z = np.array(z0, np.float64)
    perm, nc = lay["perm"], lay["num_colors"]
    with np.errstate(all="ignore"):
        for c in range(nc):
            for pos, s in _colour_sums(lay, "before", c, z, mutant).items():
                i = perm[pos]
                z[i] = (r[i] - s) * dinv[i]
        for c in range(nc - 2, -1, -1):
            for pos, t in _colour_sums(lay, "after", c, z, mutant).items():
                i = perm[pos]
                z[i] = z[i] - dinv[i] * t
    return z
