"""The device setup of spmv::SgsPreconditioner restated in numpy, and the small
matrices that reach its edges.  No GPU and no library are needed to import this.

colour_ref    the colouring of spmv_hip_mcgs_color as a SEQUENTIAL greedy in
              descending priority: colour(i) = the smallest colour not worn by
              a neighbour of higher priority, neighbours in B + B^T, B by
              sgs_build.cpp's off_diagonal().  natural: prio(i) = -i; hashed:
              prio(i) = mix64((i + 1) * 0x9E3779B97F4A7C15 mod 2^64), unsigned.
plan_ref      the plan from GIVEN colours: colour-major positions, the two
              parts in CSR over positions (a row's stored entries, symmetric
              storage: then the stable transpose of its column; stable-sorted
              by column), then sgs_layout.slice_part -- the dict
              host.SgsPreconditioner.plan_arrays() returns.
raw_color / raw_build   the two C entries on raw device arrays."""
import ctypes as C

import numpy as np

from sgs_layout import SLICED_KEYS, _McgsPart, slice_part

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
PART_TYPES = dict(color_slice=np.int32, slice_pos0=np.int32, slice_ptr=np.int64,
                  len=np.int32, col=np.int32, val=np.float64,
                  color_long=np.int32, long_pos=np.int32, long_ptr=np.int64,
                  long_col=np.int32, long_val=np.float64)


def mix64(z):
    """splitmix64's finaliser on uint64 arrays (wrapping)"""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def priority_order(n, order):
    """the rows in DESCENDING priority"""
    if order == "natural":
        return np.arange(n)
    h = mix64((np.arange(n, dtype=np.uint64) + np.uint64(1)) * GOLDEN)
    assert len(np.unique(h)) == n  # a bijection: no ties
    return np.argsort(h, kind="stable")[::-1]


def _row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def block_entries(csr, n, symmetric):
    """(rows, cols, vals) of B's entries as a row of the plan lists them: the
    stored off-diagonal entries in storage order; symmetric storage: followed
    by the mirror images of the stored lower entries"""
    rp, ci, va = (np.asarray(a) for a in csr)
    rows = _row_of(rp)
    ci = ci.astype(np.int64)
    if symmetric:
        low = ci < rows
        return (np.concatenate([rows[low], ci[low]]),
                np.concatenate([ci[low], rows[low]]),
                np.concatenate([va[low], va[low]]))
    keep = (ci < n) & (ci != rows)
    return rows[keep], ci[keep], va[keep]


def neighbours(csr, n, symmetric):
    """adjacency lists of B + B^T"""
    r, c, _ = block_entries(csr, n, symmetric)
    a, b = np.concatenate([r, c]), np.concatenate([c, r])
    order = np.argsort(a, kind="stable")
    return np.split(b[order], np.cumsum(np.bincount(a, minlength=n))[:-1])


def colour_ref(csr, n, symmetric, order):
    """-> (colours int32[n], number of colours)"""
    adj = neighbours(csr, n, symmetric)
    colour = np.full(n, -1, np.int64)
    for i in priority_order(n, order):
        worn = set(colour[adj[i]].tolist())  # (-1: of lower priority, not yet)
        c = 0
        while c in worn:
            c += 1
        colour[i] = c
    return colour.astype(np.int32), int(colour.max()) + 1 if n else 0


def is_proper(csr, n, symmetric, colours):
    r, c, _ = block_entries(csr, n, symmetric)
    return not np.any(colours[r] == colours[c])


def diagonal_of(csr, n):
    """Matrix::diagonal's rule: the entries (i, i) added in storage order from
    +0.0"""
    rp, ci, va = (np.asarray(a) for a in csr)
    rows = _row_of(rp)
    d = np.zeros(n)
    on = ci == rows
    np.add.at(d, rows[on], va[on])
    return d


def parts_ref(csr, n, symmetric, colours):
    """-> (perm, color_start, [before, after]), a part = (ptr, col, val) in
    CSR over positions: host.sgs_build's output for the given colours"""
    colours = np.asarray(colours, np.int64)
    nc = int(colours.max()) + 1 if n else 0
    perm = np.argsort(colours, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(colours, minlength=nc))])
    pos_of = np.empty(n, np.int64)
    pos_of[perm] = np.arange(n)
    r, c, v = block_entries(csr, n, symmetric)
    order = np.lexsort((c, pos_of[r]))  # stable: duplicates keep their order
    r, c, v = r[order], c[order], v[order]
    assert not np.any(colours[r] == colours[c])
    parts = []
    for sel in (colours[c] < colours[r], colours[c] > colours[r]):
        ptr = np.concatenate([[0], np.cumsum(np.bincount(pos_of[r[sel]],
                                                         minlength=n))])
        parts.append((ptr.astype(np.int64), c[sel].astype(np.int32), v[sel]))
    return perm, start.astype(np.int32), parts


def plan_ref(csr, n, symmetric, colours, d=None):
    perm, start, parts = parts_ref(csr, n, symmetric, colours)
    d = diagonal_of(csr, n) if d is None else np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        out = dict(perm=perm, color_start=start, dinv=1.0 / d)
    for name, (ptr, col, val) in zip(("before", "after"), parts):
        out[name] = slice_part(start, ptr, col, val)[0]
    return out


def same_plan(got, want):
    """None, or the name of the first array that differs (dinv and the values
    as bits)"""
    for k in ("perm", "color_start"):
        if not np.array_equal(got[k], want[k]):
            return k
    if not np.array_equal(got["dinv"].view(np.int64),
                          np.asarray(want["dinv"], np.float64).view(np.int64)):
        return "dinv"
    for h in ("before", "after"):
        for k in SLICED_KEYS:
            a = np.asarray(got[h][k])
            b = np.asarray(want[h][k]).astype(PART_TYPES[k])
            if a.dtype.kind == "f":
                a, b = a.view(np.int64), b.view(np.int64)
            if a.shape != b.shape or not np.array_equal(a, b):
                return f"{h}.{k}"
    return None


# ---- matrices --------------------------------------------------------------------------
def from_triplets(n, rows, cols, vals):
    """CSR in the order given (stable by row): unsorted columns and duplicates
    stay as they are"""
    rows = np.asarray(rows)
    order = np.argsort(rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), np.asarray(cols)[order].astype(np.int32),
            np.asarray(vals, np.float64)[order])


def _dominant(n, a, b, v):
    """the symmetric matrix with off-diagonal entries v at (a, b) and (b, a),
    strictly diagonally dominant, columns ascending"""
    rows = np.concatenate([a, b, np.arange(n)])
    cols = np.concatenate([b, a, np.arange(n)])
    off = np.bincount(np.concatenate([a, b]), weights=np.abs(np.concatenate([v, v])),
                      minlength=n)
    vals = np.concatenate([v, v, off + 1.0 + 0.25 * np.cos(np.arange(n))])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32), vals[order])


def clique(n=70):
    """every row coupled to every other: n colours -- the first-fit crosses a
    window of 64; with the natural colours row 64 has exactly 64 entries in
    `before` (at the long threshold), row 65 has 65 (beyond it), rows 5 and 4
    the same in `after`"""
    a, b = np.triu_indices(n, 1)
    return _dominant(n, a, b, -(0.5 + 0.3 * np.sin(a * 3.0 + b)))


def lonely_row(n=130):
    """a chain in which row 64 has no off-diagonal entry"""
    a = np.array([i for i in range(n - 1) if i not in (63, 64)])
    return _dominant(n, a, a + 1, -(0.5 + 0.1 * np.cos(a)))


def one_way(n=97):
    """general storage only: a chain plus entries (i, j) whose mirror (j, i) is
    absent, above and below the diagonal -- only the transposed map makes i
    and j neighbours"""
    rp, ci, va = lonely_row(n)
    rows = _row_of(rp)
    extra_r = np.array([3, 90, 40, 41, 64])
    extra_c = np.array([50, 10, 42, 39, 2])
    return from_triplets(n, np.concatenate([rows, extra_r]),
                         np.concatenate([ci, extra_c]),
                         np.concatenate([va, np.full(5, -0.125)]))


def unsorted_duplicates(n=150, seed=3):
    """columns in descending order within every row, and a column stored twice
    in some rows (both copies count, in storage order); symmetric pattern,
    diagonal twice in row 0"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, 400)
    b = rng.integers(0, n, 400)
    ok = a != b
    a, b = np.minimum(a, b)[ok], np.maximum(a, b)[ok]  # duplicates stay
    v = -rng.uniform(0.1, 1.0, len(a))
    rows = np.concatenate([a, b, np.arange(n), [0]])
    cols = np.concatenate([b, a, np.arange(n), [0]])
    vals = np.concatenate([v, v * 0.5, np.full(n, 40.0), [2.5]])
    order = np.lexsort((-cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32), vals[order])


def hand_coloured(sizes=(63, 64, 65, 128)):
    """-> (csr, colours): colour c holds exactly sizes[c] rows, interleaved in
    the natural order; every row is coupled to one or two rows of every other
    colour (a proper colouring by construction), so the slices of 63, 64, 65
    and 128 rows are all full of entries"""
    n = sum(sizes)
    colours = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    colours = colours[np.random.default_rng(11).permutation(n)]
    members = [np.flatnonzero(colours == c) for c in range(len(sizes))]
    a, b = [], []
    for i in range(n):
        for c, m in enumerate(members):
            if c != colours[i]:
                a += [i, i]
                b += [int(m[i % len(m)]), int(m[(7 * i + 1) % len(m)])]
    a, b = np.array(a), np.array(b)
    pairs = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    lo, hi = pairs // n, pairs % n
    return (_dominant(n, lo, hi, -(0.2 + 0.1 * np.sin(lo + 2.0 * hi))),
            colours.astype(np.int32))


def with_ghost_columns(csr, n, ghosts=5):
    """the same rows with entries in `ghosts` further columns >= n appended to
    some rows: a general one-block matrix of n + ghosts columns"""
    rp, ci, va = csr
    rows = _row_of(rp)
    gr = np.arange(0, n, 3)
    return from_triplets(n, np.concatenate([rows, gr]),
                         np.concatenate([ci, n + gr % ghosts]),
                         np.concatenate([va, np.full(len(gr), -0.01)])), n + ghosts


def lower_of(csr):
    """the input of symmetric storage as create_matrix keeps it: strictly lower
    entries, and the diagonal apart -> (csr_lower, diagonal)"""
    rp, ci, va = csr
    n = len(rp) - 1
    rows = _row_of(rp)
    low = ci < rows
    return (from_triplets(n, rows[low], ci[low], va[low]), diagonal_of(csr, n))


# ---- the C entries on raw device arrays -----------------------------------------------
class _Dev:
    """arrays on the device for the time of a call"""

    def __init__(self, exec_):
        self.e, self.ptrs = exec_, []

    def put(self, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        p = self.e.alloc(max(len(a), 1), dtype)
        self.ptrs.append(p)
        if len(a):
            self.e.copy_from_host(p, a)
        return p

    def close(self):
        for p in self.ptrs:
            self.e.free(p)


def export_plan(hip, plan):
    sizes = np.zeros(10, np.int64)
    assert hip.spmv_hip_mcgs_plan_sizes(plan, sizes.ctypes.data) == 0
    n, nc, ns = (int(v) for v in sizes[:3])
    out = dict(perm=np.zeros(n, np.int32), color_start=np.zeros(nc + 1, np.int32),
               dinv=np.zeros(n), bytes=int(sizes[9]))
    structs = []
    for h, name in enumerate(("before", "after")):
        ent, nl, lent = (int(v) for v in sizes[3 + 3 * h:6 + 3 * h])
        count = dict(color_slice=nc + 1, slice_pos0=ns, slice_ptr=ns + 1, len=n,
                     col=ent, val=ent, color_long=nc + 1, long_pos=nl,
                     long_ptr=nl + 1, long_col=lent, long_val=lent)
        out[name] = {k: np.zeros(count[k], PART_TYPES[k]) for k in SLICED_KEYS}
        s = _McgsPart()
        for k in SLICED_KEYS:
            setattr(s, k, out[name][k].ctypes.data)
        structs.append(s)
    assert hip.spmv_hip_mcgs_plan_export(
        plan, out["perm"].ctypes.data, out["color_start"].ctypes.data,
        out["dinv"].ctypes.data, C.byref(structs[0]), C.byref(structs[1])) == 0
    return out


def raw_color(hip, exec_, csr, n, num_cols, symmetric, order):
    """spmv_hip_mcgs_color -> (return code, colours, number, rounds)"""
    rp, ci, _ = csr
    dev = _Dev(exec_)
    try:
        d_rp, d_ci = dev.put(rp, np.int32), dev.put(ci, np.int32)
        d_col = dev.put(np.full(n, -7), np.int32)
        nc, rounds = C.c_int(), C.c_int()
        rc = hip.spmv_hip_mcgs_color(exec_.context, n, num_cols, len(ci), d_rp,
                                     d_ci, int(symmetric),
                                     1 if order == "natural" else 0, d_col,
                                     C.byref(nc), C.byref(rounds), None)
        colours = exec_.copy_to_host(d_col, n, np.int32) if rc == 0 else None
        return rc, colours, nc.value, rounds.value
    finally:
        dev.close()


def raw_build(hip, exec_, csr, n, num_cols, symmetric, colours, num_colors=None,
              diagonal=None, threshold=64):
    """spmv_hip_mcgs_plan_build -> (return code, info[4], exported arrays)"""
    rp, ci, va = csr
    dev = _Dev(exec_)
    try:
        d_rp, d_ci = dev.put(rp, np.int32), dev.put(ci, np.int32)
        d_va = dev.put(va, np.float64)
        d_di = dev.put(diagonal, np.float64) if diagonal is not None else None
        d_col = dev.put(colours, np.int32)
        nc = int(np.max(colours)) + 1 if num_colors is None else num_colors
        plan, info = C.c_void_p(), np.full(4, -1, np.int64)
        rc = hip.spmv_hip_mcgs_plan_build(
            exec_.context, n, num_cols, len(ci), d_rp, d_ci, d_va, d_di,
            int(symmetric), d_col, nc, threshold, C.byref(plan),
            info.ctypes.data, None)
        if rc != 0:
            assert not plan.value
            return rc, info, None
        try:
            return rc, info, export_plan(hip, plan)
        finally:
            assert hip.spmv_hip_mcgs_plan_destroy(plan) == 0
    finally:
        dev.close()
