"""Thin Python handles over the C ABI of libspmv_hip.so (include/spmv_hip.h).

Harness plumbing for tests/ and bench.py: owns contexts, device buffers,
streams and plans, and forwards every compute call 1:1 to the C ABI.  No
arithmetic happens in Python and nothing here falls back to numpy/torch.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import call

ALGO_AUTO, ALGO_ROWBLOCK, ALGO_VECTOR, ALGO_SCALAR, ALGO_ROWLIST = 0, 1, 2, 3, 4
PART_ALL, PART_LOCAL, PART_REMOTE, PART_LOCAL_LOWER = 0, 1, 2, 3


def device_count():
    n = C.c_int()
    call("spmv_hip_device_count", C.byref(n))
    return n.value


class Buffer:
    """A device allocation made through spmv_hip_alloc."""

    def __init__(self, ctx, nbytes, dtype=None, count=None):
        self.ctx, self.nbytes, self.dtype, self.count = ctx, int(nbytes), dtype, count
        p = C.c_void_p()
        call("spmv_hip_alloc", ctx.h, self.nbytes, C.byref(p))
        self.ptr = p.value  # None for a zero-byte allocation

    def free(self):
        # (freed = True: given back already, the address kept as a token --
        # CsrBlock.release_matrix)
        if self.ptr and not getattr(self, "freed", False):
            call("spmv_hip_free", self.ctx.h, self.ptr)
        self.ptr = None

    def numpy(self, count=None, offset=0):
        """Blocking device->host copy of `count` elements from `offset`."""
        count = self.count - offset if count is None else count
        out = np.empty(count, self.dtype)
        if count:
            isz = np.dtype(self.dtype).itemsize
            call("spmv_hip_copy_d2h_async", self.ctx.h,
                 out.ctypes.data_as(C.c_void_p), self.ptr + offset * isz,
                 count * isz, None)
            self.ctx.stream_sync()
        return out

    def at(self, offset):
        return self.ptr + offset * np.dtype(self.dtype).itemsize

    def write(self, arr):
        """Blocking host->device copy INTO this allocation (same length)."""
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.size == self.count
        if self.nbytes:
            call("spmv_hip_copy_h2d_async", self.ctx.h, self.ptr,
                 arr.ctypes.data_as(C.c_void_p), self.nbytes, None)
            self.ctx.stream_sync()


class Context:
    """spmv_hip_ctx: one GPU."""

    def __init__(self, device_id=0):
        h = C.c_void_p()
        call("spmv_hip_ctx_create", device_id, C.byref(h))
        self.h = h
        self.device_id = device_id

    def close(self):
        if self.h:
            call("spmv_hip_ctx_destroy", self.h)
            self.h = None

    @property
    def num_cus(self):
        n = C.c_int()
        call("spmv_hip_num_cus", self.h, C.byref(n))
        return n.value

    @property
    def dot_partials_len(self):
        n = C.c_int()
        call("spmv_hip_dot_partials_len", self.h, C.byref(n))
        return n.value

    # -- memory ---------------------------------------------------------
    def empty(self, count, dtype):
        return Buffer(self, int(count) * np.dtype(dtype).itemsize, dtype,
                      int(count))

    def zeros(self, count, dtype):
        b = self.empty(count, dtype)
        if b.nbytes:
            call("spmv_hip_memset_async", self.h, b.ptr, 0, b.nbytes, None)
        return b

    def upload(self, arr, dtype=None):
        arr = np.ascontiguousarray(arr, dtype=dtype)
        b = self.empty(arr.size, arr.dtype)
        if b.nbytes:
            call("spmv_hip_copy_h2d_async", self.h, b.ptr,
                 arr.ctypes.data_as(C.c_void_p), b.nbytes, None)
            self.stream_sync()  # arr may be a temporary
        return b

    def copy_h2d(self, dst_ptr, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            call("spmv_hip_copy_h2d_async", self.h, dst_ptr,
                 arr.ctypes.data_as(C.c_void_p), arr.nbytes, None)
            self.stream_sync()

    def copy(self, dst, src, nbytes, stream=None):
        call("spmv_hip_copy_d2d_async", self.h, dst, src, nbytes, stream)

    def memset(self, ptr, value, nbytes, stream=None):
        call("spmv_hip_memset_async", self.h, ptr, value, nbytes, stream)

    # -- streams / events -------------------------------------------------
    def set_option(self, key, value):
        call("spmv_hip_ctx_set_option", self.h, key.encode(), int(value))

    def synchronize(self):
        call("spmv_hip_synchronize", self.h)

    def stream_sync(self, stream=None):
        call("spmv_hip_stream_synchronize", self.h, stream)

    def stream_create(self):
        s = C.c_void_p()
        call("spmv_hip_stream_create", self.h, C.byref(s))
        return s

    def stream_destroy(self, s):
        call("spmv_hip_stream_destroy", self.h, s)

    def set_stream(self, s):
        call("spmv_hip_set_stream", self.h, s)

    def event_create(self, timing=True):
        e = C.c_void_p()
        call("spmv_hip_event_create", self.h, int(timing), C.byref(e))
        return e

    def event_destroy(self, e):
        call("spmv_hip_event_destroy", self.h, e)

    def event_record(self, e, stream=None):
        call("spmv_hip_event_record", self.h, e, stream)

    def event_sync(self, e):
        call("spmv_hip_event_synchronize", self.h, e)

    def elapsed_ms(self, e0, e1):
        ms = C.c_float()
        call("spmv_hip_event_elapsed_ms", self.h, e0, e1, C.byref(ms))
        return ms.value

    # -- kernels ------------------------------------------------------------
    def gather(self, indices, x, out, n, stream=None):
        call("spmv_hip_gather_f64", self.h, n, indices.ptr, x.ptr, out.ptr,
             stream)

    def scatter_add(self, indices, x, out, n, stream=None, dtype=np.float64):
        fn = ("spmv_hip_scatter_add_f64" if dtype == np.float64
              else "spmv_hip_scatter_add_f32")
        call(fn, self.h, n, indices.ptr, x.ptr, out.ptr, stream)

    def fill_gaussian(self, N, i_begin, count, x_ptr, stream=None):
        call("spmv_hip_fill_gaussian_f64", self.h, N, i_begin, count, x_ptr,
             stream)

    def fill_const(self, count, value, x_ptr, stream=None):
        call("spmv_hip_fill_const_f64", self.h, count, float(value), x_ptr,
             stream)

    def dot(self, n, x_ptr, y_ptr):
        """Deterministic two-stage dot product; blocking, returns a float."""
        part = self.empty(self.dot_partials_len, np.float64)
        res = self.empty(1, np.float64)
        call("spmv_hip_dot_partial_f64", self.h, n, x_ptr, y_ptr, part.ptr,
             None)
        call("spmv_hip_reduce_partials_f64", self.h, part.ptr, res.ptr, None)
        v = float(res.numpy()[0])
        part.free()
        res.free()
        return v


class CsrBlock:
    """Device-resident CSR block + its SpMV plan (what CSRMatrix owns,
    spmv/csr_matrix.cpp:22-70)."""

    def __init__(self, ctx, nrows, ncols, rowptr, colind, values,
                 diagonal=None, symmetric=False, algo=ALGO_AUTO,
                 dtype=np.float64):
        self.ctx, self.nrows, self.ncols = ctx, int(nrows), int(ncols)
        self.symmetric, self.dtype = bool(symmetric), np.dtype(dtype)
        self.owned = []

        def dev(a, dt):
            if a is None or isinstance(a, Buffer):
                return a
            b = ctx.upload(a, dt)
            self.owned.append(b)
            return b
        self.nnz = (values.count if isinstance(values, Buffer)
                    else (0 if values is None else len(values)))
        if self.nnz == 0:  # csr_matrix.cpp:34: arrays are never allocated
            rowptr = colind = values = None
        self.rowptr, self.colind = dev(rowptr, np.int32), dev(colind, np.int32)
        self.values, self.diagonal = dev(values, dtype), dev(diagonal, dtype)
        plan = C.c_void_p()
        call("spmv_hip_csr_plan_create", ctx.h, self.nrows, self.ncols,
             self.nnz, _p(self.rowptr), _p(self.colind), int(self.symmetric),
             algo, C.byref(plan))
        self.plan = plan

    def bake(self, drop=False):
        """spmv_hip_csr_plan_bake_values_*: the plan's own copy of the values
        by offset (symmetric diagonal form)."""
        name = ("spmv_hip_csr_plan_bake_values_f64" if self.dtype == np.float64
                else "spmv_hip_csr_plan_bake_values_f32")
        call(name, self.ctx.h, self.plan, None if drop else _p(self.values),
             None if drop else _p(self.diagonal), None)

    def values_changed(self):
        """spmv_hip_csr_plan_values_changed: the baked arrays were rewritten in
        place; refresh the plan's copies."""
        call("spmv_hip_csr_plan_values_changed", self.ctx.h, self.plan, None)

    def owns_matrix(self):
        """spmv_hip_csr_plan_owns_matrix: bit 0 = colind, bit 1 = values are no
        longer read by the plan's kernel"""
        m = C.c_int()
        call("spmv_hip_csr_plan_owns_matrix", self.plan, C.byref(m))
        return m.value

    def release_matrix(self):
        """spmv_hip_csr_plan_release_matrix + free this block's device copies of
        the arrays the plan owns (the buffers' addresses stay as the tokens the
        launches compare).  Returns the mask released."""
        m = self.owns_matrix()
        if m == 3:
            call("spmv_hip_csr_plan_release_matrix", self.plan, m)
            self.ctx.synchronize()
            for buf in (self.colind, self.values):
                call("spmv_hip_free", self.ctx.h, buf.ptr)
                buf.freed = True
            return m
        return 0

    def set(self, key, value):
        call("spmv_hip_csr_plan_set", self.plan, key.encode(), int(value))

    def get(self, key):
        v = C.c_int()
        call("spmv_hip_csr_plan_get", self.plan, key.encode(), C.byref(v))
        return v.value

    @property
    def algo(self):
        a = C.c_int()
        call("spmv_hip_csr_plan_algo", self.plan, C.byref(a))
        return a.value

    def mult(self, alpha, x_ptr, beta, y_ptr, dot_partials=None, stream=None):
        if self.dtype == np.float64:
            call("spmv_hip_csr_spmv_f64", self.ctx.h, self.plan, self.nrows,
                 self.ncols, self.nnz, _p(self.rowptr), _p(self.colind),
                 _p(self.values), _p(self.diagonal), float(alpha), x_ptr,
                 float(beta), y_ptr, dot_partials, stream)
        else:
            assert dot_partials is None
            call("spmv_hip_csr_spmv_f32", self.ctx.h, self.plan, self.nrows,
                 self.ncols, self.nnz, _p(self.rowptr), _p(self.colind),
                 _p(self.values), _p(self.diagonal), float(alpha), x_ptr,
                 float(beta), y_ptr, stream)

    def transpose(self, col_begin=0, col_end=None, stream=None):
        """spmv_hip_csr_plan_build_transpose over the columns [col_begin,
        col_end) (default: all of them)."""
        col_end = self.ncols if col_end is None else col_end
        call("spmv_hip_csr_plan_build_transpose", self.ctx.h, self.plan,
             _p(self.rowptr), _p(self.colind), _p(self.values),
             self.dtype.itemsize, int(col_begin), int(col_end), stream)

    def multt(self, alpha, x_ptr, beta, y_ptr, values=None, stream=None):
        """spmv_hip_csr_spmvt_*: y = alpha A^T x + beta y over the range of
        transpose(); `values`: another device array of the block's values
        (the in-place kernel runs on it)."""
        v = _p(self.values) if values is None else values
        name = ("spmv_hip_csr_spmvt_f64" if self.dtype == np.float64
                else "spmv_hip_csr_spmvt_f32")
        call(name, self.ctx.h, self.plan, self.nrows, self.ncols, self.nnz,
             _p(self.rowptr), _p(self.colind), v, float(alpha), x_ptr,
             float(beta), y_ptr, stream)

    def multm(self, alpha, x_ptr, beta, y_ptr, k, values=None, mixed=False,
              stream=None):
        """spmv_hip_csr_spmm_*: Y = alpha A X + beta Y for k INTERLEAVED vectors
        (element (i, c) at X[i * k + c]; X: ncols * k, Y: nrows * k).  `values`:
        another device array of the block's values; mixed=True: `values` is an
        fp32 copy under fp64 vectors (fp64 general blocks)."""
        v = _p(self.values) if values is None else values
        if mixed:
            assert self.dtype == np.float64 and values is not None
            name, diag = "spmv_hip_csr_spmm_f32f64", None
        else:
            name = ("spmv_hip_csr_spmm_f64" if self.dtype == np.float64
                    else "spmv_hip_csr_spmm_f32")
            diag = _p(self.diagonal)
        call(name, self.ctx.h, self.plan, self.nrows, self.ncols, self.nnz,
             _p(self.rowptr), _p(self.colind), v, diag, float(alpha), x_ptr,
             float(beta), y_ptr, int(k), stream)

    def free(self):
        if self.plan:
            call("spmv_hip_csr_plan_destroy", self.plan)
            self.plan = None
        for b in self.owned:
            b.free()
        self.owned = []


def _p(buf):
    return None if buf is None else buf.ptr


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def interleave(ctx, n, k, cols_ptr, out_ptr, ld=None, dtype=np.float64,
               stream=None):
    """k columns (column c at cols + c * ld, ld >= n) -> the interleaved n x k
    block: out[i * k + c] = cols[c * ld + i]"""
    call("spmv_hip_interleave_" + _suffix(dtype), ctx.h, int(n), int(k),
         cols_ptr, int(n if ld is None else ld), out_ptr, stream)


def deinterleave(ctx, n, k, in_ptr, cols_ptr, ld=None, dtype=np.float64,
                 stream=None):
    """the interleaved n x k block -> k columns: cols[c * ld + i] = in[i * k + c]"""
    call("spmv_hip_deinterleave_" + _suffix(dtype), ctx.h, int(n), int(k), in_ptr,
         int(n if ld is None else ld), cols_ptr, stream)


def gather_block(ctx, num_indices, indices_ptr, k, in_ptr, out_ptr,
                 dtype=np.float64, stream=None):
    """out[g * k + c] = in[indices[g] * k + c]"""
    call("spmv_hip_gather_block_" + _suffix(dtype), ctx.h, int(num_indices),
         indices_ptr, int(k), in_ptr, out_ptr, stream)


def poisson3d_block(ctx, n, row_begin, row_end, part, with_diagonal=False,
                    algo=ALGO_AUTO):
    """Generate a Poisson CSR block directly on the device
    (spmv_hip_poisson3d_count / _fill_f64)."""
    nrows = row_end - row_begin
    gb, ga = C.c_int64(), C.c_int64()
    call("spmv_hip_poisson3d_ghosts", n, row_begin, row_end, C.byref(gb),
         C.byref(ga))
    ncols = nrows + gb.value + ga.value
    if part in (PART_LOCAL, PART_LOCAL_LOWER):
        ncols_blk = nrows if part == PART_LOCAL else ncols
    else:
        ncols_blk = ncols
    rowptr = ctx.empty(nrows + 1, np.int32)
    nnz = C.c_int64()
    call("spmv_hip_poisson3d_count", ctx.h, n, row_begin, row_end, part,
         rowptr.ptr, C.byref(nnz), None)
    colind = ctx.empty(nnz.value, np.int32)
    values = ctx.empty(nnz.value, np.float64)
    diag = ctx.empty(nrows, np.float64) if with_diagonal else None
    call("spmv_hip_poisson3d_fill_f64", ctx.h, n, row_begin, row_end, part,
         rowptr.ptr, colind.ptr, values.ptr, _p(diag), None)
    blk = CsrBlock(ctx, nrows, ncols_blk, rowptr, colind, values, diag,
                   symmetric=(part == PART_LOCAL_LOWER), algo=algo)
    blk.owned += [b for b in (rowptr, colind, values, diag) if b is not None]
    blk.ghosts_below, blk.ghosts_above = gb.value, ga.value
    return blk


class AmgTailLevel(C.Structure):
    """spmv_hip_amg_tail_level: device pointers but for a, b (host)"""
    _fields_ = [("rows", C.c_int32), ("lanes_per_row", C.c_int32),
                ("nnz", C.c_int64), ("rowptr", C.c_void_p),
                ("colind", C.c_void_p), ("values", C.c_void_p),
                ("dinv", C.c_void_p), ("r", C.c_void_p), ("w", C.c_void_p),
                ("dd", C.c_void_p), ("z", C.c_void_p), ("step", C.c_void_p),
                ("a", C.c_void_p), ("b", C.c_void_p)]


class AmgTailHost(C.Structure):
    """spmv_hip_amg_tail_host"""
    _fields_ = [("num_levels", C.c_int32), ("smooth_degree", C.c_int32),
                ("coarse_degree", C.c_int32), ("coarse_scale", C.c_double),
                ("levels", C.POINTER(AmgTailLevel))]


class AmgTail:
    """spmv_hip_amg_tail: the levels of an AMG cycle that one launch runs.
    `ctx`: a spmv_hip_ctx pointer.  levels: dicts with the fields of
    AmgTailLevel; a, b: the level's Chebyshev coefficients (numpy).  The
    arrays and steps must outlive the handle.  Raises _lib.SpmvHipError
    (EINVAL: an index out of range, a NULL or unaligned vector, a step that
    does not fit the levels' rows) without launching anything."""

    def __init__(self, ctx, levels, smooth_degree, coarse_degree, coarse_scale):
        self.ctx, self.h = ctx, None
        keep, arr = [], (AmgTailLevel * len(levels))()
        for d, lv in zip(arr, levels):
            for k, v in lv.items():
                if k in ("a", "b"):
                    v = np.ascontiguousarray(v, np.float64)
                    keep.append(v)
                    v = v.ctypes.data
                elif hasattr(v, "value"):  # a c_void_p handle
                    v = v.value
                setattr(d, k, v)
        desc = AmgTailHost(len(levels), smooth_degree, coarse_degree,
                           coarse_scale, arr)
        h = C.c_void_p()
        call("spmv_hip_amg_tail_create", ctx, C.byref(desc), C.byref(h))
        self.h = h

    def set_coefficients(self, level, a, b):
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        call("spmv_hip_amg_tail_set_coefficients", self.h, int(level),
             a.ctypes.data, b.ctypes.data)

    def bytes(self):
        n = C.c_int64()
        call("spmv_hip_amg_tail_bytes", self.h, C.byref(n))
        return n.value

    def run(self, stream=None):
        call("spmv_hip_amg_tail_run_f64", self.ctx, self.h, stream)

    def close(self):
        if self.h:
            call("spmv_hip_amg_tail_destroy", self.h)
            self.h = None


class AmgExport(C.Structure):
    """spmv_hip_amg_export: host pointers, NULL skipped"""
    _fields_ = [("agg", C.c_void_p), ("member_ptr", C.c_void_p),
                ("member", C.c_void_p), ("src_ptr", C.c_void_p),
                ("src", C.c_void_p), ("xrow_ptr", C.c_void_p),
                ("xrow_src", C.c_void_p)]


AMG_HASHED, AMG_NATURAL = 0, 1
_AMG_EXPORT = (("agg", np.int32), ("member_ptr", np.int32), ("member", np.int32),
               ("src_ptr", np.int64), ("src", np.int32), ("xrow_ptr", np.int64),
               ("xrow_src", np.int32))


def amg_aggregate(ctx, num_rows, num_cols, nnz, rowptr, colind, values, diagonal,
                  symmetric, theta, order, agg):
    """spmv_hip_amg_aggregate on DEVICE pointers (`ctx`: a spmv_hip_ctx pointer;
    agg: num_rows ints) -> (n_agg, (rounds of pass 1, of pass 3), info).  Raises
    _lib.SpmvHipError; .info holds the words then."""
    n_agg, rounds, info = C.c_int32(), (C.c_int * 2)(), np.zeros(4, np.int64)
    try:
        call("spmv_hip_amg_aggregate", ctx, num_rows, num_cols, nnz, rowptr,
             colind, values, diagonal, int(bool(symmetric)), float(theta),
             int(order), agg, C.byref(n_agg), rounds, info.ctypes.data, None)
    except _lib.SpmvHipError as e:
        e.info = info
        raise
    return n_agg.value, (int(rounds[0]), int(rounds[1])), info


class AmgBuiltPlan:
    """spmv_hip_amg_plan made by spmv_hip_amg_plan_build from DEVICE arrays and
    a DEVICE agg.  coarse_rowptr: n_agg + 1 ints the caller allocated on the
    device; .coarse_colind (a device address, freed by close()) and .coarse_nnz
    are returned.  A failure raises _lib.SpmvHipError with .info and leaves
    nothing allocated."""

    def __init__(self, ctx, num_rows, num_cols, nnz, rowptr, colind, symmetric,
                 agg, n_agg, coarse_rowptr):
        self.ctx, self.h, self.coarse_colind = ctx, None, None
        h, ci, nnz_c = C.c_void_p(), C.c_void_p(), C.c_int64()
        self.info = np.zeros(4, np.int64)
        try:
            call("spmv_hip_amg_plan_build", ctx, num_rows, num_cols, nnz, rowptr,
                 colind, int(bool(symmetric)), agg, n_agg, coarse_rowptr,
                 C.byref(ci), C.byref(nnz_c), C.byref(h), self.info.ctypes.data,
                 None)
        except _lib.SpmvHipError as e:
            e.info = self.info
            raise
        self.h, self.coarse_colind, self.coarse_nnz = h, ci.value, nnz_c.value

    def sizes(self):
        return plan_sizes(self.h)

    def export(self):
        return plan_export(self.h)

    def bytes(self):
        n = C.c_int64()
        call("spmv_hip_amg_plan_bytes", self.h, C.byref(n))
        return n.value

    def close(self):
        if self.coarse_colind:
            call("spmv_hip_free", self.ctx, self.coarse_colind)
            self.coarse_colind = None
        if self.h:
            call("spmv_hip_amg_plan_destroy", self.h)
            self.h = None


def plan_sizes(plan):
    """spmv_hip_amg_plan_sizes of a plan of either builder -> dict"""
    s = np.zeros(9, np.int64)
    call("spmv_hip_amg_plan_sizes", plan, s.ctypes.data)
    keys = ("fine_rows", "coarse_rows", "num_values", "num_diagonal",
            "coarse_nnz", "src_count", "has_xrow", "xrow_count", "bytes")
    return dict(zip(keys, (int(v) for v in s)))


def plan_export(plan):
    """spmv_hip_amg_plan_export of a plan of either builder -> dict of numpy
    arrays (those the plan has)"""
    s = plan_sizes(plan)
    n, nc = s["fine_rows"], s["coarse_rows"]
    size = dict(agg=n, member_ptr=nc + 1, member=n, src_ptr=s["coarse_nnz"] + 1,
                src=s["src_count"]) if nc else {}
    if s["has_xrow"]:
        size.update(xrow_ptr=n + 1, xrow_src=s["xrow_count"])
    out = {k: np.zeros(size[k], t) for k, t in _AMG_EXPORT if k in size}
    ex = AmgExport(*[out[k].ctypes.data if k in out else None
                     for k, _ in _AMG_EXPORT])
    call("spmv_hip_amg_plan_export", plan, C.byref(ex))
    return out
