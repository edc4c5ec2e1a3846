"""GPU tests of every SpMV plan form on Inf, NaN, signed zeros, overflowing
partial sums and subnormals (recipes S1 ... S5 of special_values.py), against
the numpy restatement of the reference loops under same_bits: NaN as a class,
every other result bit for bit -- so an absent entry, a padded slot or a clamped
load that is multiplied instead of skipped (0 * Inf), a mask in the wrong place
(a lost NaN), a sum started at the first product (-0.0), another summation
order (a finite number where the loop overflows) all show.  Each case is the
smallest one the form's own test uses, and asserts the same plan keys.
test_special_values_host.py holds the recipes to their targets on the CPU."""
import numpy as np
import pytest

import special_values as sv
from spmv_amd import _lib, hip
from util import U, abs_bound

pytestmark = pytest.mark.gpu

ALL = ("S1", "S2", "S3", "S4", "S5")
GHOST = ("G0", "G1", "G2")   # ncols > nrows: the poison only in the ghost range
DOT = ("S1", "S2") + GHOST   # the recipes that also request the fused dot
ENOTSUP = -3


def _context(**options):
    c = hip.Context(0)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def _bake(blk):
    """plan_bake_values; an LX plan answers ENOTSUP beside its narrowed copy"""
    name = ("spmv_hip_csr_plan_bake_values_f64" if blk.dtype == np.float64
            else "spmv_hip_csr_plan_bake_values_f32")
    rc = getattr(_lib.hip, name)(blk.ctx.h, blk.plan, blk.values.ptr,
                                 None if blk.diagonal is None else blk.diagonal.ptr,
                                 None)
    assert rc in (0, ENOTSUP), rc


def _exact32(d):
    """the recipe's data with values that are exact in fp32"""
    va = d.va.astype(np.float32).astype(np.float64)
    return sv.Data(d.name, va, d.x.copy(), d.y0.copy(), d.ab,
                   None if d.diag is None else d.diag.copy())


def _check_dot(part, d, y_ref, tag, rtol=1e-11):
    """NaN exactly when x[:N] . y_ref is NaN, else the same infinity, else
    within the tolerance of the forms' own tests (1e-11 (|x| . |y| + 1), the
    widest of them: test_gpu_sjds.py)"""
    with np.errstate(all="ignore"):
        got = float(np.sum(part.numpy()))
    N = len(y_ref)
    want = sv.want_dot(d, N, y_ref)
    if np.isnan(want):
        assert np.isnan(got), (tag, got)
    elif np.isinf(want):
        assert got == want, (tag, got, want)
    else:
        scale = float(np.abs(d.x[:N]) @ np.abs(y_ref)) + 1.0
        assert abs(got - want) <= rtol * scale, (tag, got, want)


def _run(ctx, p, keys, knobs=(dict(),), recipes=ALL, dtype=np.float64,
         algo=hip.ALGO_ROWBLOCK, setup=None, dot=False, exact32=False,
         mixed=None, reset=None):
    """One plan form on one pattern: every recipe, every (alpha, beta) of the
    recipe, every knob setting; `keys`: plan key -> value asserted after
    `setup` (the form was taken).  mixed: the key that shows the baked fp32
    copy -- the f32f64 product on the fp32-rounded values."""
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    for recipe in recipes:
        d = p.data(recipe, dtype)
        if exact32 and recipe in ("S1", "S2", "S3"):
            d = _exact32(d)
        va = d.va
        if mixed:
            va32 = va if va.dtype == np.float32 else va.astype(np.float32)
            va = va32.astype(np.float64)
            d = sv.Data(d.name, va, d.x.copy(), d.y0.copy(), d.ab)
        if dot:
            assert p.ncols >= p.N  # (the fused dot reads x[i] of every row)
        blk = hip.CsrBlock(ctx, p.N, p.ncols, p.rp, p.ci, va, d.diag, p.sym,
                           hip.ALGO_AUTO if p.sym else algo, dtype)
        if setup:
            setup(blk)
        if mixed:
            d32 = ctx.upload(va32, np.float32)
            if mixed != "none":  # ("none": the CSR-order kernels, nothing baked)
                hip.call("spmv_hip_csr_plan_bake_values_f32f64", ctx.h, blk.plan,
                         d32.ptr, None)
                assert blk.get(mixed) == 1, (recipe, mixed)
        for k, v in keys.items():
            if k == "algo":
                assert blk.algo == v, (recipe, k)
            elif not (k == "lx_v32" and recipe in ("S4", "S5")):
                assert blk.get(k) == v, (recipe, k, blk.get(k))
        dx = ctx.upload(d.x, dtype)
        for alpha, beta in d.ab:
            y_ref = p.ref(d, alpha, beta)
            for kn in knobs:
                for k, v in kn.items():
                    if not (k == "lx_v32" and recipe in ("S4", "S5")):
                        blk.set(k, v)
                dy = ctx.upload(np.full(p.N, np.nan, dtype) if beta == 0 else d.y0,
                                dtype)
                use_dot = (dot and recipe in DOT and beta == 0
                           and dtype == np.float64)
                if mixed:
                    hip.call("spmv_hip_csr_spmv_f32f64", ctx.h, blk.plan, p.N,
                             p.ncols, blk.nnz, blk.rowptr.ptr, blk.colind.ptr,
                             d32.ptr, float(alpha), dx.ptr, float(beta), dy.ptr,
                             part.ptr if use_dot else None, None)
                else:
                    blk.mult(alpha, dx.ptr, beta, dy.ptr,
                             dot_partials=part.ptr if use_dot else None)
                y = dy.numpy()
                dy.free()
                tag = (recipe, alpha, beta, kn)
                assert sv.same_bits(y, y_ref), (
                    tag, np.flatnonzero(sv.bits(y) != sv.bits(y_ref))[:8])
                if use_dot:
                    _check_dot(part, d, y_ref, tag)
            for k, v in (reset or {}).items():
                blk.set(k, v)
        dx.free()
        if mixed:
            d32.free()
        blk.free()
    part.free()


@pytest.fixture(scope="module")
def P():
    return sv.patterns()


# ---------------------------------------------------------------------------
# General storage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("algo", [hip.ALGO_SCALAR, hip.ALGO_ROWBLOCK, hip.ALGO_ROWLIST])
def test_gather_kernels(ctx, P, algo, dtype):
    """513 x 300 and 513 x 513, empty rows, one row of 3000 entries; 600 x 900:
    the shape of a remote block, the poison also in the ghost range alone.
    ROWLIST: with plan_set "rowlist_exact" (the loop's bits at beta == 1 too;
    the default: test_rowlist_at_beta_one_keeps_rows_without_entries)."""
    keys = dict(algo=algo, lat=0, lx=0, xw=0, sjds=0)
    knobs = (dict(rowlist_exact=1),) if algo == hip.ALGO_ROWLIST else (dict(),)
    _run(ctx, P["ragged"], keys, algo=algo, dtype=dtype, knobs=knobs)
    _run(ctx, P["ragged_sq"], keys, algo=algo, dtype=dtype, knobs=knobs, dot=True)
    _run(ctx, P["remote"], keys, algo=algo, dtype=dtype, knobs=knobs, dot=True,
         recipes=ALL + GHOST)


def _rowlist_default_ref(p, d, alpha, beta):
    """the loop, but for the documented difference (spmv_hip.h): at beta == 1
    ROWLIST leaves a row without entries as it is"""
    y = p.ref(d, alpha, beta).copy()
    if beta == 1:
        empty = np.diff(p.rp) == 0
        y[empty] = d.y0[empty]
    return y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rowlist_at_beta_one_keeps_rows_without_entries(ctx, P, dtype):
    """The default (rowlist_exact = 0): no pass over all rows at beta == 1, so a
    -0.0 in a row without entries stays -0.0 where the loop's + alpha*0 gives
    +0.0; every other row, and every other beta, has the loop's bits."""
    for name in ("ragged", "remote"):
        p = P[name]
        for recipe in ("S1", "S3"):
            d = p.data(recipe, dtype)
            blk = hip.CsrBlock(ctx, p.N, p.ncols, p.rp, p.ci, d.va, None, False,
                               hip.ALGO_ROWLIST, dtype)
            assert blk.algo == hip.ALGO_ROWLIST and blk.get("rowlist_exact") == 0
            dx = ctx.upload(d.x, dtype)
            differs = False
            for alpha, beta in d.ab:
                dy = ctx.upload(np.full(p.N, np.nan, dtype) if beta == 0 else d.y0,
                                dtype)
                blk.mult(alpha, dx.ptr, beta, dy.ptr)
                y = dy.numpy()
                dy.free()
                want = _rowlist_default_ref(p, d, alpha, beta)
                assert sv.same_bits(y, want), (name, recipe, alpha, beta)
                differs |= not sv.same_bits(want, p.ref(d, alpha, beta))
            if recipe == "S3":  # the difference exists, and only there
                assert differs, name
            dx.free()
            blk.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_block_without_entries(ctx, dtype):
    """num_non_zeros == 0: every row is the loop's alpha*0 + beta*out, alpha*0
    itself at beta == 0 (out never read) -- spmv and spmm"""
    n = 7
    y0 = np.array([0.0, -0.0, 1.0, -2.5, np.inf, np.nan, -0.0], dtype)
    for alpha in (1.0, -1.0, 2.0):
        for beta in (0.0, 1.0, -0.5):
            with np.errstate(all="ignore"):
                want = np.full(n, dtype(alpha) * dtype(0))
                if beta != 0:
                    want = want + dtype(beta) * y0
            blk = hip.CsrBlock(ctx, n, 3, None, None, None, dtype=dtype)
            dx = ctx.upload(np.ones(3, dtype), dtype)
            dy = ctx.upload(np.full(n, np.nan, dtype) if beta == 0 else y0, dtype)
            blk.mult(alpha, dx.ptr, beta, dy.ptr)
            assert sv.same_bits(dy.numpy(), want), (alpha, beta)
            dy.free()
            k = 2
            dX = ctx.upload(np.ones(3 * k, dtype), dtype)
            Y0 = np.repeat(y0, k)
            dY = ctx.upload(np.full(n * k, np.nan, dtype) if beta == 0 else Y0, dtype)
            blk.multm(alpha, dX.ptr, beta, dY.ptr, k)
            ctx.synchronize()
            assert sv.same_bits(dY.numpy(), np.repeat(want, k)), (alpha, beta, "spmm")
            for b in (dx, dX, dY):
                b.free()
            blk.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice_form(P, dtype):
    ctx = _context(lat_min_nnz=0, lx_min_nnz=0, const_diagonals=0)
    for name in ("poisson9", "eight"):
        _run(ctx, P[name], dict(lat=1, lx=0),
             knobs=(dict(nontemporal=1), dict(nontemporal=0)), dtype=dtype, dot=True)
    _run(ctx, P["poisson16"], dict(lat=1, lat_chain=1),
         knobs=(dict(lat_chain=1), dict(lat_chain=0)), dtype=dtype, dot=True)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lx_forms(P, dtype):
    ctx = _context(lx_min_nnz=0)
    # the DMA kernel and the register-staged kernel on the same layout; row
    # blocks of scattered columns stay direct
    _run(ctx, P["banded"], dict(lx=1, lxw=1, lat=0),
         knobs=(dict(lx=1, lxw=1), dict(lx=1, lxw=0)), dtype=dtype, dot=True)
    # 4-bit codes on and off
    _run(ctx, P["poisson16"], dict(lx=1, lxw=1, lx4=1),
         knobs=(dict(lx4=1), dict(lx4=0)), dtype=dtype, dot=True,
         reset=dict(lx4=1))
    ctx.set_option("lx_dma", 0)  # the register-staged kernel's own layout
    _run(ctx, P["banded"], dict(lx=1, lxw=0), dtype=dtype, dot=True,
         recipes=ALL + ("G0",))
    ctx.close()


def test_lx_narrowed_value_stream(P):
    """values exact in fp32 (S1 to S3): the narrowed stream and the fp64 one;
    S4's and S5's values are refused and take the fp64 stream"""
    ctx = _context(lx_min_nnz=0)
    for name in ("banded", "poisson16"):
        _run(ctx, P[name], dict(lx=1, lxw=1, lx_v32=1), setup=_bake, exact32=True,
             knobs=(dict(lx_v32=1), dict(lx_v32=0)), dot=True,
             reset=dict())
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_xw_kernel(P, dtype):
    ctx = _context(lx_min_nnz=1 << 62, lat_min_nnz=1 << 62, sj_min_nnz=1 << 62,
                   xw_min_nnz=0, xw_min_x_bytes=0)
    _run(ctx, P["banded"], dict(xw=1, lx=0, lat=0, sjds=0),
         knobs=(dict(nontemporal=1), dict(nontemporal=0)), dtype=dtype, dot=True)
    ctx.close()


def _sj_context(**more):
    return _context(sj_min_nnz=0, lx_min_nnz=1 << 62, lat_min_nnz=1 << 62, **more)


@pytest.mark.parametrize("sigma", [1, 0])
def test_sliced_jagged_form(P, sigma):
    ctx = _sj_context(sj_wpb=16, sj_unit=2, sj_sigma=sigma)
    bake = lambda blk: blk.bake()  # noqa: E731
    # staged entirely (16-bit codes), no long rows
    _run(ctx, P["fem"], dict(sjds=1, sj_wide=0, sj_far_permille=0, sj_wpb=16),
         algo=hip.ALGO_AUTO, setup=bake, dot=True)
    # long rows gathered (unsorted columns), rows the wave takes over
    _run(ctx, P["sj_ragged"], dict(sjds=1, sj_long_panels=0), algo=hip.ALGO_AUTO,
         setup=bake, dot=True)
    # long rows through the table kernel, the panel kernel, gathered
    _run(ctx, P["fem_tail"], dict(sjds=1, sj_long_panels=1, sj_long_table=1),
         algo=hip.ALGO_AUTO, setup=bake, dot=True,
         knobs=(dict(sj_long_table=1), dict(sj_long_table=0),
                dict(sj_long_panels=0)),
         reset=dict(sj_long_panels=1, sj_long_table=1))
    # a chunk budget of 8: most entries far, 32-bit codes
    ctx.set_option("sj_max_chunks", 8)
    _run(ctx, P["sj_ragged"], dict(sjds=1, sj_wide=1), algo=hip.ALGO_AUTO,
         setup=bake, dot=True)
    ctx.close()


def test_sliced_jagged_form_fp32(P):
    ctx = _sj_context()
    _run(ctx, P["fem_tail"], dict(sjds=1), algo=hip.ALGO_AUTO,
         setup=lambda blk: blk.bake(), dtype=np.float32)
    ctx.close()


def _lat_context(const):
    return _context(lat_min_nnz=0, lx_min_nnz=0, const_diagonals=const)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_diagonal_forms(P, dtype):
    bake = lambda blk: blk.bake()  # noqa: E731
    ctx = _lat_context(0)
    knobs = (dict(wdia_xcd_group=4), dict(wdia_xcd_group=0))
    # full form: 27-point stencil (absent slots at the faces), 32 offsets
    _run(ctx, P["stencil27"], dict(wdia=1, sdia=0, wdia_offsets=27, wdia_half=0,
                                   wdia_const=0),
         setup=bake, knobs=knobs, dtype=dtype, dot=True)
    _run(ctx, P["thirty_two"], dict(wdia=1, wdia_offsets=32), setup=bake,
         knobs=knobs, dtype=dtype, dot=True)
    # half form: the values symmetric bit for bit
    _run(ctx, P["stencil27_symvals"], dict(wdia=1, wdia_offsets=27, wdia_half=1),
         setup=bake, knobs=knobs, dtype=dtype, dot=True)
    ctx.close()
    ctx = _lat_context(1)
    _run(ctx, P["stencil27_const"], dict(wdia=1, wdia_offsets=27, wdia_const=1),
         setup=bake, knobs=knobs, dtype=dtype, dot=True)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_box27_half_marched_kernel(P, dtype):
    ctx = _lat_context(0)
    _run(ctx, P["box27"], dict(wdia=1, wdia_offsets=27, wdia_half=1, wdia_const=0,
                               wdia_hbox=1),
         setup=lambda blk: blk.bake(), dtype=dtype, dot=True,
         knobs=(dict(wdia_hbox_segs=0), dict(wdia_hbox_segs=2)))
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diagonal_form_of_a_general_matrix(P, dtype):
    bake = lambda blk: blk.bake()  # noqa: E731
    ctx = _lat_context(0)
    knobs = (dict(sdia_chain=1), dict(sdia_chain=0), dict(zwalk_segments=1))
    for n in (9, 16):
        # found symmetric: the lower half by offset
        _run(ctx, P[f"poisson{n}_symvals"], dict(lat=1, sdia=1, sdia_general=1),
             setup=bake, knobs=knobs, dtype=dtype, dot=True)
        # not symmetric: the full form
        _run(ctx, P[f"poisson{n}"], dict(lat=1, sdia=1, sdia_general=2),
             setup=bake, knobs=knobs, dtype=dtype, dot=True)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_diagonal_kernels(P, dtype):
    """one number per diagonal (a whole diagonal 0.0 and another -0.0 in S2);
    the tile kernel of constant 3-D lattices"""
    ctx = _lat_context(1)
    for n in (9, 16):
        _run(ctx, P[f"poisson{n}_const"], dict(sdia=1, sdia_const=1, sdia_offsets=3),
             setup=lambda blk: blk.bake(), dtype=dtype, dot=True,
             knobs=(dict(sdia_tile=1), dict(sdia_tile=2), dict(sdia_tile=4)),
             reset=dict(sdia_tile=1))
    ctx.close()


# ---------------------------------------------------------------------------
# Symmetric storage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_symmetric_storage_forms(P, dtype):
    ctx = _lat_context(0)
    # the transposed map (four lower offsets: no lattice form)
    _run(ctx, P["four_lower"], dict(slat=0, sym_det=1), dtype=dtype, dot=True)
    for n in (9, 16):
        p = P[f"poisson{n}_lower"]
        _run(ctx, p, dict(slat=1, sdia=0), dtype=dtype, dot=True,
             knobs=(dict(nontemporal=1), dict(nontemporal=0)))
        _run(ctx, p, dict(slat=1, sdia=1), setup=lambda blk: blk.bake(),
             dtype=dtype, dot=True, knobs=(dict(sdia_chain=1), dict(sdia_chain=0)))
    ctx.close()


def test_symmetric_storage_sliced_jagged(P):
    ctx = _sj_context()
    bake = lambda blk: blk.bake()  # noqa: E731
    _run(ctx, P["fem_lower"], dict(sym_sj=1, sjds=1, sj_long_rows=0), setup=bake,
         dot=True)
    p = P["fem_tail_lower"]
    blk = hip.CsrBlock(ctx, p.N, p.N, p.rp, p.ci, p.data("S1").va,
                       p.data("S1").diag, True)
    blk.bake()
    assert blk.get("sj_long_rows") > 10 and blk.get("sj_long_sorted") == 1
    blk.free()
    _run(ctx, p, dict(sym_sj=1, sjds=1, sj_long_sorted=1), setup=bake, dot=True)
    ctx.close()


# ---------------------------------------------------------------------------
# Mixed precision: fp32 values (S5: fp32 subnormals) under fp64 vectors
# ---------------------------------------------------------------------------
MIXED = ("S1", "S2", "S3", "S5m")


def test_mixed_precision_forms(P):
    bake = lambda blk: blk.bake()  # noqa: E731
    ctx = hip.Context(0)
    # the CSR-order kernels on the caller's fp32 array (nothing baked)
    for algo in (hip.ALGO_SCALAR, hip.ALGO_ROWBLOCK, hip.ALGO_ROWLIST):
        knobs = (dict(rowlist_exact=1),) if algo == hip.ALGO_ROWLIST else (dict(),)
        _run(ctx, P["ragged"], dict(algo=algo), algo=algo, recipes=MIXED,
             mixed="none", knobs=knobs)
        _run(ctx, P["remote"], dict(algo=algo), algo=algo, recipes=MIXED + GHOST,
             mixed="none", knobs=knobs, dot=True)
    ctx.close()
    ctx = _context(lx_min_nnz=0)
    _run(ctx, P["banded"], dict(lx=1, lxw=1), recipes=MIXED + ("G0",), mixed="none",
         knobs=(dict(lx=1, lxw=1), dict(lx=1, lxw=0)), dot=True)
    ctx.close()
    ctx = _lat_context(0)
    _run(ctx, P["poisson9"], dict(lat=1), recipes=MIXED, mixed="none")
    _run(ctx, P["stencil27"], dict(wdia=1), setup=bake, recipes=MIXED,
         mixed="wdia_mixed", dot=True)
    _run(ctx, P["poisson9"], dict(sdia=1, sdia_general=2), setup=bake,
         recipes=MIXED, mixed="sdia_mixed", dot=True)
    ctx.close()
    ctx = _lat_context(1)
    _run(ctx, P["poisson9_const"], dict(sdia=1, sdia_const=1), setup=bake,
         recipes=MIXED, mixed="sdia_mixed", dot=True)
    ctx.close()
    ctx = _sj_context()
    for name in ("fem", "fem_tail"):
        _run(ctx, P[name], dict(sjds=1), algo=hip.ALGO_AUTO, setup=bake,
             recipes=MIXED, mixed="sj_mixed", dot=True)
    ctx.close()


# ---------------------------------------------------------------------------
# mult_block: k interleaved vectors, another set of poisoned entries per column
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_mult_block_columns_do_not_leak(ctx, P, k):
    p = P["banded"]
    blk = None
    for recipe in ("S1", "S3"):
        base = p.data(recipe)
        cols = []
        for c in range(k):
            q = sv.Pattern(p.rp, p.ci, p.N, p.ncols, seed=100 + c)
            cols.append(q.data(recipe))
        X = np.stack([d.x for d in cols], axis=1)
        Y0 = np.stack([d.y0 for d in cols], axis=1)
        if recipe == "S1":  # the columns' poisoned entries differ
            assert len({tuple(d.poisoned) for d in cols}) == k
        blk = hip.CsrBlock(ctx, p.N, p.ncols, p.rp, p.ci, base.va)
        d_x = ctx.upload(X)
        for alpha, beta in base.ab:
            ref = np.stack([sv.ref_spmv(p.rp, p.ci, base.va, X[:, c].copy(), alpha,
                                        beta, Y0[:, c].copy(), np.float64)
                            for c in range(k)], axis=1)
            d_y = ctx.upload(np.full((p.N, k), np.nan) if beta == 0 else Y0)
            blk.multm(alpha, d_x.ptr, beta, d_y.ptr, k)
            ctx.synchronize()
            Y = d_y.numpy().reshape(p.N, k)
            d_y.free()
            assert blk.get("mv_form") == (1 if k in (2, 4, 8) else 2)
            for c in range(k):
                assert sv.same_bits(np.ascontiguousarray(Y[:, c]),
                                    np.ascontiguousarray(ref[:, c])), (recipe, c,
                                                                       alpha, beta)
        d_x.free()
        blk.free()


# ---------------------------------------------------------------------------
# transpmult: the stable-transpose CSR sum
# ---------------------------------------------------------------------------
def _transposed(p, va):
    rp = p.rp.astype(np.int64)
    rows = np.repeat(np.arange(p.N, dtype=np.int32), np.diff(rp))
    order = np.argsort(p.ci, kind="stable")
    tp = np.zeros(p.ncols + 1, np.int64)
    np.add.at(tp, p.ci.astype(np.int64) + 1, 1)
    return np.cumsum(tp), rows[order], va[order]


@pytest.mark.parametrize("form", [1, 2, 3])
def test_transpmult_forms(P, form):
    """t_form 1 (the transposed copy), 2 (in place), 3 (a block that is its own
    transpose); t_form 0 is a plan without a transpose: nothing to launch"""
    ctx = _context(lat_min_nnz=0) if form == 3 else hip.Context(0)
    p = P["poisson16_symvals"] if form == 3 else P["ragged"]
    for recipe in ("S1", "S3"):
        d = p.data(recipe)
        q = sv.Pattern(p.rp, p.ci, p.ncols, p.N, seed=7)  # x over the ROWS
        dq = q.data(recipe)
        x, y0 = dq.x, dq.y0
        blk = hip.CsrBlock(ctx, p.N, p.ncols, p.rp, p.ci, d.va)
        assert blk.get("t_form") == 0
        if form == 3:
            blk.bake()
        blk.transpose()
        if form == 2:
            blk.set("t_in_place", 1)
        assert blk.get("t_form") == form, recipe
        tp, tr, tv = _transposed(p, d.va)
        d_x = ctx.upload(x)
        for alpha, beta in d.ab:
            ref = sv.ref_spmv(tp, tr, tv, x, alpha, beta, y0, np.float64)
            d_y = ctx.upload(np.full(p.ncols, np.nan) if beta == 0 else y0)
            blk.multt(alpha, d_x.ptr, beta, d_y.ptr)
            ctx.synchronize()
            y = d_y.numpy()
            d_y.free()
            assert sv.same_bits(y, ref), (recipe, alpha, beta)
        d_x.free()
        blk.free()
    ctx.close()


# ---------------------------------------------------------------------------
# Order-tolerant kernels: the class (finite / not finite) and the rounding bound
# ---------------------------------------------------------------------------
def test_order_tolerant_kernels_keep_the_class(P):
    ctx = hip.Context(0)
    p = P["ragged"]
    d = p.data("S1")
    blk = hip.CsrBlock(ctx, p.N, p.ncols, p.rp, p.ci, d.va, None, False,
                       hip.ALGO_VECTOR)
    assert blk.algo == hip.ALGO_VECTOR
    dx = ctx.upload(d.x)
    lens = np.diff(p.rp)
    for alpha, beta in d.ab:
        y_ref = p.ref(d, alpha, beta)
        dy = ctx.upload(np.full(p.N, np.nan) if beta == 0 else d.y0)
        blk.mult(alpha, dx.ptr, beta, dy.ptr)
        y = dy.numpy()
        dy.free()
        fin = np.isfinite(y_ref)
        assert np.array_equal(np.isfinite(y), fin), (alpha, beta)
        with np.errstate(all="ignore"):
            bound = (16 + lens) * U * abs_bound(p.rp, p.ci, d.va, d.x, alpha, beta,
                                                d.y0)
            err = np.abs(y - y_ref)
        assert np.all(err[fin] <= bound[fin] + 1e-300), (alpha, beta)
    dx.free()
    blk.free()
    ctx.close()
    # the atomic symmetric kernels (plan_set "sym_det" 0), held to the bounds of
    # test_gpu_kernels.py: fp64 16 u (|alpha| |A| |x| + |beta| |y0|)_i per row on
    # the full matrix, fp32 the absolute 16 * 2**-24 * 12; `out` poisoned
    ctx = hip.Context(0)
    for dtype in (np.float64, np.float32):
        p = P["poisson9_lower"]
        d = p.data("S1", dtype)
        blk = hip.CsrBlock(ctx, p.N, p.N, p.rp, p.ci, d.va, d.diag, True,
                           hip.ALGO_AUTO, dtype)
        assert blk.get("sym_det") == 1
        blk.set("sym_det", 0)
        assert blk.get("sym_det") == 0
        dx = ctx.upload(d.x, dtype)
        rows = np.repeat(np.arange(p.N), np.diff(p.rp))
        with np.errstate(all="ignore"):
            ax = np.abs(d.diag.astype(np.float64) * d.x)
            prod = np.abs(d.va.astype(np.float64))
            np.add.at(ax, rows, prod * np.abs(d.x[p.ci].astype(np.float64)))
            np.add.at(ax, p.ci, prod * np.abs(d.x[rows].astype(np.float64)))
        for alpha, beta in d.ab:
            y_ref = p.ref(d, alpha, beta)
            dy = ctx.upload(np.full(p.N, np.nan, dtype) if beta == 0 else d.y0,
                            dtype)
            blk.mult(alpha, dx.ptr, beta, dy.ptr)
            y = dy.numpy()
            dy.free()
            fin = np.isfinite(y_ref)
            assert np.array_equal(np.isfinite(y), fin), (dtype, alpha, beta)
            err = np.abs(y[fin].astype(np.float64) - y_ref[fin])
            if dtype == np.float64:
                bound = 16 * U * (abs(alpha) * ax + abs(beta) * np.abs(d.y0))
                assert np.all(err <= bound[fin] + 1e-300), (alpha, beta)
            else:
                assert np.all(err <= 16 * 2.0 ** -24 * 12), (alpha, beta)
        dx.free()
        blk.free()
    ctx.close()
