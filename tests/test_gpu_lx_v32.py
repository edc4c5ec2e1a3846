"""GPU parity tests of the narrowed value stream of the LX form's LDS-DMA
kernel (spmv_lxw.hip, lx32_check_kernel / lx32_convert_kernel in
spmv_csr_forms.hip): when plan_bake_values finds every value of an fp64 LX plan
exactly representable as a normal binary32 number (or +-0), the plan keeps an
fp32 copy and the kernel streams 4 instead of 8 bytes per entry, widening each
value in the row sum.  (double)(float)v has the bits of v, so every product and
every add is the one the fp64 stream gives: y is compared BIT FOR BIT (as
uint64) with the CPU oracle and with the same plan after plan_set("lx_v32", 0),
the fused dot's partials likewise.  The asserts on lx_v32 keep a silent fall
back to the fp64 stream from hiding a broken check or copy."""
import numpy as np
import pytest

import oracle
from gpu_helpers import stencil_csr
from spmv_amd import _lib, hip, host, poisson

pytestmark = pytest.mark.gpu

AB = ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0), (1.0, -0.25))
ENOTSUP = -3  # no form holds the values by offset: what an LX plan's bake returns


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64
                                        else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bake(blk):
    """plan_bake_values on the block's own device values.  An LX plan has no
    form that holds the values by offset (ENOTSUP); the narrowed copy is made
    or refused beside that and shows in plan_get("lx_v32")."""
    name = ("spmv_hip_csr_plan_bake_values_f64" if blk.dtype == np.float64
            else "spmv_hip_csr_plan_bake_values_f32")
    rc = getattr(_lib.hip, name)(blk.ctx.h, blk.plan, blk.values.ptr, None, None)
    assert rc in (0, ENOTSUP), rc


def _poisson33():
    rp, ci, va = poisson.poisson3d_csr(33)  # 35 937 rows: a partial last block
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, np.float64), 33 ** 3)


def _banded_quarters():
    """20 011 rows on nine diagonals within +-300 columns, a quarter of the
    entries dropped: one or two staged windows per row block.  Values k / 4,
    k in [-32, 32] without 0, and a few -0.0."""
    rng = np.random.default_rng(3232)
    N = 20011
    rp, ci, _ = stencil_csr(rng, N, (-290, -151, -37, -2, 0, 1, 40, 160, 300),
                            drop=0.25)
    k = rng.integers(1, 33, len(ci)) * rng.choice((-1, 1), len(ci))
    va = k / 4.0
    va[rng.choice(len(ci), 17, replace=False)] = -0.0
    return rp, ci, va, N


MATRICES = {"poisson33": _poisson33, "banded": _banded_quarters}


@pytest.fixture(scope="module")
def matrices():
    """name -> (rowptr, colind, values, N, x, y0, {(alpha, beta): y_ref}):
    the oracle's products, computed once and left unchanged."""
    out = {}
    for name, make in MATRICES.items():
        rp, ci, va, N = make()
        rng = np.random.default_rng(len(ci))
        x, y0 = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
        refs = {ab: oracle.csr_spmv(rp, ci, va, x, ab[0], ab[1], y0) for ab in AB}
        for a in (rp, ci, va, x, y0, *refs.values()):
            a.setflags(write=False)
        out[name] = (rp, ci, va, N, x, y0, refs)
    return out


@pytest.fixture(params=[1, 0], ids=["codes", "offsets"])
def lx_ctx(request):
    c = hip.Context(0)
    c.set_option("lx_min_nnz", 0)  # build the form for small test matrices too
    c.set_option("lx_codes", request.param)
    yield c
    c.close()


def _block(ctx, rp, ci, va, N, dtype=np.float64):
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK,
                       dtype)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1 and blk.get("lat") == 0
    assert blk.get("lx_staged") > 0
    return blk


def _mult(ctx, blk, dx, alpha, beta, y0, N, part=None):
    """One product into a NaN-poisoned (beta == 0) output."""
    dy = ctx.upload(np.full(N, np.nan) if beta == 0 else y0)
    blk.mult(alpha, dx.ptr, beta, dy.ptr,
             dot_partials=None if part is None else part.ptr)
    y = dy.numpy()
    dy.free()
    return y, (None if part is None else part.numpy().copy())


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_lx_v32_bit_exact_and_same_geometry(lx_ctx, matrices, name):
    """Cases 1 and 2: y against the oracle and against narrowing off, every
    alpha / beta, both non-temporal settings, with and without the fused dot;
    the launch grid and the fused dot's partial array do not move."""
    ctx = lx_ctx
    rp, ci, va, N, x, y0, refs = matrices[name]
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx_v32") == 0  # nothing baked yet
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)  # there is no copy
    grid = blk.get("lxw_grid")
    _bake(blk)
    assert blk.get("lx_v32") == 1, name
    assert blk.get("lxw_grid") == grid > 0
    dx = ctx.upload(x)
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    for (alpha, beta), y_ref in refs.items():
        for nt in (0, 1):
            blk.set("nontemporal", nt)
            for dot in (False, True):
                got = {}
                for v32 in (1, 0):
                    blk.set("lx_v32", v32)
                    assert blk.get("lx_v32") == v32
                    assert blk.get("lxw_grid") == grid
                    part.write(np.full(part.count, np.nan))
                    got[v32] = _mult(ctx, blk, dx, alpha, beta, y0, N,
                                     part if dot else None)
                    tag = (name, alpha, beta, nt, dot, v32)
                    assert _same_bits(got[v32][0], y_ref), tag
                assert _same_bits(got[1][0], got[0][0])
                if dot:
                    assert np.array_equal(got[1][1], got[0][1]), tag
                    assert np.isfinite(got[1][1]).all(), tag
    for b in (dx, part):
        b.free()
    blk.free()


def _check_y(ctx, blk, rp, ci, va, N, x, dx, what):
    y, _ = _mult(ctx, blk, dx, 1.0, 0.0, None, N)
    assert _same_bits(y, oracle.csr_spmv(rp, ci, va, x)), what


@pytest.mark.parametrize("bad", [0.1, 2.0 ** -140, 1e39],
                         ids=["inexact", "fp32_subnormal", "fp32_overflow"])
def test_lx_v32_refusals(lx_ctx, matrices, bad):
    """Case 3: one entry of the last row block that binary32 cannot hold as a
    normal number keeps the whole plan on the fp64 stream."""
    ctx = lx_ctx
    rp, ci, va, N, x = matrices["poisson33"][:5]
    va = va.copy()
    va[len(va) - 5] = bad
    blk = _block(ctx, rp, ci, va, N)
    _bake(blk)
    assert blk.get("lx_v32") == 0, bad
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)
    dx = ctx.upload(x)
    _check_y(ctx, blk, rp, ci, va, N, x, dx, bad)
    dx.free()
    blk.free()


def test_lx_v32_rebake_and_context_option(lx_ctx, matrices):
    """Case 4: exact -> inexact -> exact values in the same device array, baked
    again each time; the context option lx_narrow_values = 0."""
    ctx = lx_ctx
    rp, ci, va, N, x = matrices["banded"][:5]
    dx = ctx.upload(x)
    blk = _block(ctx, rp, ci, va, N)
    inexact = va.copy()
    inexact[len(va) // 2] = 1.0 / 3.0
    other = va * 2.0  # exact again, another matrix
    for vals, want in ((va, 1), (inexact, 0), (other, 1)):
        blk.values.write(vals)
        _bake(blk)
        assert blk.get("lx_v32") == want
        _check_y(ctx, blk, rp, ci, vals, N, x, dx, want)
    kib_narrow = blk.get("plan_kib")
    blk.values.write(inexact)  # in place, then values_changed: the copy goes
    blk.values_changed()
    assert blk.get("lx_v32") == 0
    _check_y(ctx, blk, rp, ci, inexact, N, x, dx, "values_changed")
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)
    blk.free()
    ctx.set_option("lx_narrow_values", 0)
    try:
        blk = _block(ctx, rp, ci, va, N)
        _bake(blk)
    finally:
        ctx.set_option("lx_narrow_values", 1)
    assert blk.get("lx_v32") == 0
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)
    # the copy is 4 B per entry of plan memory (+ padding)
    d = kib_narrow - blk.get("plan_kib")
    assert 4 * len(ci) // 1024 - 1 <= d <= (4 * len(ci) + 64) // 1024 + 1, d
    _check_y(ctx, blk, rp, ci, va, N, x, dx, "lx_narrow_values = 0")
    dx.free()
    blk.free()


def test_lx_v32_cg_same_history_and_x():
    """Case 5: host.cg_ex at 33^3 with the CSR-order options, 40 iterations at
    rtol 0 and once with a tolerance stop (default defer_x): history, k and x
    are equal between lx_narrow_values 1 and 0."""
    rp, ci, va, N = _poisson33()
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    ctx = exec_.context
    b = oracle.csr_spmv(rp, ci, va, np.ones(N))
    d_b, d_x = exec_.alloc(N), exec_.alloc(N)
    exec_.copy_from_host(d_b, b)
    runs = {}
    for narrow in (1, 0):
        opts = ((b"lat_min_nnz", 1 << 62, 1 << 20), (b"lx_min_nnz", 0, 1 << 20),
                (b"lx_narrow_values", narrow, 1))
        for k_, v_, _ in opts:
            _lib.call("spmv_hip_ctx_set_option", ctx, k_, v_)
        try:
            A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [],
                                          False, host.P2P_NONBLOCKING)
        finally:
            for k_, _, d_ in opts:
                _lib.call("spmv_hip_ctx_set_option", ctx, k_, d_)
        assert A.plan_get("lx") == 1 and A.plan_get("lxw") == 1
        assert A.plan_get("lx_v32") == narrow
        ws = host.CgWorkspace(exec_)
        out = []
        for kmax, rtol in ((40, 0.0), (300, 1e-4)):
            exec_.copy_from_host(d_x, np.full(N, 777.0))
            k, hist, _, _ = host.cg_ex(comm, exec_, A, d_b, d_x, kmax, rtol, ws,
                                       history=True)
            out.append((k, hist.copy(), exec_.copy_to_host(d_x, N)))
        runs[narrow] = out
        ws.close()
        A.close()
    for (k1, h1, x1), (k0, h0, x0) in zip(runs[1], runs[0]):
        assert k1 == k0
        assert np.array_equal(h1, h0) and np.array_equal(x1, x0)
        assert np.isfinite(x1).all() and not np.any(x1 == 777.0)
    assert runs[1][0][0] == 40 and 0 < runs[1][1][0] < 300
    exec_.free(d_b), exec_.free(d_x)
    comm.close()
    exec_.close()


def test_lx_v32_not_elsewhere(matrices):
    """Case 6: a float32 block and a csr_in_place (XW) plan keep their
    streams."""
    rp, ci, va, N, x = matrices["poisson33"][:5]
    ctx = hip.Context(0)
    ctx.set_option("lx_min_nnz", 0)
    blk = _block(ctx, rp, ci, va.astype(np.float32), N, np.float32)
    _bake(blk)
    assert blk.get("lx_v32") == 0
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)
    x32 = x.astype(np.float32)
    dx = ctx.upload(x32)
    dy = ctx.upload(np.full(N, np.nan, np.float32))
    blk.mult(1.0, dx.ptr, 0.0, dy.ptr)
    assert _same_bits(dy.numpy(),
                      oracle.csr_spmv(rp, ci, va.astype(np.float32), x32))
    for b in (dx, dy):
        b.free()
    blk.free()
    ctx.set_option("csr_in_place", 1)
    ctx.set_option("xw_min_nnz", 0)
    ctx.set_option("xw_min_x_bytes", 0)
    ctx.set_option("xw_probe", 0)
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK)
    assert blk.get("lx") == 0 and blk.get("xw") == 1
    _bake(blk)
    assert blk.get("lx_v32") == 0
    with pytest.raises(Exception):
        blk.set("lx_v32", 1)
    dx = ctx.upload(x)
    _check_y(ctx, blk, rp, ci, va, N, x, dx, "xw")
    dx.free()
    blk.free()
    ctx.close()
