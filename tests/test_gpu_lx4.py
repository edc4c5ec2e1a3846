"""GPU parity tests of the 4-bit codes of the LX form's LDS-DMA kernel
(spmv_lxw.hip, lx4_encode_kernel in spmv_csr_forms.hip): a row block whose
16-bit offsets are the row's lane plus one of at most 16 distances streams one
nibble per entry and carries the distances as a dictionary in its record.
Every product is compared BIT FOR BIT with the CPU oracle and with the same
plan running on its 16-bit offsets (plan key lx4 = 0); the fused dot's
partials likewise.  The asserts on lx4 / lx4_blocks keep a silent fall-back to
the offsets from hiding a broken encoder."""
import numpy as np
import pytest

import oracle
from gpu_helpers import stencil_csr as _stencil_csr
from spmv_amd import hip, poisson

pytestmark = pytest.mark.gpu

AB = ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0), (1.0, -0.25))


@pytest.fixture()
def lx_ctx():
    c = hip.Context(0)
    c.set_option("lx_min_nnz", 0)  # build the form for small test matrices too
    yield c
    c.close()


def _mult(ctx, blk, x_dev, alpha, beta, y0, nrows, dtype, part=None):
    """One product into a NaN-poisoned (beta == 0) output; y and, with `part`,
    the fused dot's partial sums."""
    dy = ctx.upload(np.full(nrows, np.nan, dtype) if beta == 0 else y0, dtype)
    if part is not None:
        blk.mult(alpha, x_dev.ptr, beta, dy.ptr, dot_partials=part.ptr)
    else:
        blk.mult(alpha, x_dev.ptr, beta, dy.ptr)
    y = dy.numpy()
    dy.free()
    return y, (part.numpy().copy() if part is not None else None)


def _check_all(ctx, name, rp, ci, va, nrows, ncols, dtype, rng, want_coded,
               nts=(0, 1)):
    """Codes on (both look-ups) and off against the oracle, every alpha / beta
    and non-temporal setting; the fused dot's partials where it exists (fp64,
    beta == 0).  want_coded: 'all', 'some' or 'none' of the staged blocks."""
    va = va.astype(dtype)
    x = rng.uniform(-1, 1, ncols).astype(dtype)
    y0 = rng.uniform(-1, 1, nrows).astype(dtype)
    blk = hip.CsrBlock(ctx, nrows, ncols, rp, ci, va, None, False,
                       hip.ALGO_ROWBLOCK, dtype)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1, name
    staged, coded = blk.get("lx_staged"), blk.get("lx4_blocks")
    print(f"{name}: lx_staged={staged} lx4_blocks={coded} "
          f"lx4={blk.get('lx4')} lx4_all={blk.get('lx4_all')}")
    if want_coded == "all":
        assert blk.get("lx4") == 1, name
        assert coded == staged and blk.get("lx4_all") == 1, (name, coded, staged)
    elif want_coded == "some":
        assert blk.get("lx4") == 1, name
        assert 0 < coded < staged and blk.get("lx4_all") == 0, (name, coded,
                                                                 staged)
    else:
        assert blk.get("lx4") == 0 and coded == 0, name
        with pytest.raises(Exception):
            blk.set("lx4", 1)  # there are no codes
    dx = ctx.upload(x, dtype)
    part = (ctx.empty(ctx.dot_partials_len, np.float64)
            if dtype == np.float64 else None)
    variants = [(0, 1)] if want_coded == "none" else [(0, 1), (1, 1), (1, 2)]
    for alpha, beta in AB:
        y_ref = oracle.csr_spmv(rp, ci, va, x, alpha, beta, y0)  # f32-aware
        for nt in nts:
            blk.set("nontemporal", nt)
            for dot in ((False, True) if part is not None and beta == 0
                        else (False,)):
                base = None
                for lx4, lut in variants:
                    blk.set("lx4", lx4)
                    blk.set("lx4_lut", lut)
                    y, p = _mult(ctx, blk, dx, alpha, beta, y0, nrows, dtype,
                                 part if dot else None)
                    tag = (name, alpha, beta, nt, dot, lx4, lut)
                    assert np.array_equal(y, y_ref), tag
                    if lx4 == 0:
                        base = (y, p)
                    else:
                        assert np.array_equal(y, base[0]), tag
                        if dot:
                            assert np.array_equal(p, base[1]), tag
    blk.set("lx4_lut", 1)
    for b in (dx, part):
        if b is not None:
            b.free()
    return blk


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lx4_coded_matrices_bit_exact(lx_ctx, dtype):
    """7-point Poisson and a tridiagonal matrix: every staged row block touches
    at most 7 diagonals, so every one must be coded."""
    ctx = lx_ctx
    rng = np.random.default_rng(4004)
    cases = []
    for n in (16, 20, 33, 48):
        rp, ci, va = poisson.poisson3d_csr(n)
        cases.append((f"poisson{n}", rp, ci.astype(np.int32), va, n ** 3))
    rp, ci, va = oracle.tridiag_csr(70001)  # odd column count: rounded windows
    cases.append(("tridiag", rp, ci, va, 70001))
    for name, rp, ci, va, N in cases:
        blk = _check_all(ctx, name, rp, ci, va, N, N, dtype, rng, "all")
        blk.free()


@pytest.mark.parametrize("n", [32, 33, 48])
def test_lx4_plane_walk_bit_exact(lx_ctx, n):
    """The stencil matrices and knob sets of test_lxw_plane_walk_bit_exact
    (random values, a third of the entries dropped, forced plane-walk tables,
    one workgroup per CU, the register-staged kernel in between): all coded,
    same bits with the codes on and off, fused dot's partials included."""
    ctx = lx_ctx
    rng = np.random.default_rng(500 + n)
    N = n ** 3
    offs = [-n * n, -n, -1, 0, 1, n, n * n]
    for drop in (0.0, 0.3):
        rp, ci, va = _stencil_csr(rng, N, offs, drop=drop)
        x = rng.uniform(-1, 1, N)
        y0 = rng.uniform(-1, 1, N)
        blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK)
        assert blk.get("lx") == 1 and blk.get("lxw") == 1 and blk.get("lat") == 0
        assert blk.get("lx4") == 1 and blk.get("lx4_all") == 1
        assert blk.get("lx4_blocks") == blk.get("lx_staged") > 0
        dx = ctx.upload(x)
        part = ctx.empty(ctx.dot_partials_len, np.float64)
        for alpha, beta in ((1.0, 0.0), (-0.5, 0.75)):
            y_ref = oracle.csr_spmv(rp, ci, va, x, alpha, beta, y0)
            for knobs in (dict(), dict(zwalk_segments=1), dict(zwalk_segments=2),
                          dict(zwalk_segments=3), dict(zwalk=0),
                          dict(zwalk=1, lxw_blocks_per_cu=1),
                          dict(lxw_blocks_per_cu=0), dict(lxw=0), dict(lxw=1)):
                for k, v in knobs.items():
                    blk.set(k, v)
                dot = beta == 0
                got = {}
                for lx4, lut in ((1, 1), (0, 1), (1, 2)):
                    blk.set("lx4", lx4)
                    blk.set("lx4_lut", lut)
                    got[lx4, lut] = _mult(ctx, blk, dx, alpha, beta, y0, N,
                                          np.float64, part if dot else None)
                    tag = (n, drop, alpha, knobs, lx4, lut)
                    assert np.array_equal(got[lx4, lut][0], y_ref), tag
                for key in ((1, 1), (1, 2)):
                    if dot:  # the same partial sums, slot for slot
                        assert np.array_equal(got[key][1], got[0, 1][1]), (
                            n, drop, alpha, knobs, key)
                if dot:
                    want = float(np.dot(x, y_ref))
                    s = float(np.sum(got[1, 1][1]))
                    assert abs(s - want) <= 1e-12 * (np.abs(x) @ np.abs(y_ref))
        blk.set("lx4_lut", 1)
        for b in (dx, part):
            b.free()
        blk.free()


def _diagonals_csr(rng, nrows, ncols, offsets_of_row):
    rows, cols = [], []
    for i in range(nrows):
        c = sorted(i + d for d in offsets_of_row(i))
        rows += [i] * len(c)
        cols += c
    rp = np.zeros(nrows + 1, np.int64)
    np.add.at(rp, np.asarray(rows) + 1, 1)
    return (np.cumsum(rp).astype(np.int32), np.asarray(cols, np.int32),
            rng.uniform(-1, 1, len(cols)))


def _banded(rng, nrb, extra_in):
    """Diagonals 0, 3, ..., 45 (16 of them), the even rows on the first eight
    and the odd rows on the last eight: one window per row block (gaps of at
    most 3 columns), so a block's distinct distances are its distinct
    diagonals -- 16.  The row blocks for which extra_in(block) holds have
    diagonal 48 too on every fourth row: 17."""
    nrows = 256 * nrb - 37  # a ragged last block
    low = [3 * k for k in range(8)]
    high = [24 + 3 * k for k in range(8)]

    def offs(i):
        o = list(low if i % 2 == 0 else high)
        if extra_in(i // 256) and i % 4 == 0:
            o.append(48)
        return o

    ncols = (nrows + 64) & ~3
    return _diagonals_csr(rng, nrows, ncols, offs) + (nrows, ncols)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lx4_mixed_and_uncoded_blocks(lx_ctx, dtype):
    """Row blocks with exactly 16 distinct distances beside blocks with 17 (the
    choice is per block: the latter read their 16-bit offsets in the same
    launch), and a matrix whose blocks all have 17: no codes at all."""
    ctx = lx_ctx
    rng = np.random.default_rng(1617)
    nrb = 8
    rp, ci, va, nrows, ncols = _banded(rng, nrb, lambda b: b % 2 == 1)
    blk = _check_all(ctx, "banded16/17", rp, ci, va, nrows, ncols, dtype, rng,
                     "some")
    assert blk.get("lx_staged") == nrb and blk.get("lx4_blocks") == nrb // 2
    blk.free()
    rp, ci, va, nrows, ncols = _banded(rng, nrb, lambda b: True)
    blk = _check_all(ctx, "banded17", rp, ci, va, nrows, ncols, dtype, rng,
                     "none")
    assert blk.get("lx_staged") == nrb
    blk.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lx4_27_point_stencil_falls_back(lx_ctx, dtype):
    """The 27-point stencil with the lattice and wide-diagonal forms off (no
    lattice analysis below 2^20 entries, nothing baked): an interior row block
    touches 27 diagonals, more than a dictionary holds.  No codes, same bits."""
    ctx = lx_ctx
    rng = np.random.default_rng(27)
    n = 20
    N = n ** 3
    rp, ci, va = poisson.stencil27_csr(n)
    ci = ci.astype(np.int32)
    va = np.asarray(va).astype(dtype)
    x = rng.uniform(-1, 1, N).astype(dtype)
    y0 = rng.uniform(-1, 1, N).astype(dtype)
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK,
                       dtype)
    assert blk.get("lat") == 0 and blk.get("wdia") == 0
    assert blk.get("lx4") == 0 and blk.get("lx4_blocks") == 0
    with pytest.raises(Exception):
        blk.set("lx4", 1)
    dx = ctx.upload(x, dtype)
    for alpha, beta in AB:
        y_ref = oracle.csr_spmv(rp, ci, va, x, alpha, beta, y0)
        for nt in (0, 1):
            blk.set("nontemporal", nt)
            y, _ = _mult(ctx, blk, dx, alpha, beta, y0, N, dtype)
            assert np.array_equal(y, y_ref), (alpha, beta, nt)
    dx.free()
    blk.free()


def test_lx4_toggles_and_context_option(lx_ctx):
    """lx4 and lxw toggled on one coded plan (the register-staged kernel reads
    the 16-bit offsets of the same plan); a plan made with the context option
    lx_codes = 0 has no codes and refuses lx4 = 1."""
    ctx = lx_ctx
    rng = np.random.default_rng(99)
    n = 33
    N = n ** 3
    rp, ci, va = poisson.poisson3d_csr(n)
    ci = ci.astype(np.int32)
    x = rng.uniform(-1, 1, N)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dx = ctx.upload(x)
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK)
    assert blk.get("lx4") == 1 and blk.get("lx4_all") == 1
    kib_coded = blk.get("plan_kib")
    grid = blk.get("lxw_grid")
    assert grid > 0
    parts = []
    for key, v in (("lx4", 1), ("lx4", 0), ("lx4", 1), ("lxw", 0), ("lxw", 1),
                   ("lx4", 0), ("lxw", 0), ("lxw", 1), ("lx4", 1)):
        blk.set(key, v)
        assert blk.get(key) == v
        assert blk.get("lxw_grid") == grid  # the geometry does not move
        y, p = _mult(ctx, blk, dx, 1.0, 0.0, None, N, np.float64, part)
        assert np.array_equal(y, y_ref), (key, v)
        if blk.get("lxw") == 1:
            parts.append(p)
    for p in parts[1:]:
        assert np.array_equal(p, parts[0])
    blk.free()
    ctx.set_option("lx_codes", 0)
    try:
        blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK)
    finally:
        ctx.set_option("lx_codes", 1)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1
    assert blk.get("lx4") == 0 and blk.get("lx4_blocks") == 0
    assert blk.get("lx4_all") == 0
    assert blk.get("lxw_grid") == grid
    # the codes are 0.5 B per entry of plan memory (+ padding)
    assert 0 < kib_coded - blk.get("plan_kib") <= (len(ci) // 2 + 64) // 1024 + 1
    with pytest.raises(Exception):
        blk.set("lx4", 1)
    y, p = _mult(ctx, blk, dx, 1.0, 0.0, None, N, np.float64, part)
    assert np.array_equal(y, y_ref)
    assert np.array_equal(p, parts[0])
    blk.free()
    for b in (dx, part):
        b.free()


def test_lx4_at_512_cubed():
    """The benchmark's CSR-order plan (create_poisson3d with the lattice
    analysis off): every staged block is coded, y with the codes equals y with
    the 16-bit offsets bit for bit, and the launch grid does not depend on the
    toggle."""
    from spmv_amd import _lib, host
    n = 512
    N = n ** 3
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    ctx = exec_.context
    _lib.call("spmv_hip_ctx_set_option", ctx, b"lat_min_nnz", 1 << 62)
    try:
        A = host.Matrix.create_poisson3d(comm, exec_, n, False,
                                         host.P2P_NONBLOCKING)
    finally:
        _lib.call("spmv_hip_ctx_set_option", ctx, b"lat_min_nnz", 1 << 20)
    assert A.plan_get("lat") == 0 and A.plan_get("lx") == 1
    assert A.plan_get("lxw") == 1 and A.plan_get("lx4") == 1
    assert A.plan_get("lx4_all") == 1
    assert A.plan_get("lx4_blocks") == A.plan_get("lx_staged") > 0
    print("512^3 CSR-order plan: plan_us", A.plan_get("plan_us"), "plan_kib",
          A.plan_get("plan_kib"))
    grid = A.plan_get("lxw_grid")
    assert grid > 0
    d_x, d_y = exec_.alloc(N), exec_.alloc(N)
    _lib.call("spmv_hip_fill_gaussian_f64", ctx, N, 0, N, d_x, None)
    ys = []
    for lx4, lut in ((1, 1), (0, 1), (1, 2)):
        A.plan_set("lx4", lx4)
        A.plan_set("lx4_lut", lut)
        assert A.plan_get("lx4") == lx4 and A.plan_get("lxw_grid") == grid
        _lib.call("spmv_hip_fill_const_f64", ctx, N, float("nan"), d_y, None)
        A.mult(d_x, d_y)
        ys.append(exec_.copy_to_host(d_y, N))
    assert np.isfinite(ys[1]).all() and np.abs(ys[1]).max() > 0
    assert np.array_equal(ys[0], ys[1])
    assert np.array_equal(ys[2], ys[1])
    A.close()
    exec_.free(d_x), exec_.free(d_y)
    comm.close()
    exec_.close()
