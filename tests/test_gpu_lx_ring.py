"""GPU parity tests of the ring variant of the LX form's LDS-DMA kernel
(csr_lxw_ring_kernel in spmv_lxw.hip; plan key / context option "lx_ring"):
three LDS slots, two row blocks in flight per workgroup, ONE counted wait per
step.  A miscounted wait shows as wrong bits, not as a fault, so every
comparison is equality of bits (uint64 view): y against the CPU oracle, y AND
the whole array of the fused dot's partials against the same plan after
plan_set("lx_ring", 0).  Outputs are NaN-poisoned, partials NaN-filled before
each launch.  The matrices are large enough for a workgroup to walk 2-3 row
blocks (prologue, drain, fewer than three) and 5-6 (the ring wraps, uneven
tails); the asserts on lx_ring keep a silent fall-back from hiding the kernel."""
import math

import numpy as np
import pytest

import oracle
from gpu_helpers import stencil_csr
from spmv_amd import _lib, hip, host, poisson

pytestmark = pytest.mark.gpu

AB = ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0), (1.0, -0.25))
ENOTSUP = -3
DIAGS = (-290, -151, -37, -2, 0, 1, 40, 160, 300)  # those of _banded_quarters
NO_LATTICE = 1 << 62


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bake(blk):
    rc = _lib.hip.spmv_hip_csr_plan_bake_values_f64(blk.ctx.h, blk.plan,
                                                    blk.values.ptr, None, None)
    assert rc in (0, ENOTSUP), rc


def _poisson(n):
    rp, ci, va = poisson.poisson3d_csr(n)
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, np.float64), n ** 3)


def _quarters(rng, ci):
    """Values k / 4, k in [-32, 32] without 0, and a few -0.0."""
    k = rng.integers(1, 33, len(ci)) * rng.choice((-1, 1), len(ci))
    va = k / 4.0
    va[rng.choice(len(ci), 17, replace=False)] = -0.0
    return va


def _banded(N, seed):
    """N rows on the nine diagonals of DIAGS, a quarter of the entries dropped;
    N is no multiple of 256: the last row block is partial.  (N a multiple of
    4: every column lies in a whole 16-byte chunk of x, so the blocks at the
    end of the matrix are staged like the others.)"""
    rng = np.random.default_rng(seed)
    rp, ci, _ = stencil_csr(rng, N, DIAGS, drop=0.25)
    return rp, ci, _quarters(rng, ci), N


def _distances_per_block(rp, ci, N):
    """Most distinct (column - row) in a row block.  The diagonals lie closer
    than the window gap, so a block stages ONE window and the distinct
    distances of its offsets are its distinct diagonals."""
    rows = np.repeat(np.arange(N), np.diff(rp))
    key = (rows // 256).astype(np.int64) * 4096 + (ci - rows + 2048)
    u = np.unique(key)
    return np.bincount(u // 4096)


def _banded_wide_block(N, seed, block):
    """The banded matrix with ten more diagonals (400, 402, ..., 418: one per
    row, by row % 10) in the rows of one row block: 19 distinct distances
    there, more than a dictionary holds."""
    rp, ci, va, N = _banded(N, seed)
    rows = np.repeat(np.arange(N), np.diff(rp))
    extra = np.arange(256 * block, 256 * block + 256)
    rows = np.concatenate((rows, extra))
    cols = np.concatenate((ci, extra + 400 + 2 * (extra % 10)))
    vals = np.concatenate((va, np.full(len(extra), 0.75)))
    order = np.lexsort((cols, rows))
    rp2 = np.zeros(N + 1, np.int64)
    np.add.at(rp2, rows + 1, 1)
    return (np.cumsum(rp2).astype(np.int32), cols[order].astype(np.int32),
            vals[order], N)


def _with_refs(rp, ci, va, N):
    rng = np.random.default_rng(len(ci))
    x, y0 = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    refs = {ab: oracle.csr_spmv(rp, ci, va, x, ab[0], ab[1], y0) for ab in AB}
    for a in (rp, ci, va, x, y0, *refs.values()):
        a.setflags(write=False)
    return rp, ci, va, N, x, y0, refs


@pytest.fixture(scope="module")
def big():
    """name -> (rowptr, colind, values, N, x, y0, {(alpha, beta): y_ref}): the
    oracle's products, computed once and left unchanged."""
    return {"poisson72": _with_refs(*_poisson(72)),
            "banded400k": _with_refs(*_banded(400012, 7201))}


def _ctx(codes=1, ring=1):
    c = hip.Context(0)
    c.set_option("lx_min_nnz", 0)
    c.set_option("lat_min_nnz", NO_LATTICE)  # the CSR-order plan, any size
    c.set_option("lx_codes", codes)
    c.set_option("lx_ring", ring)
    return c


def _block(ctx, rp, ci, va, N):
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK,
                       np.float64)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1 and blk.get("lat") == 0
    _bake(blk)
    return blk


def _force_ring(blk):
    """By default a launch takes the ring kernel only when a workgroup walks
    many row blocks (it pays from some tens of steps on); these matrices are
    small on purpose, so the kernel is asked for by name."""
    blk.set("lx_ring", 1)
    assert blk.get("lx_ring") == 1


def _mult(ctx, blk, dx, alpha, beta, y0, N, part):
    """One product into a NaN-poisoned (beta == 0) output, the partials
    NaN-filled before the launch."""
    dy = ctx.upload(np.full(N, np.nan) if beta == 0 else y0)
    if part is not None:
        part.write(np.full(part.count, np.nan))
    blk.mult(alpha, dx.ptr, beta, dy.ptr,
             dot_partials=None if part is None else part.ptr)
    y = dy.numpy()
    dy.free()
    return y, (None if part is None else part.numpy().copy())


def _ring_against_plain(ctx, blk, m, tag):
    """Every alpha / beta, both non-temporal settings, with and without the
    fused dot: the ring kernel against the oracle and against lx_ring = 0."""
    rp, ci, va, N, x, y0, refs = m
    grid = blk.get("lxw_grid")
    dx = ctx.upload(x)
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    for (alpha, beta), y_ref in refs.items():
        for nt in (0, 1):
            blk.set("nontemporal", nt)
            for dot in (False, True):
                got = {}
                for ring in (1, 0):
                    blk.set("lx_ring", ring)
                    assert blk.get("lx_ring") == ring
                    assert blk.get("lxw_grid") == grid
                    got[ring] = _mult(ctx, blk, dx, alpha, beta, y0, N,
                                      part if dot else None)
                    what = tag + (alpha, beta, nt, dot, ring)
                    assert _same_bits(got[ring][0], y_ref), what
                assert _same_bits(got[1][0], got[0][0]), what
                if dot:
                    assert _same_bits(got[1][1], got[0][1]), what
                    assert np.isfinite(got[1][1]).all(), what
    blk.set("lx_ring", 1)
    for b in (dx, part):
        b.free()


@pytest.mark.parametrize("name", ["poisson72", "banded400k"])
def test_lx_ring_bit_exact_both_grids(big, name):
    """Cases 1 and 2.  Default workgroups per CU: 2-3 row blocks per workgroup
    (prologue, drain, fewer than three); one per CU: 5-6 (the ring wraps, both
    parities, uneven tails).  The plane-walk table on and off where the matrix
    has one."""
    m = big[name]
    rp, ci, va, N = m[:4]
    if name == "banded400k":  # (else the plan is ineligible: case 3)
        assert _distances_per_block(rp, ci, N).max() <= 16
        assert N % 256 != 0
    nrb = (N + 255) // 256
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx_v32") == 1 and blk.get("lx4") == 1
    assert blk.get("lx_staged") == nrb == blk.get("lx4_blocks")
    assert blk.get("lx_ring_blocks") == nrb
    assert blk.get("lx_ring") == 0  # gated: a workgroup walks 2-3 row blocks
    _force_ring(blk)
    steps = []
    for per_cu in (0, 1):
        blk.set("lxw_blocks_per_cu", per_cu)
        grid = blk.get("lxw_grid")
        steps.append(math.ceil(nrb / grid))
        for zwalk in ((1, 0) if blk.get("zwalk") == 1 else (0,)):
            blk.set("zwalk", zwalk)
            assert blk.get("lx_ring") == 1, (name, per_cu, zwalk)
            _ring_against_plain(ctx, blk, m, (name, per_cu, zwalk))
        if blk.get("zwalk_grid") > 0:
            blk.set("zwalk", 1)
    print(f"{name}: row blocks per workgroup {steps}")
    blk.free()
    ctx.close()
    if max(steps) < 5:
        pytest.skip(f"{nrb} row blocks give a workgroup at most {max(steps)} "
                    "steps on this device: the ring never wraps")


def _ineligible(make_ctx, rp, ci, va, N):
    """lx_ring is 0 and cannot be set; y and the partials equal the oracle and
    what a plan made under the context option lx_ring = 0 gives."""
    rng = np.random.default_rng(N)
    x, y0 = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    got = {}
    for ring in (1, 0):
        ctx = make_ctx(ring)
        blk = _block(ctx, rp, ci, va, N)
        assert blk.get("lx_ring") == 0
        with pytest.raises(Exception):
            blk.set("lx_ring", 1)
        assert blk.get("lx_ring") == 0
        dx = ctx.upload(x)
        part = ctx.empty(ctx.dot_partials_len, np.float64)
        out = []
        for alpha, beta in AB:
            y, p = _mult(ctx, blk, dx, alpha, beta, y0, N, part)
            assert _same_bits(y, oracle.csr_spmv(rp, ci, va, x, alpha, beta, y0))
            out.append((y, p))
        got[ring] = out
        for b in (dx, part):
            b.free()
        blk.free()
        ctx.close()
    for (y1, p1), (y0_, p0) in zip(got[1], got[0]):
        assert _same_bits(y1, y0_) and _same_bits(p1, p0)


def test_lx_ring_ineligible_wide_block():
    """Case 3a: one row block with more than 16 distinct distances."""
    rp, ci, va, N = _banded_wide_block(20012, 7203, 5)
    d = _distances_per_block(rp, ci, N)
    assert d[5] > 16 and np.delete(d, 5).max() <= 16
    _ineligible(lambda ring: _ctx(ring=ring), rp, ci, va, N)


def test_lx_ring_ineligible_inexact_value():
    """Case 3b: one value binary32 does not hold: no narrowed stream."""
    rp, ci, va, N = _poisson(33)
    va = va.copy()
    va[len(va) - 5] = 0.1
    _ineligible(lambda ring: _ctx(ring=ring), rp, ci, va, N)


def test_lx_ring_ineligible_without_codes():
    """Case 3c: context option lx_codes = 0."""
    rp, ci, va, N = _poisson(33)
    _ineligible(lambda ring: _ctx(codes=0, ring=ring), rp, ci, va, N)


def test_lx_ring_eligible_small_matrix_single_step():
    """36^3 (a multiple of 4 rows, a partial last block): 183 row blocks, one
    per workgroup -- the ring never turns, the prologue and the drain are all
    there is."""
    m = _with_refs(*_poisson(36))
    ctx = _ctx()
    blk = _block(ctx, *m[:4])
    _force_ring(blk)
    _ring_against_plain(ctx, blk, m, ("poisson36",))
    blk.free()
    ctx.close()


def test_lx_ring_cg_same_history_and_x():
    """Case 4: host.cg_ex on 72^3 in the CSR-order plan, 12 iterations with the
    history; the context option lx_ring on (2: no gate on the steps per
    workgroup, which are 3 here), then 0: history and x keep their bits."""
    rp, ci, va, N = _poisson(72)
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    ctx = exec_.context
    b = oracle.csr_spmv(rp, ci, va, np.ones(N))
    d_b, d_x = exec_.alloc(N), exec_.alloc(N)
    exec_.copy_from_host(d_b, b)
    runs = {}
    for ring in (1, 0):
        opts = ((b"lat_min_nnz", NO_LATTICE, 1 << 20), (b"lx_min_nnz", 0, 1 << 20),
                (b"lx_ring", 2 * ring, 1))
        for k_, v_, _ in opts:
            _lib.call("spmv_hip_ctx_set_option", ctx, k_, v_)
        try:
            A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [],
                                          False, host.P2P_NONBLOCKING)
        finally:
            for k_, _, d_ in opts:
                _lib.call("spmv_hip_ctx_set_option", ctx, k_, d_)
        assert A.plan_get("lx") == 1 and A.plan_get("lxw") == 1
        assert A.plan_get("lx_v32") == 1
        assert A.plan_get("lx_ring") == ring
        ws = host.CgWorkspace(exec_)
        exec_.copy_from_host(d_x, np.full(N, 777.0))
        k, hist, _, _ = host.cg_ex(comm, exec_, A, d_b, d_x, 12, 0.0, ws,
                                   history=True)
        runs[ring] = (k, hist.copy(), exec_.copy_to_host(d_x, N))
        ws.close()
        A.close()
    (k1, h1, x1), (k0, h0, x0) = runs[1], runs[0]
    assert k1 == k0 == 12
    assert _same_bits(h1, h0) and _same_bits(x1, x0)
    assert np.isfinite(x1).all() and not np.any(x1 == 777.0)
    exec_.free(d_b), exec_.free(d_x)
    comm.close()
    exec_.close()
