"""GPU parity tests of the ring kernel's 4-bit VALUE codes (csr_lxw_ring_kernel
<..., VC = true> in spmv_lxw.hip; plan arrays lx_vcode / lx_vdict, csr_plan.h;
lxvc_encode_kernel in spmv_csr_forms.hip): a row block whose stored values have
at most 16 distinct 64-bit patterns streams one nibble per entry and a 128-byte
fp64 dictionary instead of its values.

Every comparison is np.array_equal (on the uint64 view where NaNs occur): y of
mult and of mult with the fused dot against the one-lane-per-row kernel
(plan_set("algo", 3)) of the same plan, y and the whole array of the dot's
partials against the same plan after plan_set("lx_vcode", 0).  y is prefilled
with 0xFF bytes, the partials with NaN; each case runs with beta = 0 and
beta != 0, at the default grid and with the grid capped at two workgroups
(plan_set("lxw_grid_cap")), so that the prologue, the wrap of the three slots
and the drain are all reached.  The ring is asked for by name: its default
starts at 128 steps per workgroup.

The layout case: a ring-eligible block has at most 2045 entries (lx_ring_fits:
the fp32 slot's bound, which the value-coded ring keeps), so its codes span at
most 1038 bytes with the alignment slack -- two pieces can be needed, never
filled.  The case takes the spans the rule allows: exactly one piece (1024
bytes), 13 bytes over one piece and the longest possible (1038)."""
import numpy as np
import pytest

from spmv_amd import _lib, hip

pytestmark = pytest.mark.gpu

AB = ((1.0, 0.0), (-0.5, 0.75))
ENOTSUP = -3
NO_LATTICE = 1 << 62


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _ctx():
    c = hip.Context(0)
    c.set_option("lx_min_nnz", 0)
    c.set_option("lat_min_nnz", NO_LATTICE)  # the CSR-order plan, any size
    return c


def _pattern(N, cols_of_row):
    """rowptr, colind from row -> iterable of columns (kept in the order given;
    columns outside [0, N) are dropped)."""
    rp = np.zeros(N + 1, np.int64)
    ci = []
    for r in range(N):
        ci.extend(k for k in cols_of_row(r) if 0 <= k < N)
        rp[r + 1] = len(ci)
    return rp.astype(np.int32), np.asarray(ci, np.int32)


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _most_distinct_per_block(rp, va):
    blk = _rows_of(rp) // 256
    return max(np.unique(_bits(va)[blk == b]).size for b in np.unique(blk))


BAND = (-37, -2, 0, 1, 40)


def _banded(N=5 * 256 + 100):
    return _pattern(N, lambda r: [r + d for d in BAND])


def _poisson(n):
    from spmv_amd import poisson
    rp, ci, va = poisson.poisson3d_csr(n)
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, np.float64), n ** 3)


def _bake(ctx, blk):
    rc = _lib.hip.spmv_hip_csr_plan_bake_values_f64(ctx.h, blk.plan,
                                                    blk.values.ptr, None, None)
    assert rc in (0, ENOTSUP), rc


def _block(ctx, rp, ci, va, N):
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK,
                       np.float64)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1 and blk.get("lat") == 0
    _bake(ctx, blk)
    # two workgroups per CU, the 7-point plan's figure (a plan with few entries
    # per row block has small two-slot buffers and more workgroups per CU than
    # the ring's slots allow)
    blk.set("lxw_blocks_per_cu", 2)
    return blk


def _mult(ctx, blk, dx, alpha, beta, y0, N, part):
    """One product into y prefilled with 0xFF bytes (beta == 0) or y0, the
    partials NaN-filled before the launch."""
    fill = np.frombuffer(b"\xff" * (8 * N), np.float64)
    dy = ctx.upload(fill if beta == 0 else y0)
    if part is not None:
        part.write(np.full(part.count, np.nan))
    blk.mult(alpha, dx.ptr, beta, dy.ptr,
             dot_partials=None if part is None else part.ptr)
    y = dy.numpy()
    dy.free()
    return y, (None if part is None else part.numpy().copy())


def _check(ctx, blk, N, tag, x=None, vcode=True, finite=True):
    """mult and mult with the dot, beta = 0 and != 0: the plan's DMA kernel
    (`vcode`: the value-coded ring, asserted) against the one-lane-per-row
    kernel and against lx_vcode = 0."""
    rng = np.random.default_rng(N)
    if x is None:
        x = rng.uniform(-1, 1, N)
    y0 = rng.uniform(-1, 1, N)
    dx = ctx.upload(x)
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    for alpha, beta in AB:
        blk.set("algo", hip.ALGO_SCALAR)
        y_ref, _ = _mult(ctx, blk, dx, alpha, beta, y0, N, None)
        y_ref_d, p_ref = _mult(ctx, blk, dx, alpha, beta, y0, N, part)
        blk.set("algo", hip.ALGO_ROWBLOCK)
        assert np.array_equal(_bits(y_ref_d), _bits(y_ref))
        assert np.isfinite(y_ref).all() == finite
        got = {}
        for v in ((1, 0) if vcode else (None,)):
            if v is None:  # (no value codes: the key stays as it is)
                assert blk.get("lx_vcode_all") == 0
            else:
                blk.set("lx_vcode", v)
                assert blk.get("lx_vcode") == v
            if v:
                assert blk.get("lx_vcode_all") == 1 and blk.get("lx_ring") == 1
            y, _ = _mult(ctx, blk, dx, alpha, beta, y0, N, None)
            y_d, p = _mult(ctx, blk, dx, alpha, beta, y0, N, part)
            what = tag + (alpha, beta, v)
            assert np.array_equal(_bits(y), _bits(y_ref)), what
            assert np.array_equal(_bits(y_d), _bits(y_ref)), what
            if finite:
                assert np.isfinite(p).all(), what
                # x . (alpha A x) summed over another grid: N products of
                # magnitude <= |x_i| |c_i|, each sum within N eps of the exact
                c = y_ref - beta * y0 if beta else y_ref
                bound = 2 * N * np.finfo(np.float64).eps * np.abs(x * c).sum()
                assert abs(p.sum() - p_ref.sum()) <= bound, what
            got[v] = (y_d, p)
        if vcode:
            assert np.array_equal(_bits(got[1][0]), _bits(got[0][0])), tag
            assert np.array_equal(_bits(got[1][1]), _bits(got[0][1])), tag
            blk.set("lx_vcode", 1)
    dx.free()
    part.free()


def _check_both_grids(ctx, blk, N, tag, **kw):
    nrb = (N + 255) // 256
    assert blk.get("lx_vcode_blocks") == nrb and blk.get("lx_vcode_all") == 1
    assert blk.get("lx_vcode") == 1  # on by default
    blk.set("lx_ring", 1)  # by name: these matrices are small on purpose
    for cap in (0, 2):
        blk.set("lxw_grid_cap", cap)
        assert blk.get("lx_ring") == 1
        if cap:
            assert blk.get("lxw_grid") == min(cap, nrb)
        _check(ctx, blk, N, tag + (cap,), **kw)


def _run(rp, ci, va, N, tag, v32=None, pwr4=False, **kw):
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    if v32 is not None:
        assert blk.get("lx_v32") == v32
    _check_both_grids(ctx, blk, N, tag, **kw)
    if pwr4:  # the instantiation with four x pieces per wave, under the cap
        assert blk.get("lx_ring_pwr") == 3
        blk.set("lx_ring_pwr", 4)
        _check(ctx, blk, N, tag + ("pwr4",), **kw)
    blk.free()
    ctx.close()


def test_vcode_poisson():
    """12^3: 6.75 row blocks, 3.5 per workgroup under the cap; two values."""
    rp, ci, va, N = _poisson(12)
    assert _most_distinct_per_block(rp, va) == 2
    _run(rp, ci, va, N, ("poisson",), v32=1, pwr4=True)


def test_vcode_values_not_exact_in_fp32():
    """0.1, 1/3, pi, ...: the fp32 copy is refused, the value-coded ring runs."""
    rp, ci = _banded()
    pool = np.array([0.1, 1 / 3, np.pi, -np.e, 1e-3, 7.0 / 9.0, -0.3])
    va = pool[np.random.default_rng(3).integers(0, len(pool), len(ci))]
    _run(rp, ci, va, len(rp) - 1, ("inexact",), v32=0, pwr4=True)


def _sixteen(extra):
    """The banded matrix, block 2 with exactly 16 distinct values (`extra`: a
    17th in one entry of it), every other block with three."""
    rp, ci = _banded()
    rows = _rows_of(rp)
    rng = np.random.default_rng(16)
    va = rng.integers(1, 4, len(ci)) / 4.0
    j2 = np.flatnonzero(rows // 256 == 2)
    va[j2] = (1 + np.arange(len(j2)) % 16) / 8.0
    if extra:
        va[j2[len(j2) // 2]] = 17 / 8.0
    return rp, ci, va, len(rp) - 1


def test_vcode_sixteen_values_in_a_block():
    rp, ci, va, N = _sixteen(False)
    assert _most_distinct_per_block(rp, va) == 16
    _run(rp, ci, va, N, ("16",))


def test_vcode_seventeen_values_in_a_block():
    """One block past the dictionary: no value codes, the plan's other kernel
    (here the ring on the fp32 copy) gives the right answer."""
    rp, ci, va, N = _sixteen(True)
    assert _most_distinct_per_block(rp, va) == 17
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx_vcode_all") == 0 and blk.get("lx_vcode") == 0
    assert blk.get("lx_vcode_blocks") == (N + 255) // 256 - 1
    assert blk.get("lx_v32") == 1
    blk.set("lx_ring", 1)
    for cap in (0, 2):
        blk.set("lxw_grid_cap", cap)
        _check(ctx, blk, N, ("17", cap), vcode=False)
    blk.free()
    ctx.close()


def _special():
    """The banded matrix with +0.0 and -0.0, +-Inf, a quiet NaN, two subnormals,
    +-1e308 and ordinary numbers in the dictionaries of row blocks 0 and 1 (the
    other blocks: all but the NaN); x holds +-0, Inf and 1e10 (1e308 * 1e10
    overflows).  Which of two DIFFERENT NaNs an addition returns is left open
    by IEEE 754 and changes when a compiler commutes the operands, so kernels
    that agree operation for operation may still differ there.  The case
    keeps every row to ONE NaN pattern: the even rows below 600 hold the
    stored NaN and nothing that makes an invalid operation (no Inf, no 1e308
    among their values, no Inf or 1e10 among their x: those sit at columns
    from 700 on), every other row holds no stored NaN and meets only the NaN
    the hardware makes for Inf - Inf and 0 * Inf."""
    rp, ci = _banded()
    N = len(rp) - 1
    rows = _rows_of(rp)
    tame = np.array([0.0, -0.0, 5e-324, -3e-310, 1.0, -2.5, 0.1, np.nan])
    wild = np.array([0.0, -0.0, 5e-324, -3e-310, 1.0, -2.5, 0.1, np.inf,
                     -np.inf, 1e308, -1e308])
    rng = np.random.default_rng(8)
    # mostly ordinary numbers, so that many rows stay finite
    few = rng.random(len(ci)) < 0.25
    va = np.where(few, wild[rng.integers(0, len(wild), len(ci))],
                  wild[rng.integers(4, 7, len(ci))])
    nan_row = (rows < 600) & (rows % 2 == 0)
    va[nan_row] = np.where(few, tame[rng.integers(0, len(tame), len(ci))],
                           tame[rng.integers(4, 7, len(ci))])[nan_row]
    for b in (0, 1):
        assert np.unique(_bits(va[rows // 256 == b])).size == 12
    x = rng.uniform(-1, 1, N)
    x[rng.choice(N, 60, replace=False)] = 0.0
    x[rng.choice(N, 60, replace=False)] = -0.0
    x[700 + rng.choice(N - 700, 10, replace=False)] = np.inf
    x[700 + rng.choice(N - 700, 40, replace=False)] = 1e10
    assert ci[nan_row].max() < 700
    return rp, ci, va, N, x


def test_vcode_special_values():
    """Bits compared; see _special."""
    rp, ci, va, N, x = _special()
    _run(rp, ci, va, N, ("special",), v32=0, x=x, finite=False)


def _layout():
    """Block 0: 258 entries; blocks 1-3: 2045 entries each (253 rows of eight,
    three of seven, on the diagonals -4..3), the most a ring block holds;
    block 4: partial.  Their spans start at entries 258, 2303 and 4348: the
    16-byte chunks around their codes hold 1024, 1038 and 1037 bytes."""
    N = 4 * 256 + 52

    def cols(r):
        b, t = divmod(r, 256)
        if b == 0:
            return [r, r + 1] if t < 2 else [r]
        if b < 4:
            return [r + d for d in range(-4, 4 if t >= 3 else 3)]
        return [r - 1, r, r + 1]
    rp, ci = _pattern(N, cols)
    spans = []
    for b in (1, 2, 3):
        a, e = int(rp[256 * b]), int(rp[256 * b + 256])
        assert e - a == 2045
        spans.append(((e + 1) >> 1) - ((a >> 1) & ~15))
    assert spans == [1024, 1038, 1037]
    va = (1 + np.random.default_rng(4).integers(0, 16, len(ci))) / 16.0
    return rp, ci, va, N


def test_vcode_layout_boundaries():
    _run(*_layout(), ("layout",), pwr4=True)


def test_vcode_one_block_matrix():
    N = 200
    rp, ci = _pattern(N, lambda r: [r - 1, r, r + 1])
    va = np.where(ci == _rows_of(rp), 2.0, -1.0) + 0.1
    _run(rp, ci, va, N, ("one block",), v32=0)


def test_vcode_neighbouring_dictionaries_differ():
    """The value set changes with every row block: a slot's dictionary is not
    read by a neighbour's row sum."""
    rp, ci = _banded(9 * 256 + 20)
    blk_of = _rows_of(rp) // 256
    rng = np.random.default_rng(12)
    va = (blk_of + 1) * 100.0 + rng.integers(0, 5 + blk_of % 7, len(ci)) * 0.1
    assert np.unique(va[blk_of == 3]).size != np.unique(va[blk_of == 4]).size
    assert not np.intersect1d(va[blk_of == 3], va[blk_of == 4]).size
    _run(rp, ci, va, len(rp) - 1, ("neighbours",), v32=0)


def test_vcode_rebake():
    """Values baked again after the first apply: more than 16 distinct in one
    block, then back -- lx_vcode_all follows and the results follow."""
    rp, ci, va, N = _poisson(12)
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    _check_both_grids(ctx, blk, N, ("first",))
    va2 = va.copy()
    j1 = np.flatnonzero(_rows_of(rp) // 256 == 1)
    va2[j1[:40]] = np.random.default_rng(1).uniform(1, 2, 40)
    assert _most_distinct_per_block(rp, va2) > 16
    blk.values.write(va2)
    _bake(ctx, blk)
    assert blk.get("lx_vcode_all") == 0 and blk.get("lx_vcode") == 0
    assert blk.get("lx_v32") == 0
    _check(ctx, blk, N, ("many values",), vcode=False)
    va3 = va * 0.1  # two values again, not exact in fp32
    blk.values.write(va3)
    _bake(ctx, blk)
    assert blk.get("lx_v32") == 0
    _check_both_grids(ctx, blk, N, ("back",))
    blk.free()
    ctx.close()
