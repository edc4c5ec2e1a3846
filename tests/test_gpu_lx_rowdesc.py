"""GPU parity tests of the ring kernel's row descriptors (csr_lxw_ring_kernel in
spmv_lxw.hip; plan array "lx_rowdesc", csr_plan.h): a row's span inside its
block's values slot comes from one 16-bit word that arrives by LDS-DMA -- bits
0..10 the row's first entry relative to the block's span start, bits 11..15 its
length (at most 31) -- instead of two row-pointer loads.

Every comparison is np.array_equal: y of mult and of mult with the fused dot
against the one-lane-per-row kernel (plan_set("algo", 3)) of the same plan, y
and the whole array of the dot's partials against the same plan after
plan_set("lx_ring", 0).  (The one-lane-per-row kernel sums the dot over another
grid, so its partials are other numbers; only their total is compared with it,
within the rounding of a sum of N terms.)  y is prefilled with 0xFF bytes, the
partials with NaN; each case runs with beta = 0 and beta != 0, at the default
grid and with the grid capped at two workgroups (plan_set("lxw_grid_cap")), so
that a small matrix gives a workgroup many row blocks and the ring wraps.

A row block of a coded plan has at most 16 distinct (column - row), so a row
reaches the descriptor's 31 entries only with repeated columns; the two limit
cases store one row's 16 columns again and again.  A row block without any entry is
not ring-eligible (lx_ring_fits wants entries), so the matrix with such a block
checks the answer of the kernel the plan falls back to."""
import numpy as np
import pytest

from spmv_amd import _lib, hip, host, poisson

pytestmark = pytest.mark.gpu

AB = ((1.0, 0.0), (-0.5, 0.75))
ENOTSUP = -3
NO_LATTICE = 1 << 62
DESC_MAX_LEN = 31


def _ctx():
    c = hip.Context(0)
    c.set_option("lx_min_nnz", 0)
    c.set_option("lat_min_nnz", NO_LATTICE)  # the CSR-order plan, any size
    return c


def _quarters(rng, n):
    """Values k / 4, k in [-32, 32] without 0: exact in fp32."""
    return rng.integers(1, 33, n) * rng.choice((-1, 1), n) / 4.0


def _from_rows(N, cols_of_row, seed):
    """CSR from row -> iterable of columns (kept in the order given; columns
    outside [0, N) are dropped)."""
    rp = np.zeros(N + 1, np.int64)
    ci = []
    for r in range(N):
        c = [k for k in cols_of_row(r) if 0 <= k < N]
        ci.extend(c)
        rp[r + 1] = len(ci)
    rng = np.random.default_rng(seed)
    return (rp.astype(np.int32), np.asarray(ci, np.int32),
            _quarters(rng, len(ci)), N)


def _poisson(n):
    rp, ci, va = poisson.poisson3d_csr(n)
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, np.float64), n ** 3)


BAND = (-37, -2, 0, 1, 40)


def _banded_empty_rows(with_empty_block):
    """Five full row blocks and a partial one on five diagonals.  Empty: row 0,
    the first and the last row of block 1, every third row of block 3, the
    matrix's last row -- and, asked for, all of block 2."""
    N = 5 * 256 + 100

    def cols(r):
        b, t = divmod(r, 256)
        if r in (0, N - 1) or (b == 1 and t in (0, 255)) or (b == 3 and t % 3 == 0):
            return ()
        if with_empty_block and b == 2:
            return ()
        return [r + d for d in BAND]
    return _from_rows(N, cols, 11 + with_empty_block)


D16 = tuple(range(-8, 8))


def _rows_8_9_16():
    """Rows of 16, 9, 8 and 4 entries by row % 8 on 16 diagonals (6.6 per row:
    a block's entries fit the ring's values slot)."""
    N = 4 * 256 + 60
    lens = (16, 9, 8, 4, 4, 4, 4, 4)

    def cols(r):
        n = lens[r % 8]
        return [r + d for d in D16[(16 - n) // 2:(16 - n) // 2 + n]]
    return _from_rows(N, cols, 21)


def _long_row(length):
    """Three diagonals, and one row in the middle of block 1 with `length`
    entries: its 16 columns r - 8 .. r + 7, stored again and again."""
    N = 3 * 256 + 40
    long_r = 256 + 130

    def cols(r):
        if r == long_r:
            return [r + D16[k % 16] for k in range(length)]
        return [r - 1, r, r + 1]
    return _from_rows(N, cols, 31 + length)


def _every_residue():
    """34 row blocks of 3 * 256 + 1 entries (three diagonals, one more entry in
    one row of each block): the span starts take every residue mod 32."""
    N = 34 * 256

    def cols(r):
        c = [r - 1, r, r + 1]
        if r % 256 == 77:
            c.append(r + 5)
        return c
    m = _from_rows(N, cols, 41)
    assert np.unique(m[0][:-1:256] % 32).size == 32
    return m


def _block(ctx, rp, ci, va, N):
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False, hip.ALGO_ROWBLOCK,
                       np.float64)
    assert blk.get("lx") == 1 and blk.get("lxw") == 1 and blk.get("lat") == 0
    rc = _lib.hip.spmv_hip_csr_plan_bake_values_f64(ctx.h, blk.plan,
                                                    blk.values.ptr, None, None)
    assert rc in (0, ENOTSUP), rc
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


def _check(ctx, blk, m, tag, ring=True):
    """mult and mult with the dot, beta = 0 and != 0: the plan's DMA kernel
    (`ring`: the ring kernel, asserted) against the one-lane-per-row kernel and
    against lx_ring = 0."""
    rp, ci, va, N = m
    rng = np.random.default_rng(N)
    x, y0 = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    dx = ctx.upload(x)
    part = ctx.empty(ctx.dot_partials_len, np.float64)
    for alpha, beta in AB:
        blk.set("algo", hip.ALGO_SCALAR)
        y_ref, _ = _mult(ctx, blk, dx, alpha, beta, y0, N, None)
        y_ref_d, p_ref = _mult(ctx, blk, dx, alpha, beta, y0, N, part)
        blk.set("algo", hip.ALGO_ROWBLOCK)
        assert np.array_equal(y_ref_d, y_ref) and np.isfinite(y_ref).all()
        got = {}
        for r in ((1, 0) if ring else (0,)):
            blk.set("lx_ring", r)
            assert blk.get("lx_ring") == r
            y, _ = _mult(ctx, blk, dx, alpha, beta, y0, N, None)
            y_d, p = _mult(ctx, blk, dx, alpha, beta, y0, N, part)
            what = tag + (alpha, beta, r)
            assert np.array_equal(y, y_ref), what
            assert np.array_equal(y_d, y_ref), what
            assert np.isfinite(p).all(), what
            # x . (alpha A x) summed over another grid: N products of
            # magnitude <= |x_i| |c_i|, each sum within N eps of the exact one
            c = y_ref - beta * y0 if beta else y_ref
            bound = 2 * N * np.finfo(np.float64).eps * np.abs(x * c).sum()
            assert abs(p.sum() - p_ref.sum()) <= bound, what
            got[r] = (y_d, p)
        if ring:
            assert np.array_equal(got[1][0], got[0][0]), tag
            assert np.array_equal(got[1][1], got[0][1]), tag
            blk.set("lx_ring", 1)
    dx.free()
    part.free()


def _check_ring_both_grids(m, tag):
    rp, ci, va, N = m
    nrb = (N + 255) // 256
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx_rowdesc") == 1
    assert blk.get("lx_v32") == 1 and blk.get("lx4") == 1
    assert blk.get("lx_ring_blocks") == nrb, (tag, blk.get("lx_ring_blocks"))
    # two workgroups per CU, the 7-point plan's figure: a plan with few entries
    # per row block has small two-slot buffers, more workgroups per CU than
    # the ring's fixed 8-KiB value slots allow, and keeps the two-slot kernel
    blk.set("lxw_blocks_per_cu", 2)
    blk.set("lx_ring", 1)  # by name: these matrices are small on purpose
    for cap in (0, 2):
        blk.set("lxw_grid_cap", cap)
        assert blk.get("lx_ring") == 1
        if cap:
            assert blk.get("lxw_grid") == min(cap, nrb)
        _check(ctx, blk, m, (tag, cap))
    # (these plans stage at most 12 x pieces: three per wave by default) the
    # instantiation with four x pieces per wave, still under the cap
    assert blk.get("lx_ring_pwr") == 3
    blk.set("lx_ring_pwr", 4)
    assert blk.get("lx_ring_pwr") == 4
    _check(ctx, blk, m, (tag, "pwr4"))
    blk.free()
    ctx.close()


@pytest.mark.parametrize("n", [8, 12, 24])
def test_rowdesc_poisson(n):
    """8^3: two row blocks (a workgroup has fewer than three); 12^3: 6.75 row
    blocks, the last one partial; 24^3: 54, 27 per workgroup under the cap --
    the ring wraps nine times."""
    _check_ring_both_grids(_poisson(n), ("poisson", n))


def test_rowdesc_empty_rows():
    """Empty first and last rows of a block, runs of empty rows, an empty
    first and last row of the matrix."""
    m = _banded_empty_rows(False)
    rp = m[0]
    assert rp[257] == rp[256] and rp[512] == rp[511] and rp[1] == 0
    _check_ring_both_grids(m, ("empty rows",))


def test_rowdesc_block_of_empty_rows():
    """A row block without entries is not ring-eligible: lx_ring cannot be
    set, and the plan's two-slot kernel gives the right answer."""
    m = _banded_empty_rows(True)
    rp, ci, va, N = m
    assert rp[768] == rp[512]
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx_ring_blocks") < (N + 255) // 256
    assert blk.get("lx_ring") == 0
    with pytest.raises(Exception):
        blk.set("lx_ring", 1)
    _check(ctx, blk, m, ("empty block",), ring=False)
    blk.free()
    ctx.close()


def test_rowdesc_rows_of_8_9_16():
    """Rows that end at, one past and two trips past the 8-entry trip of the
    row sum."""
    m = _rows_8_9_16()
    assert {8, 9, 16} <= set(np.diff(m[0]).tolist())
    _check_ring_both_grids(m, ("8 9 16",))


def test_rowdesc_row_at_the_length_limit():
    m = _long_row(DESC_MAX_LEN)
    assert np.diff(m[0]).max() == DESC_MAX_LEN
    _check_ring_both_grids(m, ("limit",))


def test_rowdesc_row_past_the_length_limit():
    """One row of 32 entries: its block is not counted, the plan keeps the
    two-slot kernel and gives the right answer."""
    m = _long_row(DESC_MAX_LEN + 1)
    rp, ci, va, N = m
    nrb = (N + 255) // 256
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    assert blk.get("lx4_blocks") == nrb  # coded all the same
    assert blk.get("lx_ring_blocks") == nrb - 1
    assert blk.get("lx_ring") == 0
    with pytest.raises(Exception):
        blk.set("lx_ring", 1)
    _check(ctx, blk, m, ("past the limit",), ring=False)
    blk.free()
    ctx.close()


def test_rowdesc_every_residue_of_the_span_start():
    _check_ring_both_grids(_every_residue(), ("residues",))


def test_rowdesc_values_changed():
    """New values written in place, plan_values_changed: the descriptors (they
    depend on the pattern alone) stay, the ring kernel stays and multiplies
    the new values."""
    rp, ci, va, N = _poisson(12)
    ctx = _ctx()
    blk = _block(ctx, rp, ci, va, N)
    blk.set("lx_ring", 1)
    blk.set("lxw_grid_cap", 2)
    va2 = _quarters(np.random.default_rng(5), len(va))
    blk.values.write(va2)
    blk.values_changed()
    assert blk.get("lx_rowdesc") == 1 and blk.get("lx_v32") == 1
    assert blk.get("lx_ring_blocks") == (N + 255) // 256
    assert blk.get("lx_ring") == 1
    _check(ctx, blk, (rp, ci, va2, N), ("values_changed",))
    blk.free()
    ctx.close()


def test_rowdesc_cg_same_history_and_x():
    """host.cg_ex on 24^3, 30 iterations with the history, eight workgroups (7
    row blocks each): the context option lx_ring 2 (no gate on the steps),
    then 0 -- history and x keep their bits."""
    import oracle
    rp, ci, va, N = _poisson(24)
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
        A.plan_set("lxw_grid_cap", 8)
        assert A.plan_get("lx_rowdesc") == 1 and A.plan_get("lx_v32") == 1
        assert A.plan_get("lx_ring") == ring
        ws = host.CgWorkspace(exec_)
        exec_.copy_from_host(d_x, np.full(N, 777.0))
        k, hist, _, _ = host.cg_ex(comm, exec_, A, d_b, d_x, 30, 0.0, ws,
                                   history=True)
        runs[ring] = (k, hist.copy(), exec_.copy_to_host(d_x, N))
        ws.close()
        A.close()
    (k1, h1, x1), (k0, h0, x0) = runs[1], runs[0]
    assert k1 == k0 == 30
    assert np.array_equal(h1, h0) and np.array_equal(x1, x0)
    assert np.isfinite(x1).all() and not np.any(x1 == 777.0)
    exec_.free(d_b), exec_.free(d_x)
    comm.close()
    exec_.close()
