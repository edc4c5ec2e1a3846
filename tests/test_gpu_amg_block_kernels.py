"""The five block kernels of hip/spmv_amg_block.hip launched ALONE through the
C ABI (spmv_hip_*_block_f64) and compared bit for bit, column by column, with
the numpy restatements of the single-vector kernels (amg_kernel_cases.py; one
rounding per operation; special_values.same_bits: NaN where and only where the
restatement has one).

Widths 1..8 (2, 4, 8: the streaming form; the others and every block that is
only 8-byte aligned: one thread per row), cached and non-temporal.  Every
output lies between guard words, every input is read back unchanged.  The
columns of a block carry DIFFERENT recipes -- benign, NaN, +-Inf, signed zeros,
values that overflow, subnormals -- so a kernel that mixed two columns, or let
one column's special values leak into its neighbour, could not pass.

Rows: 1, 2, 3; per width the rows at which rows * K / 2 16-byte elements are
one below, exactly and one above 256 (what the lanes of a workgroup load in one
pass) and 1 024 (a workgroup's unit, kUnit of blas1_stream.h); and one length
beyond a pass of the streaming grid (8 workgroups per CU, read from the device).
Aggregates: a single member, 130 members (the arrow matrix's), and a coarse
level of one row."""
import numpy as np
import pytest

import amg_kernel_cases as kc
import test_gpu_amg as ta
import test_gpu_pcg as tp
from spmv_amd import _lib
from test_gpu_amg_kernels import Pool, kexec, nt, pool  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

hip = _lib.hip
EINVAL = ta.EINVAL
WIDTHS = tuple(range(1, 9))
TINY = 5e-324


def rows_for(K):
    out = {1, 2, 3}
    for target in (kc.BLOCK, kc.UNIT):  # in 16-byte elements
        r = -(-2 * target // K)
        out |= {max(r - 1, 1), r, r + 1}
    return sorted(out)


def recipe(c, v, seed):
    """column c of a block: the vector v dressed by the c-th recipe"""
    v = np.array(v, np.float64)
    n = len(v)
    kind = c % 6
    if kind == 1:
        v[::max(1, n // 5)] = np.nan
    elif kind == 2:
        v[::max(1, n // 4)] = np.inf
        v[1::max(1, n // 4)] = -np.inf
    elif kind == 3:
        v[::2] = kc.NZ
        v[1::4] = 0.0
    elif kind == 4:
        v = v * 1.7e308
    elif kind == 5:
        v = np.round(v * 9) * TINY
    return v


def block(n, K, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return np.stack([recipe(c, rng.uniform(lo, hi, n), seed + c)
                     for c in range(K)], axis=1)


def flat(B):
    return np.ascontiguousarray(B).reshape(-1)


def dinv_of(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 3.0, n)
    if n >= 3:
        d[n // 2] = np.inf  # (a subnormal diagonal entry)
    return d


# ---- the restatements: the single-vector ones, column by column ----------------------
def apply0_ref(b0, R, dinv):
    with np.errstate(all="ignore"):
        return np.float64(b0) * (dinv[:, None] * R)


def step_ref(a, b, W, R, dinv, D, Z):
    with np.errstate(all="ignore"):
        t = np.float64(b) * (dinv[:, None] * (R - W))
        e = np.float64(a) * D + t
        return e, Z + e


def post0_ref(b0, W, R, dinv, Z):
    cols = [kc.post0_ref(b0, W[:, c], R[:, c], dinv, Z[:, c])
            for c in range(W.shape[1])]
    return (np.stack([d for d, _ in cols], axis=1),
            np.stack([z for _, z in cols], axis=1))


# ---- the three streaming kernels ---------------------------------------------------------
def _streaming(pool, n, K, off):
    ctx = pool.e.context
    W, R, D, Z = (block(n, K, 10 * n + K + s) for s in (1, 2, 3, 4))
    dinv_h = dinv_of(n, n + K)
    w, r = pool.vec(flat(W), off), pool.vec(flat(R), off)
    dinv = pool.vec(dinv_h, 1 - off)  # (shared by the columns, any alignment)
    what = (n, K, off)
    for with_d in (True, False):
        z, d = pool.out(n * K, off), pool.out(n * K, off)
        rc = hip.spmv_hip_cheb_apply0_block_f64(ctx, n, K, 0.75, r.ptr, dinv.ptr,
                                                d.ptr if with_d else None, z.ptr,
                                                None)
        assert rc == 0, ("apply0", what)
        want = apply0_ref(0.75, R, dinv_h)
        z.expect(flat(want), ("apply0 z", what, with_d))
        (d.expect(flat(want), ("apply0 d", what)) if with_d
         else d.unchanged(("apply0: d written", what)))
    for last in (0, 1):
        z, d = pool.vec(flat(Z), off), pool.vec(flat(D), off)
        rc = hip.spmv_hip_cheb_step_block_f64(ctx, n, K, 0.3, -1.25, last, w.ptr,
                                              r.ptr, dinv.ptr, d.ptr, z.ptr, None)
        assert rc == 0, ("step", what)
        want_d, want_z = step_ref(0.3, -1.25, W, R, dinv_h, D, Z)
        z.expect(flat(want_z), ("step z", what, last))
        (d.unchanged(("step: last wrote d", what)) if last
         else d.expect(flat(want_d), ("step d", what)))
    for with_d in (True, False):
        z, d = pool.vec(flat(Z), off), pool.out(n * K, off)
        rc = hip.spmv_hip_amg_post0_block_f64(ctx, n, K, 1.5, w.ptr, r.ptr,
                                              dinv.ptr, d.ptr if with_d else None,
                                              z.ptr, None)
        assert rc == 0, ("post0", what)
        want_d, want_z = post0_ref(1.5, W, R, dinv_h, Z)
        z.expect(flat(want_z), ("post0 z", what, with_d))
        (d.expect(flat(want_d), ("post0 d", what)) if with_d
         else d.unchanged(("post0: d written", what)))
    for v in (w, r, dinv):
        v.unchanged(what)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "8off"])
@pytest.mark.parametrize("K", WIDTHS)
def test_streaming_kernels(kexec, nt, K, off):  # noqa: F811
    for n in rows_for(K):
        p = Pool(kexec)
        try:
            _streaming(p, n, K, off)
        finally:
            p.close()


def test_one_unaligned_block_sends_a_native_width_to_the_row_form(pool):  # noqa: F811
    """only z is 8 bytes off: the same bits, no 16-byte access to it"""
    n, K, ctx = 301, 4, pool.e.context
    R = block(n, K, 5)
    dinv_h = dinv_of(n, 6)
    r, dinv = pool.vec(flat(R)), pool.vec(dinv_h)
    z, d = pool.out(n * K, 1), pool.out(n * K)
    assert hip.spmv_hip_cheb_apply0_block_f64(ctx, n, K, 2.0, r.ptr, dinv.ptr,
                                              d.ptr, z.ptr, None) == 0
    want = flat(apply0_ref(2.0, R, dinv_h))
    z.expect(want, "z"), d.expect(want, "d")


@pytest.mark.parametrize("K", [2, 3, 8])
def test_streaming_beyond_one_pass_of_the_grid(pool, K):  # noqa: F811
    cus = pool.e.num_cus
    if K == 3:  # one thread per row: a pass is grid_cap workgroups of 256 rows
        n = kc.grid_cap(cus) * kc.BLOCK + 300
        assert n > kc.grid_cap(cus) * kc.BLOCK
    else:
        n = (2 * kc.grid_cap(cus) * kc.UNIT) // K + kc.UNIT + 3
        assert n * K // 2 > kc.grid_cap(cus) * kc.UNIT
    ctx = pool.e.context
    rng = np.random.default_rng(K)
    W, R, D, Z = (rng.uniform(-1, 1, (n, K)) for _ in range(4))
    dinv_h = rng.uniform(0.2, 3.0, n)
    w, r, dinv = pool.vec(flat(W)), pool.vec(flat(R)), pool.vec(dinv_h)
    z, d = pool.vec(flat(Z)), pool.vec(flat(D))
    assert hip.spmv_hip_cheb_step_block_f64(ctx, n, K, 0.3, -1.25, 0, w.ptr,
                                            r.ptr, dinv.ptr, d.ptr, z.ptr,
                                            None) == 0
    want_d, want_z = step_ref(0.3, -1.25, W, R, dinv_h, D, Z)
    z.expect(flat(want_z), ("wrap z", K)), d.expect(flat(want_d), ("wrap d", K))


# ---- restrict and prolong -------------------------------------------------------------------
def steps():
    """(name, step): sizes 1 and 130 among small ones, scattered; one aggregate
    of everything (a coarse level of one row); lengths round a workgroup"""
    out = [("one130", kc.make_step(kc._agg_of_sizes(
        np.array([1, 130, 2, 3, 1, 7]), 4))),
        ("single", kc.make_step(np.zeros(1, np.int64))),
        ("onerow", kc.make_step(np.zeros(5, np.int64)))]
    for nc in (255, 256, 257):
        rng = np.random.default_rng(nc)
        out.append((f"aggregates{nc}", kc.make_step(kc._agg_of_sizes(
            rng.integers(1, 4, nc), nc + 1))))
    return out


def _restrict(pool, name, step, K, off):
    n, nc = step["fine_rows"], step["coarse_rows"]
    R, W = block(n, K, n + K), block(n, K, n + K + 50)
    if n >= 3:  # r == w: +0.0 ; -0.0 - +0.0 = -0.0
        W[0, :] = R[0, :]
        R[2, :], W[2, :] = kc.NZ, 0.0
    plan = pool.plan(step)
    r, w = pool.vec(flat(R), off), pool.vec(flat(W), off)
    out = pool.out(nc * K, off)
    rc = hip.spmv_hip_amg_restrict_block_f64(pool.e.context, plan, K, r.ptr,
                                             w.ptr, out.ptr, None)
    assert rc == 0, (name, K, off)
    want = np.stack([kc.restrict_ref(step, R[:, c], W[:, c]) for c in range(K)],
                    axis=1)
    out.expect(flat(want), ("restrict", name, K, off))
    r.unchanged(name), w.unchanged(name)


def _prolong(pool, name, step, K, off):
    n, nc = step["fine_rows"], step["coarse_rows"]
    E, Z = block(nc, K, nc + K), block(n, K, n + K + 7)
    plan = pool.plan(step)
    e = pool.vec(flat(E), off)
    for scale in (1.0, 1.6, -0.0):
        z = pool.vec(flat(Z), off)
        rc = hip.spmv_hip_amg_prolong_block_f64(pool.e.context, plan, K,
                                                float(scale), e.ptr, z.ptr, None)
        assert rc == 0, (name, K, off)
        want = np.stack([kc.prolong_ref(step, scale, E[:, c], Z[:, c])
                         for c in range(K)], axis=1)
        z.expect(flat(want), ("prolong", name, K, off, scale))
    e.unchanged(name)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "8off"])
@pytest.mark.parametrize("K", WIDTHS)
def test_restrict_and_prolong(kexec, nt, K, off):  # noqa: F811
    for name, step in steps():
        p = Pool(kexec)
        try:
            _restrict(p, name, step, K, off)
            _prolong(p, name, step, K, off)
        finally:
            p.close()


@pytest.mark.parametrize("K", WIDTHS)
def test_prolong_at_the_streaming_lengths(kexec, nt, K):  # noqa: F811
    for n in rows_for(K):
        p = Pool(kexec)
        try:
            _prolong(p, f"rows{n}", kc.prolong_case(n)[0], K, 0)
        finally:
            p.close()


@pytest.mark.parametrize("K", [3, 8])
def test_restrict_and_prolong_beyond_one_pass_of_the_grid(pool, K):  # noqa: F811
    cus = pool.e.num_cus
    nc = kc.grid_cap(cus) * kc.BLOCK + 300
    rng = np.random.default_rng(8)
    step = kc.make_step(kc._agg_of_sizes(rng.integers(1, 3, nc), 9))
    n = step["fine_rows"]
    if K == 8:
        assert n * K // 2 > kc.grid_cap(cus) * kc.UNIT
    R, W = rng.uniform(-1, 1, (n, K)), rng.uniform(-1, 1, (n, K))
    plan = pool.plan(step)
    r, w, out = pool.vec(flat(R)), pool.vec(flat(W)), pool.out(nc * K)
    assert hip.spmv_hip_amg_restrict_block_f64(pool.e.context, plan, K, r.ptr,
                                               w.ptr, out.ptr, None) == 0
    want = np.stack([kc.restrict_ref(step, R[:, c], W[:, c]) for c in range(K)],
                    axis=1)
    out.expect(flat(want), ("restrict wrap", K))
    E = rng.uniform(-1, 1, (nc, K))
    e, z = pool.vec(flat(E)), pool.vec(flat(R))
    assert hip.spmv_hip_amg_prolong_block_f64(pool.e.context, plan, K, 1.6, e.ptr,
                                              z.ptr, None) == 0
    want = np.stack([kc.prolong_ref(step, 1.6, E[:, c], R[:, c])
                     for c in range(K)], axis=1)
    z.expect(flat(want), ("prolong wrap", K))


# ---- what the entry points refuse -------------------------------------------------------------
def test_refused_arguments(pool):  # noqa: F811
    ctx, n = pool.e.context, 40
    step = kc.prolong_case(n)[0]
    plan = pool.plan(step)
    v = [pool.vec(np.ones(n * 8)) for _ in range(5)]
    w, r, dinv, d, z = (x.ptr for x in v)
    for nrhs in (0, 9, -2):
        assert hip.spmv_hip_cheb_apply0_block_f64(ctx, n, nrhs, 1.0, r, dinv, d,
                                                  z, None) == EINVAL
        assert hip.spmv_hip_cheb_step_block_f64(ctx, n, nrhs, 1.0, 1.0, 0, w, r,
                                                dinv, d, z, None) == EINVAL
        assert hip.spmv_hip_amg_post0_block_f64(ctx, n, nrhs, 1.0, w, r, dinv, d,
                                                z, None) == EINVAL
        assert hip.spmv_hip_amg_restrict_block_f64(ctx, plan, nrhs, r, w, z,
                                                   None) == EINVAL
        assert hip.spmv_hip_amg_prolong_block_f64(ctx, plan, nrhs, 1.0, r, z,
                                                  None) == EINVAL
    assert hip.spmv_hip_cheb_apply0_block_f64(ctx, n, 4, 1.0, r, None, d, z,
                                              None) == EINVAL
    assert hip.spmv_hip_cheb_apply0_block_f64(ctx, -1, 4, 1.0, r, dinv, d, z,
                                              None) == EINVAL
    assert hip.spmv_hip_cheb_step_block_f64(ctx, n, 4, 1.0, 1.0, 1, w, r, dinv,
                                            None, z, None) == EINVAL
    assert hip.spmv_hip_amg_post0_block_f64(ctx, n, 4, 1.0, None, r, dinv, d, z,
                                            None) == EINVAL
    assert hip.spmv_hip_amg_restrict_block_f64(ctx, None, 4, r, w, z,
                                               None) == EINVAL
    assert hip.spmv_hip_amg_prolong_block_f64(ctx, plan, 4, 1.0, None, z,
                                              None) == EINVAL
    # n == 0: nothing is launched, nothing is required
    assert hip.spmv_hip_cheb_apply0_block_f64(ctx, 0, 4, 1.0, None, None, None,
                                              None, None) == 0
    pool.e.synchronize()
    for x in v:
        x.unchanged("refused")
