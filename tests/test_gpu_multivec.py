"""GPU tests of the multi-vector product (Matrix::mult_block): the native
kernel and the per-column fallback, every storage and plan form, bit for bit
against the oracle's single-vector product applied column by column on the CPU
(never against the library's own mult); the interleave / de-interleave / block
pack kernels; update_block + mult_block on 1-3 ranks in every model."""
import numpy as np
import pytest

import oracle
from spmv_amd import _lib, hip, host, poisson
from util import lower_split

pytestmark = pytest.mark.gpu

EINVAL = -1
KS = (1, 2, 3, 4, 5, 8, 16)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.synchronize()
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ref_block(rp, ci, va, X, alpha, beta, Y0, diag=None):
    """the oracle's single-vector product, column by column; X is n x k (its
    C order IS the interleaved layout).  beta == 0: Y is write-only, the result
    is alpha * sum itself (the oracle's `+ 0 * out` would turn the -0.0 of an
    empty row into +0.0), as in test_gpu_transpose.ref_t."""
    dt = X.dtype
    cols = []
    for c in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, c])
        y0 = None if beta == 0 else np.ascontiguousarray(Y0[:, c])
        a, b = (1.0, 0.0) if beta == 0 else (alpha, beta)
        if diag is None:
            y = oracle.csr_spmv(rp, ci, va, x, a, b, y0)
        else:
            y = oracle.csr_spmv_sym(rp, ci, va, diag, x, a, b, y0)
        if beta == 0:
            y = (dt.type(alpha) * np.asarray(y, dt)).astype(dt)
        cols.append(np.asarray(y, dt))
    return np.stack(cols, axis=1)


def run_m(ctx, blk, X, alpha, beta, Y0, nrows, values=None, mixed=False):
    """one multm through the C ABI; the output is NaN-poisoned when beta == 0"""
    k = X.shape[1]
    dt = X.dtype
    d_x = ctx.upload(X)
    d_y = ctx.upload(np.full((nrows, k), np.nan, dt) if beta == 0 else Y0)
    blk.multm(alpha, d_x.ptr, beta, d_y.ptr, k, values=values, mixed=mixed)
    ctx.synchronize()
    Y = d_y.numpy().reshape(nrows, k)
    d_x.free(), d_y.free()
    return Y


def random_block(rng, nrows, ncols, dtype):
    """empty rows, duplicate columns, a few rows of more than 2000 entries, odd
    row starts and an odd nnz (8 nnz and the row starts are not multiples of
    16 bytes)"""
    lens = rng.integers(0, 12, nrows)
    lens[rng.random(nrows) < 0.1] = 0
    lens[0] = 3  # the second row starts at an odd entry
    for i in rng.choice(np.arange(1, nrows), 3, replace=False):
        lens[i] = 2001 + 2 * int(rng.integers(0, 300))
    if int(lens.sum()) % 2 == 0:
        lens[1] += 1
    cols = []
    for i in range(nrows):
        c = rng.integers(0, ncols, lens[i])
        if lens[i] > 2:
            c[-1] = c[0]  # a duplicate
        cols.append(np.sort(c, kind="stable"))
    ci = np.concatenate(cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    va = rng.uniform(-1, 1, len(ci)).astype(dtype)
    return rp, ci, va


@pytest.mark.parametrize("kind", ["f64", "f32", "mixed"])
@pytest.mark.parametrize("shape", [(4500, 3000), (3001, 5200)])
def test_random_rectangular_native_and_fallback(ctx, kind, shape):
    nrows, ncols = shape
    rng = np.random.default_rng(nrows + ncols)
    dt = np.float32 if kind == "f32" else np.float64
    rp, ci, va = random_block(rng, nrows, ncols, dt)
    assert np.diff(rp).max() > 2000 and (np.diff(rp) == 0).any() and len(ci) % 2
    empty = np.diff(rp) == 0
    blk = hip.CsrBlock(ctx, nrows, ncols, rp, ci, va, dtype=dt)
    if kind == "mixed":
        va_used = va.astype(np.float32)
        va_ref = va_used.astype(np.float64)
        d_v = ctx.upload(va_used, np.float32)
        other = ctx.upload(va_used, np.float32)
        pointers = (d_v.ptr, other.ptr)
    else:
        va_ref = va
        other = ctx.upload(va)  # same values, not the array the plan saw
        pointers = (None, other.ptr)
    for k in KS:
        X = rng.uniform(-1, 1, (ncols, k)).astype(dt)
        Y1 = rng.uniform(-1, 1, (nrows, k)).astype(dt)
        for alpha in (1.0, -0.5):
            for beta in (0.0, 1.5):
                ref = ref_block(rp, ci, va_ref, X, alpha, beta, Y1)
                for native in (1, 0):
                    blk.set("mv_native", native)
                    assert blk.get("mv_native") == native
                    for v in pointers:
                        Y = run_m(ctx, blk, X, alpha, beta, Y1, nrows, values=v,
                                  mixed=kind == "mixed")
                        want = 1 if (native and k in (2, 4, 8) and kind != "f32") else 2
                        assert blk.get("mv_form") == want, (k, native, kind)
                        assert not np.isnan(Y).any()
                        assert same_bits(Y, ref), (kind, k, alpha, beta, native)
                    if alpha < 0 and beta == 0:  # empty rows: -0.0 exactly
                        assert (Y[empty] == 0).all() and np.signbit(Y[empty]).all()
    blk.set("mv_native", 1)
    assert blk.get("mv_kib") >= (nrows + ncols) * 16 * dt().itemsize // 1024
    other.free()
    if kind == "mixed":
        d_v.free()
    blk.free()


@pytest.mark.parametrize("kind", ["f64", "mixed"])
def test_unaligned_values_and_vectors(ctx, kind):
    """a values / colind pointer that is only element-aligned: the native kernel
    takes its element-wise path for every row block; X or Y at an 8-byte offset:
    the per-column form (its 16-byte loads and stores need the alignment)"""
    nrows, ncols = 3001, 2600
    rng = np.random.default_rng(77)
    rp, ci, va = random_block(rng, nrows, ncols, np.float64)
    vdt = np.float32 if kind == "mixed" else np.float64
    va_used = va.astype(vdt)
    va_ref = va_used.astype(np.float64)
    d_rp = ctx.upload(rp)
    d_ci = ctx.upload(np.concatenate([[0], ci]).astype(np.int32))
    d_va = ctx.upload(np.concatenate([[0], va_used]).astype(vdt), vdt)
    for k in (2, 4, 8):
        X = rng.uniform(-1, 1, (ncols, k))
        Y1 = rng.uniform(-1, 1, (nrows, k))
        d_x = ctx.upload(np.concatenate([[0.0], X.ravel()]))
        for off_ci, off_va, off_x, off_y in ((1, 1, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0),
                                            (0, 0, 1, 0), (0, 0, 0, 1)):
            d_c = ctx.upload(ci) if off_ci == 0 else None
            d_v = ctx.upload(va_used, vdt) if off_va == 0 else None
            cptr = d_c.ptr if d_c else d_ci.at(1)
            vptr = d_v.ptr if d_v else d_va.at(1)
            d_x0 = ctx.upload(X) if off_x == 0 else None
            xptr = d_x0.ptr if d_x0 else d_x.at(1)
            plan = C_plan(ctx, nrows, ncols, len(ci), d_rp.ptr, cptr)
            for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
                y0 = np.full((nrows, k), np.nan) if beta == 0 else Y1
                d_y = ctx.upload(np.concatenate([np.zeros(off_y), y0.ravel()]))
                name = ("spmv_hip_csr_spmm_f32f64" if kind == "mixed"
                        else "spmv_hip_csr_spmm_f64")
                hip.call(name, ctx.h, plan, nrows, ncols, len(ci), d_rp.ptr, cptr,
                         vptr, None, alpha, xptr, beta, d_y.at(off_y), k, None)
                ctx.synchronize()
                form = C_get(plan, "mv_form")
                assert form == (2 if off_x or off_y else 1), (k, off_ci, off_va,
                                                              off_x, off_y)
                Y = d_y.numpy()[off_y:].reshape(nrows, k)
                assert same_bits(Y, ref_block(rp, ci, va_ref, X, alpha, beta, Y1)), (
                    kind, k, off_ci, off_va, off_x, alpha, beta)
                d_y.free()
            hip.call("spmv_hip_csr_plan_destroy", plan)
            for b in (d_c, d_v, d_x0):
                if b:
                    b.free()
        d_x.free()
    for b in (d_rp, d_ci, d_va):
        b.free()


def C_plan(ctx, nrows, ncols, nnz, rowptr, colind):
    import ctypes as C
    plan = C.c_void_p()
    hip.call("spmv_hip_csr_plan_create", ctx.h, nrows, ncols, nnz, rowptr, colind, 0,
             hip.ALGO_ROWBLOCK, C.byref(plan))
    return plan


def C_get(plan, key):
    import ctypes as C
    v = C.c_int()
    hip.call("spmv_hip_csr_plan_get", plan, key.encode(), C.byref(v))
    return v.value


def _check_k4(ctx, blk, rp, ci, va, diag, tag, refs=None, released=False):
    """k = 4 through the per-column fallback (and natively where the block
    allows it) against the oracle per column"""
    nrows, ncols = blk.nrows, blk.ncols
    rng = np.random.default_rng(nrows)
    X = rng.uniform(-1, 1, (ncols, 4))
    Y1 = rng.uniform(-1, 1, (nrows, 4))
    for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
        ref = (refs[(alpha, beta)] if refs
               else ref_block(rp, ci, va, X, alpha, beta, Y1, diag))
        for native in (0, 1):
            blk.set("mv_native", native)
            Y = run_m(ctx, blk, X, alpha, beta, Y1, nrows)
            general = diag is None and not released
            assert blk.get("mv_form") == (1 if native and general else 2), tag
            assert same_bits(Y, ref), (tag, alpha, beta, native)
    blk.set("mv_native", 1)
    return X, Y1


def test_every_plan_form_poisson_64(ctx):
    n = 64
    N = n ** 3
    # AUTO plan: the lattice analysis finds constant diagonals
    blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL)
    blk.bake()
    rp, ci, va = blk.rowptr.numpy(), blk.colind.numpy(), blk.values.numpy()
    assert blk.get("sdia") == 1 or blk.get("wdia") == 1 or blk.get("lat") == 1
    _check_k4(ctx, blk, rp, ci, va, None, "auto")
    blk.free()
    # lattice analysis off: the LX form
    ctx.set_option("lat_min_nnz", 1 << 62)
    blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL)
    assert blk.get("lat") == 0 and blk.get("lx") == 1
    _check_k4(ctx, blk, rp, ci, va, None, "lx")
    blk.free()
    # csr_in_place: the caller's arrays as they are (XW / gather kernels)
    ctx.set_option("csr_in_place", 1)
    blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL)
    assert blk.get("lat") == 0 and blk.get("lx") == 0 and blk.get("sjds") == 0
    _check_k4(ctx, blk, rp, ci, va, None, "in_place")
    blk.free()
    ctx.set_option("csr_in_place", 0)
    ctx.set_option("lat_min_nnz", 1 << 20)
    # symmetric storage
    sym = hip.poisson3d_block(ctx, n, 0, N, hip.PART_LOCAL_LOWER, with_diagonal=True)
    _check_k4(ctx, sym, sym.rowptr.numpy(), sym.colind.numpy(), sym.values.numpy(),
              sym.diagonal.numpy(), "sym")
    sym.free()


def test_every_plan_form_fem_1m(ctx):
    N = 1_000_000
    rp, ci, va = poisson.fem_like_csr(N)
    blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False)
    blk.bake()
    assert blk.get("sjds") == 1
    # the references first: after the release only the plan holds the matrix
    rng = np.random.default_rng(N)
    X = rng.uniform(-1, 1, (N, 4))
    Y1 = rng.uniform(-1, 1, (N, 4))
    refs = {ab: ref_block(rp, ci, va, X, ab[0], ab[1], Y1)
            for ab in ((1.0, 0.0), (-0.5, 1.5))}
    X2, _ = _check_k4(ctx, blk, rp, ci, va, None, "sjds", refs)
    assert same_bits(X, X2)
    assert blk.owns_matrix() == 3  # no long rows: the CSR arrays can go
    assert blk.release_matrix() == 3
    _check_k4(ctx, blk, rp, ci, va, None, "released", refs, released=True)
    blk.free()
    lrp, lci, lva, dg = lower_split(rp, ci, va)
    sym = hip.CsrBlock(ctx, N, N, lrp, lci, lva, dg, True)
    sym.bake()
    _check_k4(ctx, sym, lrp, lci, lva, dg, "sym_sj")
    sym.free()


def test_released_plan_small(ctx):
    """a plan after release_csr: the fallback passes the (dangling) tokens on"""
    c = hip.Context(0)
    c.set_option("sj_min_nnz", 0)
    c.set_option("lx_min_nnz", 1 << 62)
    c.set_option("lat_min_nnz", 1 << 62)
    rp, ci, va = poisson.fem_like_csr(9000, jitter=64, layer=500)
    nr = len(rp) - 1
    blk = hip.CsrBlock(c, nr, nr, rp, ci, va, None, False)
    blk.bake()
    assert blk.get("sjds") == 1 and blk.owns_matrix() == 3
    assert blk.release_matrix() == 3
    _check_k4(c, blk, rp, ci, va, None, "released_small", released=True)
    blk.free()
    c.close()


@pytest.mark.parametrize("case", ["poisson128", "unstructured1m"])
def test_native_kernel_at_size(ctx, case):
    if case == "poisson128":
        n = 128
        N = n ** 3
        blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL, algo=hip.ALGO_ROWBLOCK)
        rp, ci, va = blk.rowptr.numpy(), blk.colind.numpy(), blk.values.numpy()
    else:
        N = 1_000_000
        rp, ci, va = poisson.unstructured_csr(N)
        blk = hip.CsrBlock(ctx, N, N, rp, ci, va, None, False)
    rng = np.random.default_rng(N)
    for k in (2, 4, 8):
        X = rng.uniform(-1, 1, (N, k))
        Y1 = rng.uniform(-1, 1, (N, k))
        for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
            for nt in (0, 1):
                blk.set("nontemporal", nt)
                Y = run_m(ctx, blk, X, alpha, beta, Y1, N)
                assert blk.get("mv_form") == 1
                assert same_bits(Y, ref_block(rp, ci, va, X, alpha, beta, Y1)), (
                    case, k, alpha, beta, nt)
    blk.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_interleave_roundtrip_and_gather_block(ctx, dtype):
    rng = np.random.default_rng(11)
    for n, k, pad in ((1, 1, 0), (127, 3, 0), (129, 4, 5), (1000, 16, 0),
                      (777, 17, 3), (5000, 40, 1), (300, 2, 0)):
        ld = n + pad
        A = rng.uniform(-1, 1, (n, k)).astype(dtype)
        d_a = ctx.upload(A)
        d_c = ctx.upload(np.full(ld * k, np.nan, dtype))
        d_b = ctx.upload(np.full(n * k, np.nan, dtype))
        hip.deinterleave(ctx, n, k, d_a.ptr, d_c.ptr, ld, dtype)
        cols = d_c.numpy().reshape(k, ld)
        assert same_bits(cols[:, :n], A.T.copy())
        assert np.isnan(cols[:, n:]).all()  # the padding is not written
        hip.interleave(ctx, n, k, d_c.ptr, d_b.ptr, ld, dtype)
        assert same_bits(d_b.numpy().reshape(n, k), A)
        idx = rng.integers(0, n, 2 * n + 1).astype(np.int32)
        d_i = ctx.upload(idx)
        d_g = ctx.upload(np.full(len(idx) * k, np.nan, dtype))
        hip.gather_block(ctx, len(idx), d_i.ptr, k, d_a.ptr, d_g.ptr, dtype)
        assert same_bits(d_g.numpy().reshape(len(idx), k), A[idx])
        for b in (d_a, d_b, d_c, d_i, d_g):
            b.free()


def test_einval_cases_raise(ctx):
    rng = np.random.default_rng(2)
    rp, ci, va = random_block(rng, 500, 400, np.float64)
    blk = hip.CsrBlock(ctx, 500, 400, rp, ci, va)
    d = ctx.upload(np.zeros(500 * 4 + 400 * 4))
    for bad in (lambda: blk.multm(1.0, d.ptr, 0.0, d.at(1600), 0),
                lambda: blk.multm(1.0, d.ptr, 0.0, d.at(1600), -3),
                lambda: blk.multm(1.0, None, 0.0, d.at(1600), 4),
                # in (400 x 4) and out (500 x 4) overlap
                lambda: blk.multm(1.0, d.ptr, 0.0, d.at(1592), 4),
                lambda: blk.multm(1.0, d.at(100), 0.0, d.ptr, 4),
                lambda: blk.set("mv_native", 2),
                lambda: hip.interleave(ctx, 10, 0, d.ptr, d.at(100)),
                lambda: hip.interleave(ctx, 10, 2, d.ptr, d.at(100), ld=9),
                lambda: hip.deinterleave(ctx, 10, 2, d.ptr, d.at(10)),
                lambda: hip.gather_block(ctx, 3, None, 2, d.ptr, d.at(100))):
        with pytest.raises(_lib.SpmvHipError) as e:
            bad()
        assert e.value.code == EINVAL
    assert blk.get("mv_form") == 0  # nothing was launched
    blk.multm(1.0, d.ptr, 0.0, d.at(1600), 4)  # adjacent, not overlapping
    ctx.synchronize()
    assert blk.get("mv_form") == 1
    d.free()
    blk.free()
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    A = host.Matrix.create_poisson3d(comm, exec_, 8, False, host.P2P_BLOCKING)
    p = exec_.alloc(8 ** 3 * 4)
    for bad in (lambda: A.mult_block(p, p, 0), lambda: A.col_map().update_block(p, 0),
                lambda: A.col_map().update_finalise_block(p, -1),
                lambda: A.mult_block(p, p, 2)):  # X and Y overlap
        with pytest.raises(host.SpmvHostError):
            bad()
    exec_.free(p)
    A.close()
    comm.close()
    exec_.close()


# ---- the host layer on one rank: mixed precision, the fp32 library type -----
def test_matrix_mult_block_mixed_and_f32():
    rng = np.random.default_rng(8)
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    N = 3000
    rp, ci, va = _sym_matrix(rng, N, 0.004)
    va = va * rng.uniform(0.5, 1.5, len(va))  # not symmetric
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [], False,
                                  host.P2P_BLOCKING)
    assert A.enable_mixed()
    va32 = va.astype(np.float32).astype(np.float64)
    for k in (2, 3):
        X = rng.uniform(-1, 1, (N, k))
        d_x, d_y = exec_.alloc(N * k), exec_.alloc(N * k)
        exec_.copy_from_host(d_x, X)
        for mixed, vals in ((False, va), (True, va32)):
            A.use_mixed(mixed)
            exec_.copy_from_host(d_y, np.full(N * k, np.nan))
            A.col_map().update_block(d_x, k)
            A.mult_block(d_x, d_y, k)
            exec_.synchronize()
            Y = exec_.copy_to_host(d_y, N * k).reshape(N, k)
            ref = np.stack([oracle.dist_spmv(1, rp, ci, vals,
                                             np.ascontiguousarray(X[:, c]), False,
                                             host.P2P_BLOCKING)
                            for c in range(k)], axis=1)
            assert same_bits(Y, ref), (k, mixed)
            assert A.plan_get("mv_form") == (1 if k == 2 else 2)
        exec_.free(d_x), exec_.free(d_y)
    A.close()
    va_f = va.astype(np.float32)
    F = host.MatrixF32(comm, exec_, rp, ci, va_f, N, N, [], [])
    X = rng.uniform(-1, 1, (N, 4)).astype(np.float32)
    d_x, d_y = exec_.alloc(N * 4, np.float32), exec_.alloc(N * 4, np.float32)
    exec_.copy_from_host(d_x, X)
    exec_.copy_from_host(d_y, np.full(N * 4, np.nan, np.float32))
    F.update_block(d_x, 4)
    F.mult_block(d_x, d_y, 4)
    exec_.synchronize()
    Y = exec_.copy_to_host(d_y, N * 4, np.float32).reshape(N, 4)
    assert same_bits(Y, ref_block(rp, ci, va_f, X, 1.0, 0.0, None))
    exec_.free(d_x), exec_.free(d_y)
    F.close()
    comm.close()
    exec_.close()


# ---- distributed: update_block -> mult_block --------------------------------
def _sym_matrix(rng, N, density=0.05, gaps=False):
    dense = rng.random((N, N)) < density
    if gaps:  # columns nobody else wants: no halo is one contiguous run
        dense[:, 3::5] = False
        dense[3::5, :] = False
    dense = dense | dense.T | np.eye(N, dtype=bool)
    vals = rng.uniform(-1, 1, (N, N))
    vals = (vals + vals.T) / 2
    rp = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)
    return rp, np.nonzero(dense)[1].astype(np.int32), vals[dense]


CMS = [host.P2P_BLOCKING, host.P2P_NONBLOCKING, host.COLLECTIVE_BLOCKING,
       host.COLLECTIVE_NONBLOCKING]


def _block_refs(world, rp, ci, va, X, ranges=None):
    """oracle.dist_spmv per column, for both storages and both kinds of model"""
    refs = {}
    for sym in (False, True):
        for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
            refs[(sym, cm)] = np.stack(
                [oracle.dist_spmv(world, rp, ci, va, np.ascontiguousarray(X[:, c]),
                                  sym, cm, ranges) for c in range(X.shape[1])], axis=1)
    return refs


def _ref_for(refs, sym, cm):
    overlap = cm in (host.P2P_NONBLOCKING, host.COLLECTIVE_NONBLOCKING)
    return refs[(sym, host.P2P_NONBLOCKING if overlap else host.P2P_BLOCKING)]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_distributed_update_block_mult_block(world):
    """an unstructured split: the halo is not one contiguous run, so the block
    pack kernel runs; all four variants of mult, k = 2 and 4"""
    from thread_world import ThreadWorld
    rng = np.random.default_rng(70 + world)
    N = 90
    rp, ci, va = _sym_matrix(rng, N, 0.15, gaps=True)
    ranges = oracle.owner_ranges(world, N)
    Xs = {k: rng.uniform(-1, 1, (N, k)) for k in (2, 4)}
    refs = {k: _block_refs(world, rp, ci, va, Xs[k]) for k in Xs}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        nloc = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        nall = nloc + len(gh)
        for sym in (False, True):
            for cm in CMS:
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, nloc, nloc,
                                              [], gh, sym, cm)
                cmap = A.col_map()
                if world > 1:
                    assert cmap.packs, "the halo must need the pack kernel"
                for k in (4, 2, 4):  # (the send buffer grows, then is reused)
                    d_x, d_y = exec_.alloc(nall * k), exec_.alloc(nloc * k)
                    exec_.memset(d_x, 0xFF, 8 * nall * k)  # NaN ghosts
                    exec_.copy_from_host(d_x, Xs[k][r0:r1])
                    exec_.copy_from_host(d_y, np.full(nloc * k, np.nan))
                    cmap.update_block(d_x, k)
                    A.mult_block(d_x, d_y, k)
                    exec_.synchronize()
                    got = exec_.copy_to_host(d_x, nall * k).reshape(nall, k)
                    assert same_bits(got[nloc:], Xs[k][gh]), (rank, sym, cm, k)
                    y = tw.gather(rank, exec_.copy_to_host(d_y, nloc * k))
                    assert same_bits(y.reshape(N, k), _ref_for(refs[k], sym, cm)), (
                        rank, sym, cm, k)
                    exec_.free(d_x), exec_.free(d_y)
                A.close()

    tw.run(rank_body, gpu=True)


@pytest.mark.parametrize("n,parts", [(10, (3, 1, 1)), (8, (1, 2, 1)), (9, (1, 1, 1))])
def test_distributed_poisson_boxes_and_slabs(n, parts):
    """Poisson on a box partition (packed sends for boxes cut along x or y) and,
    through create_poisson3d, on slabs (the contiguous-run fast path: the block
    is sent straight from the vector)"""
    from thread_world import ThreadWorld
    from util import box_partition, permute_csr
    world = parts[0] * parts[1] * parts[2]
    N = n ** 3
    rng = np.random.default_rng(n)
    k = 4
    X = rng.uniform(-1, 1, (N, k))
    perm, branges = box_partition(n, parts)
    brp, bci, bva = permute_csr(*poisson.poisson3d_csr(n), perm)
    brefs = _block_refs(world, brp, bci.astype(np.int32), bva, X, branges)
    srp, sci, sva = poisson.poisson3d_csr(n)
    sranges = oracle.owner_ranges(world, N)
    srefs = _block_refs(world, srp, sci.astype(np.int32), sva, X)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        for boxes in (True, False):
            ranges, refs = (branges, brefs) if boxes else (sranges, srefs)
            r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
            for sym in (False, True):
                for cm in (host.P2P_BLOCKING, host.COLLECTIVE_NONBLOCKING):
                    if boxes:
                        A = host.Matrix.create_poisson3d_boxes(comm, exec_, n, parts,
                                                               sym, cm)
                    else:
                        A = host.Matrix.create_poisson3d(comm, exec_, n, sym, cm)
                    cmap = A.col_map()
                    if not boxes and world > 1:
                        assert not cmap.packs
                    nloc, nall = r1 - r0, r1 - r0 + cmap.num_ghosts()
                    assert cmap.local_size() == nloc
                    d_x, d_y = exec_.alloc(nall * k), exec_.alloc(nloc * k)
                    exec_.memset(d_x, 0xFF, 8 * nall * k)
                    exec_.copy_from_host(d_x, X[r0:r1])
                    exec_.copy_from_host(d_y, np.full(nloc * k, np.nan))
                    cmap.update_block(d_x, k)
                    A.mult_block(d_x, d_y, k)
                    exec_.synchronize()
                    y = tw.gather(rank, exec_.copy_to_host(d_y, nloc * k))
                    assert same_bits(y.reshape(N, k), _ref_for(refs, sym, cm)), (
                        boxes, rank, sym, cm)
                    A.close()
                    exec_.free(d_x), exec_.free(d_y)

    tw.run(rank_body, gpu=True)


def test_onesided_map_sends_blocks_two_sided():
    """onesided_put_active: update() moves the halo by peer stores; a block of
    k > 1 vectors goes through the two-sided exchange of the same map (the peer
    windows hold one 8-byte element per ghost), and the two can alternate"""
    from thread_world import ThreadWorld
    world, n, k = 2, 12, 4
    N = n ** 3
    rp, ci, va = poisson.poisson3d_csr(n)
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (N, k))
    ranges = oracle.owner_ranges(world, N)
    refs = _block_refs(world, rp, ci.astype(np.int32), va, X)
    tw = ThreadWorld(world, timeout=60.0)

    def rank_body(rank, comm, exec_):
        import ctypes as C
        # a compute stream per rank, as ranks in processes of their own have
        stream = C.c_void_p()
        _lib.call("spmv_hip_stream_create", exec_.context, C.byref(stream))
        _lib.call("spmv_hip_set_stream", exec_.context, stream)
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        nloc = r1 - r0
        for sym in (False, True):
            A = host.Matrix.create_poisson3d(comm, exec_, n, sym,
                                             host.ONESIDED_PUT_ACTIVE)
            cmap = A.col_map()
            assert cmap.onesided() and not cmap.overlapping()
            nall = nloc + cmap.num_ghosts()
            d_x, d_y = exec_.alloc(nall * k), exec_.alloc(nloc * k)
            d_1, d_z = exec_.alloc(nall), exec_.alloc(nloc)
            exec_.memset(d_x, 0xFF, 8 * nall * k)
            exec_.copy_from_host(d_x, X[r0:r1])
            exec_.copy_from_host(d_1, np.ascontiguousarray(X[r0:r1, 0]))
            exec_.copy_from_host(d_y, np.full(nloc * k, np.nan))
            # (the symmetric block's fallback allocates its scratch at the first
            # launch: do that before anybody waits in a put kernel)
            A.mult_block(d_x, d_y, k)
            exec_.synchronize()
            tw.bar.wait()
            cmap.update(d_1)  # one-sided
            A.mult(d_1, d_z)
            cmap.update_block(d_x, k)  # two-sided, same map
            A.mult_block(d_x, d_y, k)
            cmap.update(d_1)
            exec_.synchronize()
            y = tw.gather(rank, exec_.copy_to_host(d_y, nloc * k))
            assert same_bits(y.reshape(N, k), refs[(sym, host.P2P_BLOCKING)]), sym
            z = tw.gather(rank, exec_.copy_to_host(d_z, nloc))
            assert same_bits(z, refs[(sym, host.P2P_BLOCKING)][:, 0]), sym
            tw.bar.wait()  # nobody closes while a neighbour still exchanges
            A.close()
            for p in (d_x, d_y, d_1, d_z):
                exec_.free(p)
        _lib.call("spmv_hip_set_stream", exec_.context, None)
        _lib.call("spmv_hip_stream_destroy", exec_.context, stream)

    tw.run(rank_body, gpu=True)
