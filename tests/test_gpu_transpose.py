"""GPU tests of the transposed product (Matrix::transpmult): every form of the
kernel layer (copy + inner plan, in place, self-transpose) bit for bit against
the row-order CSR sum of the STABLE transpose, and the distributed
transpmult -> reverse_update sequence of demos/restrictmain.cpp."""
import numpy as np
import pytest

import oracle
from spmv_amd import _lib, hip, host, poisson

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.synchronize()
    c.close()


def stable_transpose(rp, ci, va, ncols):
    """CSR of A^T: entries sorted by column, ties in CSR order."""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp))
    order = np.argsort(np.asarray(ci), kind="stable")
    tp = np.zeros(ncols + 1, np.int64)
    np.add.at(tp, np.asarray(ci, np.int64) + 1, 1)
    return np.cumsum(tp).astype(np.int32), rows[order], np.asarray(va)[order]


def ref_t(rp, ci, va, ncols, x, alpha, beta, y0, c0=0, c1=None):
    """out[j - c0] = alpha s_j + beta y0[j - c0] (beta == 0: y0 never read)"""
    c1 = ncols if c1 is None else c1
    tp, tr, tv = stable_transpose(rp, ci, va, ncols)
    dt = np.asarray(va).dtype
    s = oracle.csr_spmv(tp, tr, tv.astype(dt), np.asarray(x, dt))[c0:c1]
    if beta == 0:
        return (dt.type(alpha) * s).astype(dt)
    return oracle.csr_spmv(tp[c0:c1 + 1] - tp[c0], tr[tp[c0]:tp[c1]],
                           tv[tp[c0]:tp[c1]].astype(dt), np.asarray(x, dt),
                           alpha, beta, np.asarray(y0, dt))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def random_block(rng, nrows, ncols, dtype):
    """empty rows and columns, duplicates, and a few columns of > 2000 entries"""
    lens = rng.integers(0, 9, nrows)
    lens[rng.random(nrows) < 0.1] = 0
    cols = []
    hot = rng.integers(0, ncols, 2)
    for i in range(nrows):
        c = rng.integers(0, ncols // 2, lens[i]) * 2  # odd columns stay empty
        c = np.concatenate([c, hot])                  # > 2000 entries each
        if lens[i] > 2:
            c = np.concatenate([c, c[:1]])            # a duplicate
        cols.append(np.sort(c, kind="stable"))
    ci = np.concatenate(cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    va = rng.uniform(-1, 1, len(ci)).astype(dtype)
    return rp, ci, va


def run_t(ctx, blk, x, alpha, beta, ncols_out, dtype, values=None, fill=None):
    d_x = ctx.upload(x.astype(dtype))
    y0 = (np.full(ncols_out, np.nan, dtype) if fill is None
          else np.asarray(fill, dtype))
    d_y = ctx.upload(y0)
    blk.multt(alpha, d_x.ptr, beta, d_y.ptr, values=values)
    ctx.synchronize()
    y = d_y.numpy()
    d_x.free(), d_y.free()
    return y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(4500, 3000), (3000, 5200)])
def test_random_rectangular_every_form(ctx, dtype, shape):
    nrows, ncols = shape
    rng = np.random.default_rng(nrows + ncols)
    rp, ci, va = random_block(rng, nrows, ncols, dtype)
    assert np.diff(stable_transpose(rp, ci, va, ncols)[0]).max() > 2000
    x = rng.uniform(-1, 1, nrows).astype(dtype)
    y1 = rng.uniform(-1, 1, ncols).astype(dtype)
    for in_place_opt in (0, 1):
        ctx.set_option("csr_in_place", in_place_opt)
        blk = hip.CsrBlock(ctx, nrows, ncols, rp, ci, va, dtype=dtype)
        blk.transpose()
        assert blk.get("t_form") == (2 if in_place_opt else 1)
        other = ctx.upload(va)  # same values, another pointer: in place
        for force in (0, 1):
            blk.set("t_in_place", force)
            assert blk.get("t_form") == (2 if force or in_place_opt else 1)
            for alpha in (1.0, -0.5):
                for beta in (0.0, 1.5):
                    fill = None if beta == 0 else y1
                    ref = ref_t(rp, ci, va, ncols, x, alpha, beta, y1)
                    for v in (None, other.ptr):
                        y = run_t(ctx, blk, x, alpha, beta, ncols, dtype, v, fill)
                        assert not np.isnan(y).any()
                        assert same_bits(y, ref), (in_place_opt, force, alpha, beta)
                    if alpha < 0 and beta == 0:  # empty columns: -0.0 exactly
                        assert np.signbit(y[1::2][ref[1::2] == 0]).all()
        blk.set("t_in_place", 0)
        assert blk.get("t_kib") > 0 and blk.get("t_plan_us") > 0
        other.free()
        blk.free()
    ctx.set_option("csr_in_place", 0)


def test_column_subrange_leaves_the_rest(ctx):
    rng = np.random.default_rng(5)
    nrows, ncols = 2000, 3000
    rp, ci, va = random_block(rng, nrows, ncols, np.float64)
    keep = (ci >= 1000) & (ci < 2500)
    rows = np.repeat(np.arange(nrows), np.diff(rp))[keep]
    ci2, va2 = ci[keep], va[keep]
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))])
    rp2 = rp2.astype(np.int32)
    x = rng.uniform(-1, 1, nrows)
    blk = hip.CsrBlock(ctx, nrows, ncols, rp2, ci2, va2)
    blk.transpose(1000, 2500)
    fill = rng.uniform(-1, 1, ncols)
    d_x, d_y = ctx.upload(x), ctx.upload(fill)
    blk.multt(-0.5, d_x.ptr, 0.0, d_y.at(1000))
    y = d_y.numpy()
    ref = ref_t(rp2, ci2, va2, ncols, x, -0.5, 0.0, None, 1000, 2500)
    assert same_bits(y[1000:2500], ref)
    assert same_bits(y[:1000], fill[:1000]) and same_bits(y[2500:], fill[2500:])
    # an entry outside the range is refused
    with pytest.raises(_lib.SpmvHipError) as e:
        blk.transpose(1000, 2000)
    assert e.value.code == EINVAL
    assert blk.get("t_form") == 0
    d_x.free(), d_y.free()
    blk.free()


def test_einval_after_release_and_symmetric(ctx):
    N = 16 ** 3
    ctx.set_option("lat_min_nnz", 0)
    blk2 = hip.poisson3d_block(ctx, 16, 0, N, hip.PART_ALL)
    ctx.set_option("lat_min_nnz", 1 << 20)
    blk2.bake()
    assert blk2.release_matrix() == 3
    with pytest.raises(_lib.SpmvHipError) as e:
        blk2.transpose()
    assert e.value.code == EINVAL
    sym = hip.poisson3d_block(ctx, 16, 0, N, hip.PART_LOCAL_LOWER, with_diagonal=True)
    with pytest.raises(_lib.SpmvHipError) as e:
        sym.transpose()
    assert e.value.code == EINVAL
    for b in (blk2, sym):
        b.free()


@pytest.mark.parametrize("skew", [0, 300000])
def test_poisson_64_self_and_skewed(ctx, skew):
    n = 64
    N = n ** 3
    ctx.set_option("poisson_skew_ppm", skew)
    blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL)
    ctx.set_option("poisson_skew_ppm", 0)
    blk.bake()
    rp, ci, va = blk.rowptr.numpy(), blk.colind.numpy(), blk.values.numpy()
    blk.transpose()
    # symmetric: its own transpose; skewed: the copy, whose transpose has
    # constant diagonals again
    assert blk.get("t_form") == (3 if skew == 0 else 1)
    if skew:
        assert blk.get("t.sdia_const") == 1 or blk.get("t.wdia_const") == 1
    x = oracle.gaussian_x_fast(N)
    y1 = np.linspace(-1, 1, N)
    for force in (0, 1):
        blk.set("t_in_place", force)
        for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
            y = run_t(ctx, blk, x, alpha, beta, N, np.float64,
                      fill=None if beta == 0 else y1)
            assert same_bits(y, ref_t(rp, ci, va, N, x, alpha, beta, y1))
    blk.set("t_in_place", 0)
    blk.free()


def test_values_changed_self_to_general(ctx):
    """a self-transposed block rewritten in place into a non-symmetric one:
    values_changed demotes it to the in-place kernel; a copy refreshes"""
    n = 24
    N = n ** 3
    for skew in (0, 200000):
        ctx.set_option("poisson_skew_ppm", skew)
        blk = hip.poisson3d_block(ctx, n, 0, N, hip.PART_ALL)
        ctx.set_option("poisson_skew_ppm", 0)
        rp, ci, va = blk.rowptr.numpy(), blk.colind.numpy(), blk.values.numpy()
        blk.transpose()
        assert blk.get("t_form") == (3 if skew == 0 else 1)
        rng = np.random.default_rng(7)
        va2 = va * rng.uniform(0.5, 1.5, len(va))
        blk.values.write(va2)
        blk.values_changed()
        assert blk.get("t_form") == 2 if skew == 0 else blk.get("t_form") == 1
        x = rng.uniform(-1, 1, N)
        y = run_t(ctx, blk, x, -1.0, 0.0, N, np.float64)
        assert same_bits(y, ref_t(rp, ci, va2, N, x, -1.0, 0.0, None))
        # and back: symmetric values again -> the self form
        blk.values.write(va if skew == 0 else va2)
        blk.values_changed()
        if skew == 0:
            assert blk.get("t_form") == 3
        blk.free()


@pytest.mark.parametrize("kind", ["unstructured", "fem"])
def test_large_generated_matrices(ctx, kind):
    nrows = 1 << 20
    if kind == "unstructured":
        rp, ci, va = poisson.unstructured_csr(nrows)
    else:
        rp, ci, va = poisson.fem_like_csr(nrows)
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    blk = hip.CsrBlock(ctx, nrows, nrows, rp, ci, va)
    blk.bake()
    blk.transpose()
    assert blk.get("t_form") in (1, 3)
    x = oracle.gaussian_x_fast(nrows)
    ref = ref_t(rp, ci, va, nrows, x, 1.0, 0.0, None)
    for force in (0, 1):
        blk.set("t_in_place", force)
        assert same_bits(run_t(ctx, blk, x, 1.0, 0.0, nrows, np.float64), ref)
    blk.free()


# ---- distributed: transpmult -> reverse_update ------------------------------
def _localise(rp, ci, va, r0, r1, c0, c1):
    """rows [r0, r1), owned columns [c0, c1) -> local CSR + ghosts"""
    a, b = int(rp[r0]), int(rp[r1])
    g = np.asarray(ci[a:b], np.int64)
    ghost = (g < c0) | (g >= c1)
    ghosts = np.unique(g[ghost])
    lc = np.where(ghost, (c1 - c0) + np.searchsorted(ghosts, g), g - c0)
    return ((rp[r0:r1 + 1] - rp[r0]).astype(np.int32), lc.astype(np.int32),
            np.asarray(va[a:b]).copy(), ghosts)


def _sym_lower(lrp, lci, lva, nloc, r0):
    """the stored local block of symmetric storage: strictly lower, diagonal"""
    rows = np.repeat(np.arange(nloc), np.diff(lrp))
    own = lci < nloc
    lower = own & (lci < rows)
    diag = np.zeros(nloc)
    np.add.at(diag, rows[own & (lci == rows)], lva[own & (lci == rows)])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[lower], minlength=nloc))])
    return rp.astype(np.int32), lci[lower], lva[lower], diag


def _sym_matrix(rng, N, density=0.05):
    dense = rng.random((N, N)) < density
    dense = dense | dense.T | np.eye(N, dtype=bool)
    vals = rng.uniform(-1, 1, (N, N))
    vals = (vals + vals.T) / 2
    rp = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)
    return rp, np.nonzero(dense)[1].astype(np.int32), vals[dense]


CMS = [host.P2P_BLOCKING, host.P2P_NONBLOCKING, host.COLLECTIVE_BLOCKING,
       host.COLLECTIVE_NONBLOCKING]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_distributed_transpmult_reverse_update(world):
    from thread_world import ThreadWorld
    rng = np.random.default_rng(40 + world)
    N = 90
    rp, ci, va = _sym_matrix(rng, N)
    # a non-symmetric twin with the same pattern (general storage only)
    va_g = va * rng.uniform(0.5, 1.5, len(va))
    b = rng.uniform(-1, 1, N)
    ranges = oracle.owner_ranges(world, N)
    sizes = np.diff(ranges)
    locs = {}
    for r in range(world):
        r0, r1 = int(ranges[r]), int(ranges[r + 1])
        locs[r] = (_localise(rp, ci, va, r0, r1, r0, r1),
                   _localise(rp, ci, va_g, r0, r1, r0, r1))
    plans = oracle.l2g_plans(sizes, [locs[r][0][3] for r in range(world)])
    refs = {}
    for sym in (False, True):
        tails = []
        for r in range(world):
            r0, r1 = int(ranges[r]), int(ranges[r + 1])
            lrp, lci, lva, gh = locs[r][0] if sym else locs[r][1]
            nloc, nall = r1 - r0, r1 - r0 + len(gh)
            t = ref_t(lrp, lci, lva, nall, b[r0:r1], 1.0, 0.0, None)
            if sym:  # the stored block's forward symmetric product
                lo = _sym_lower(lrp, lci, lva, nloc, r0)
                t[:nloc] = oracle.csr_spmv_sym(lo[0], lo[1], lo[2], lo[3], b[r0:r1])
                rem = lci >= nloc
                rows = np.repeat(np.arange(nloc), np.diff(lrp))
                rrp = np.concatenate([[0], np.cumsum(
                    np.bincount(rows[rem], minlength=nloc))]).astype(np.int32)
                t[nloc:] = ref_t(rrp, lci[rem], lva[rem], nall, b[r0:r1], 1.0, 0.0,
                                 None, nloc, nall)
            tails.append(t)
        refs[sym] = (tails, oracle.l2g_reverse_update(plans, [t.copy() for t in tails]))
    # the adjoint identity on the general matrix: <A x, b> = <x, A^T b>
    x = rng.uniform(-1, 1, N)
    Ax = oracle.csr_spmv(rp, ci, va_g, x)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        nloc = r1 - r0
        for sym in (False, True):
            lrp, lci, lva, gh = locs[rank][0] if sym else locs[rank][1]
            nall = nloc + len(gh)
            for cm in CMS:
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, nloc, nloc,
                                              [], gh, sym, cm)
                d_b, d_y = exec_.alloc(nloc), exec_.alloc(max(nall, 1))
                exec_.copy_from_host(d_b, b[r0:r1])
                exec_.copy_from_host(d_y, np.full(nall, np.nan))
                A.transpmult(d_b, d_y)
                exec_.synchronize()
                y = exec_.copy_to_host(d_y, nall)
                assert same_bits(y, refs[sym][0][rank]), (rank, sym, cm)
                m = host.L2GMap(comm, nloc, gh, exec_, host.P2P_BLOCKING)
                m.reverse_update(d_y)
                exec_.synchronize()
                y = exec_.copy_to_host(d_y, nall)
                assert same_bits(y[:nloc], refs[sym][1][rank][:nloc]), (rank, sym, cm)
                if not sym:
                    aTb = tw.gather(rank, y[:nloc])
                    lhs, rhs = np.dot(Ax, b), np.dot(x, aTb)
                    bound = 1e-13 * (np.abs(va_g).sum() * np.abs(x).max()
                                     * np.abs(b).max())
                    assert abs(lhs - rhs) <= bound, (lhs, rhs)
                m.close()
                A.close()
                exec_.free(d_b), exec_.free(d_y)

    tw.run(rank_body, gpu=True)


@pytest.mark.parametrize("world", [2, 3])
def test_restriction_sequence(world):
    """restrictmain: psp = R^T q; reverse_update(psp); update(psp); R psp"""
    from thread_world import ThreadWorld
    M = 60
    rows, cols, vals = [], [], []
    for i in range(M):
        for c, w in ((2 * i - 1, 0.25), (2 * i, 0.5), (2 * i + 1, 0.25)):
            if 0 <= c < 2 * M:
                rows.append(i), cols.append(c), vals.append(w)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))]).astype(np.int32)
    ci, va = np.array(cols, np.int32), np.array(vals)
    rng = np.random.default_rng(9)
    q = rng.uniform(-1, 1, M)
    rr = oracle.owner_ranges(world, M)
    cr = 2 * rr
    locs = [_localise(rp, ci, va, int(rr[r]), int(rr[r + 1]), int(cr[r]),
                      int(cr[r + 1])) for r in range(world)]
    plans = oracle.l2g_plans(np.diff(cr), [l[3] for l in locs])
    tails = [ref_t(l[0], l[1], l[2], int(cr[r + 1] - cr[r]) + len(l[3]),
                   q[rr[r]:rr[r + 1]], 1.0, 0.0, None) for r, l in enumerate(locs)]
    rev = oracle.l2g_reverse_update(plans, [t.copy() for t in tails])
    psp_ref = np.concatenate([rev[r][:int(cr[r + 1] - cr[r])] for r in range(world)])
    # the owners' shares make up the global R^T q
    assert np.allclose(psp_ref, oracle.csr_spmv(*stable_transpose(rp, ci, va, 2 * M),
                                                q), rtol=1e-14, atol=0)
    out_ref = oracle.csr_spmv(rp, ci, va, psp_ref)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        lrp, lci, lva, gh = locs[rank]
        nr, nc = int(rr[rank + 1] - rr[rank]), int(cr[rank + 1] - cr[rank])
        for cm in CMS:
            R = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, nr, nc, [], gh,
                                          False, cm)
            cmap = R.col_map()
            assert cmap.local_size() == nc and cmap.num_ghosts() == len(gh)
            d_q, d_p, d_o = exec_.alloc(nr), exec_.alloc(nc + len(gh)), exec_.alloc(nr)
            exec_.copy_from_host(d_q, q[rr[rank]:rr[rank + 1]])
            R.transpmult(d_q, d_p)
            m = host.L2GMap(comm, nc, gh, exec_, host.P2P_BLOCKING)
            m.reverse_update(d_p)
            exec_.synchronize()
            p = exec_.copy_to_host(d_p, nc)
            assert same_bits(p, rev[rank][:nc]), (rank, cm)
            cmap.update(d_p)
            R.mult(d_p, d_o)
            exec_.synchronize()
            o = tw.gather(rank, exec_.copy_to_host(d_o, nr))
            assert np.allclose(o, out_ref, rtol=1e-14, atol=0)
            m.close()
            R.close()
            exec_.free(d_q), exec_.free(d_p), exec_.free(d_o)

    tw.run(rank_body, gpu=True)


def test_matrix_f32_transpmult_and_release():
    rng = np.random.default_rng(3)
    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    N = 500
    rp, ci, va = _sym_matrix(rng, N)
    va = (va * rng.uniform(0.5, 1.5, len(va)))
    b = rng.uniform(-1, 1, N)
    A = host.MatrixF32(comm, exec_, rp, ci, va, N, N, [], [])
    d_b, d_y = exec_.alloc(N, np.float32), exec_.alloc(N, np.float32)
    exec_.copy_from_host(d_b, b.astype(np.float32))
    A.transpmult(d_b, d_y)
    y = exec_.copy_to_host(d_y, N, np.float32)
    assert same_bits(y, ref_t(rp, ci, va.astype(np.float32), N, b, 1.0, 0.0, None))
    A.close()
    # release_csr without a map built before: a clear error; with one (the
    # symmetric Poisson matrix is its own transpose): mult's bits
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"lat_min_nnz", 0)
    n = 16
    N3 = n ** 3
    d_x, d_z, d_w = exec_.alloc(N3), exec_.alloc(N3), exec_.alloc(N3)
    exec_.copy_from_host(d_x, oracle.gaussian_x_fast(N3))
    for eager in (False, True):
        P = host.Matrix.create_poisson3d(comm, exec_, n, False, host.P2P_BLOCKING)
        if eager:
            P.enable_transpose()
            assert P.plan_get("t_form") == 3
        assert P.release_csr() > 0
        if eager:
            P.transpmult(d_x, d_z)
            P.mult(d_x, d_w)
            exec_.synchronize()
            assert same_bits(exec_.copy_to_host(d_z, N3), exec_.copy_to_host(d_w, N3))
        else:
            with pytest.raises(host.SpmvHostError, match="enable_transpose"):
                P.transpmult(d_x, d_z)
        P.close()
    for p in (d_x, d_z, d_w, d_b, d_y):
        exec_.free(p)
    comm.close()
    exec_.close()
