"""A plan gives back the device memory it took: every plan form is created,
baked, run once against the oracle and destroyed, three times over, and the
device's free memory after the third round equals that after the first.

The shapes are those of test_gpu_multivec.test_every_plan_form_*, so that every
plan-building file's builder and its free function run: the lattice / diagonal
forms, LX, XW, symmetric storage (as created, and with the lattice analysis
let in: its stored block is below lat_min_nnz), the sliced jagged form with its long-row
list, the merged symmetric form, a multi-vector plan and the multicolour
Gauss-Seidel preconditioner.

The bound is equality.  Measured on an MI355X with the builders as they were
before they got owned scratch (plan_scratch.h) and as they are now: the free
memory after each of the three rounds is the same figure in both, a drift of
0 bytes per round.  The readings are printed before the assertion."""
import numpy as np
import pytest

import oracle
from spmv_amd import _lib, hip, host, poisson
from util import lower_split

pytestmark = pytest.mark.gpu

N64 = 64
FEM_ROWS = 1_000_000
ENOTSUP = -3  # no form holds the values by offset: what an LX or XW plan's bake returns


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.synchronize()
    c.close()


@pytest.fixture(scope="module")
def problems():
    """the matrices and the oracle's products, computed once"""
    N = N64 ** 3
    rp, ci, va = poisson.poisson3d_csr(N64)
    ci = ci.astype(np.int32)
    x = oracle.gaussian_x_fast(N)
    p = {"x64": x, "y64": oracle.csr_spmv(rp, ci, va, x),
         "y64_sym": oracle.csr_spmv_sym(*oracle.poisson3d_lower(N64), x)}
    X = np.random.default_rng(N).uniform(-1, 1, (N, 4))
    p["X64"] = X
    p["Y64"] = np.stack([oracle.csr_spmv(rp, ci, va, np.ascontiguousarray(X[:, c]))
                         for c in range(4)], axis=1)
    frp, fci, fva = poisson.fem_like_csr(FEM_ROWS)
    xf = oracle.gaussian_x_fast(FEM_ROWS)
    p["fem"] = (frp, fci, fva)
    p["fem_sym"] = lower_split(frp, fci, fva)
    p["xf"] = xf
    p["yf"] = oracle.csr_spmv(frp, fci, fva, xf)
    p["yf_sym"] = oracle.csr_spmv_sym(*p["fem_sym"], xf)
    return p


def _bake_csr_order(blk):
    """plan_bake_values of a plan whose kernels read the caller's arrays: the
    bake runs (and may make the LX form's narrowed copy) and says ENOTSUP"""
    rc = _lib.hip.spmv_hip_csr_plan_bake_values_f64(
        blk.ctx.h, blk.plan, blk.values.ptr,
        None if blk.diagonal is None else blk.diagonal.ptr, None)
    assert rc in (0, ENOTSUP), rc


def _spmv_once(ctx, blk, x, ref, tag):
    d_x = ctx.upload(x)
    d_y = ctx.upload(np.full(blk.nrows, np.nan))
    blk.mult(1.0, d_x.ptr, 0.0, d_y.ptr)
    ctx.synchronize()
    y = d_y.numpy()
    d_x.free(), d_y.free()
    assert np.array_equal(y, ref), tag


def _one_round(ctx, exec_, comm, p):
    N = N64 ** 3
    # general storage: the lattice / diagonal forms, then one multi-vector product
    blk = hip.poisson3d_block(ctx, N64, 0, N, hip.PART_ALL)
    blk.bake()
    assert blk.get("sdia") == 1 or blk.get("wdia") == 1 or blk.get("lat") == 1
    _spmv_once(ctx, blk, p["x64"], p["y64"], "auto")
    d_x, d_y = ctx.upload(p["X64"]), ctx.upload(np.full((N, 4), np.nan))
    blk.multm(1.0, d_x.ptr, 0.0, d_y.ptr, 4)
    ctx.synchronize()
    Y = d_y.numpy().reshape(N, 4)
    d_x.free(), d_y.free()
    assert np.array_equal(Y, p["Y64"]), "mult_block"
    blk.free()
    # lattice analysis off: LX
    ctx.set_option("lat_min_nnz", 1 << 62)
    try:
        blk = hip.poisson3d_block(ctx, N64, 0, N, hip.PART_ALL)
        _bake_csr_order(blk)
        assert blk.get("lat") == 0 and blk.get("lx") == 1
        _spmv_once(ctx, blk, p["x64"], p["y64"], "lx")
        blk.free()
        # the caller's arrays as they are: XW
        ctx.set_option("csr_in_place", 1)
        blk = hip.poisson3d_block(ctx, N64, 0, N, hip.PART_ALL)
        _bake_csr_order(blk)
        assert blk.get("lat") == 0 and blk.get("lx") == 0 and blk.get("sjds") == 0
        _spmv_once(ctx, blk, p["x64"], p["y64"], "in_place")
        blk.free()
    finally:
        ctx.set_option("csr_in_place", 0)
        ctx.set_option("lat_min_nnz", 1 << 20)
    # symmetric storage: with the default options (its 0.79 M stored entries
    # are below lat_min_nnz: the transposed-map kernel, no form to bake into),
    # then with the lattice analysis on (the symmetric lattice / diagonal forms)
    sym = hip.poisson3d_block(ctx, N64, 0, N, hip.PART_LOCAL_LOWER, with_diagonal=True)
    _bake_csr_order(sym)
    _spmv_once(ctx, sym, p["x64"], p["y64_sym"], "sym")
    sym.free()
    ctx.set_option("lat_min_nnz", 0)
    try:
        sym = hip.poisson3d_block(ctx, N64, 0, N, hip.PART_LOCAL_LOWER,
                                  with_diagonal=True)
        sym.bake()
        assert sym.get("sdia") == 1
        _spmv_once(ctx, sym, p["x64"], p["y64_sym"], "sym_lattice")
        sym.free()
    finally:
        ctx.set_option("lat_min_nnz", 1 << 20)
    # no lattice: the sliced jagged form, the merged symmetric form
    frp, fci, fva = p["fem"]
    blk = hip.CsrBlock(ctx, FEM_ROWS, FEM_ROWS, frp, fci, fva, None, False)
    blk.bake()
    assert blk.get("sjds") == 1
    _spmv_once(ctx, blk, p["xf"], p["yf"], "sjds")
    blk.free()
    lrp, lci, lva, dg = p["fem_sym"]
    sym = hip.CsrBlock(ctx, FEM_ROWS, FEM_ROWS, lrp, lci, lva, dg, True)
    sym.bake()
    _spmv_once(ctx, sym, p["xf"], p["yf_sym"], "sym_sj")
    sym.free()
    # the multicolour Gauss-Seidel preconditioner of the 64^3 matrix
    A = host.Matrix.create_poisson3d(comm, exec_, N64, False, host.P2P_NONBLOCKING)
    M = host.SgsPreconditioner(exec_, A)
    assert M.rows() == N and M.num_colors() >= 2
    M.close()
    A.close()
    ctx.synchronize()


def test_plan_cycles_return_their_memory(ctx, problems):
    import torch

    exec_ = host.HipExecutor(0)
    comm = host.Comm.self_comm()
    free = []
    torch.cuda.init()  # (its own context's memory is taken before the first reading)
    try:
        for _ in range(3):
            _one_round(ctx, exec_, comm, problems)
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
    finally:
        comm.close()
        exec_.close()
    print("free bytes after each round:", free,
          "drift per round:", [free[i + 1] - free[i] for i in range(2)])
    assert free[2] == free[0], free
