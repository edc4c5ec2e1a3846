"""The block sweeps alone: mcgs_sweep_block_kernel (hip/spmv_mcgs.hip) through
spmv_hip_mcgs_apply_block_f64 on the hand-coloured cases of sgs_kernel_cases.py,
and spmv::sgs_apply_block through SgsPreconditioner / Ilu0Preconditioner objects.

The contract is bit-exactness: column c of Z = M^-1 R has the bits of the
single-vector sweep on column c.  Nothing here has a tolerance.

  C ABI     every sweep case (slice edges, the 64-entry chunk edge, a colour of
            one row, the padding slot that would show 0 * Inf) with the recipes
            benign, poison, negzero, overflow_before, overflow_after and
            subnormal as the plan's values; nrhs = 1, 2, 3, 4, 8; the columns
            of a block carry DIFFERENT recipes' r and prefill of z, so a lane
            that mixed two columns up would show.  Compared as bits, NaN
            matching NaN, against the numpy sweep (Ilu0Ref.apply on the
            matrix's own values) per column; R and Z between guard words, 16-
            byte aligned and 8 bytes off; R is read back unchanged.
  objects   Poisson 11^3 and 24^3, banded4097 and ragged3001 (two rows of
            about 500 entries, 24+ colours, single-row colours), both
            storages, SGS and ILU(0): column c equals sgs_apply on column c on
            the GPU and the numpy restatement, np.array_equal, for every
            combination of aligned / 8 bytes off of R and Z; nrhs outside 1..8
            and overlapping blocks are refused and write nothing."""
import ctypes as C

import numpy as np
import pytest

import ilu0_cases as ic
import oracle
import sgs_kernel_cases as kc
import sgs_layout as sl
import special_values as sv
import test_gpu_pcg as tp
import test_gpu_sgs as ts
from spmv_amd import hip, host
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)
from test_gpu_sgs_kernels import _same

pytestmark = pytest.mark.gpu

G = 16  # guard doubles on either side of R and Z
GUARD = -7.25e77
NRHS = (1, 2, 3, 4, 8)
RECIPES = ("benign", "poison", "negzero", "overflow_before", "overflow_after",
           "subnormal")
SENTINEL = tp.SENTINEL


# ---- 1. through the C ABI on the hand-coloured cases ----------------------------------
def _combos():
    return [pytest.param(name, rname, id=f"{name}-{rname}")
            for name, case in kc.cases().items()
            for rname in RECIPES if case.recipes()[rname].sweep]


@pytest.mark.parametrize("name,rname", _combos())
def test_block_sweep_through_the_abi(ctx, name, rname):
    case = kc.cases()[name]
    recs = case.recipes()
    rec = recs[rname]
    l, u, d = fac = case.parts_values(rec.va)
    with np.errstate(all="ignore"):
        dinv = 1.0 / case.diag_of(rec.va)
    struct, keep = sl.mcgs_host(sl.with_values(case.lay, l, u), dinv)
    plan = C.c_void_p()
    hip.call("spmv_hip_mcgs_plan_create", ctx.h,
             C.cast(C.pointer(struct), C.c_void_p), C.byref(plan))
    n = case.n
    # column c carries the r and the prefill of recipe order[c % 6]: the plan's
    # own recipe first, then the others
    order = [rname] + [r for r in RECIPES if r != rname]
    want = {r: case.apply(fac, recs[r].r) for r in order}
    size = n * max(NRHS) + 2 * G + 1
    d_r, d_z = ctx.empty(size, np.float64), ctx.empty(size, np.float64)
    try:
        for nrhs in NRHS:
            names = [order[c % len(order)] for c in range(nrhs)]
            R = np.stack([np.asarray(recs[r].r, np.float64) for r in names], 1)
            Z0 = np.stack([np.asarray(recs[r].z0, np.float64) for r in names], 1)
            for off in (0, 1):
                lo, hi = G + off, G + off + n * nrhs
                for buf, data in ((d_r, R), (d_z, Z0)):
                    img = np.full(size, GUARD)
                    img[lo:hi] = data.reshape(-1)
                    buf.write(img)
                hip.call("spmv_hip_mcgs_apply_block_f64", ctx.h, plan, None,
                         d_r.at(lo), d_z.at(lo), nrhs, None)
                ctx.stream_sync()
                r_back, z_back = d_r.numpy(), d_z.numpy()
                what = (name, rname, nrhs, off)
                for img, v in ((r_back, "R"), (z_back, "Z")):
                    assert np.all(img[:lo] == GUARD), (what, v, "guard in front")
                    assert np.all(img[hi:] == GUARD), (what, v, "guard behind")
                assert sv.same_bits(r_back[lo:hi], R.reshape(-1)), what
                Z = z_back[lo:hi].reshape(n, nrhs)
                for c, r in enumerate(names):
                    _same(np.ascontiguousarray(Z[:, c]), want[r], what + (c, r))
    finally:
        ctx.stream_sync()
        d_r.free()
        d_z.free()
        hip.call("spmv_hip_mcgs_plan_destroy", plan)


# ---- 2. through the objects ----------------------------------------------------------------
NAMES = ("poisson11", "poisson24", "banded4097", "ragged3001")
OFFSETS = ((0, 0), (1, 1), (0, 1), (1, 0))  # doubles off 16-byte alignment: R, Z


class _Problem:
    """One matrix in both storages with SGS and ILU(0) objects, their numpy
    restatements and eight right-hand sides."""

    def __init__(self, exec_, comm, name):  # noqa: F811
        self.name, self.exec_ = name, exec_
        self.csr = ts._make_csr(name)
        self.N = N = len(self.csr[0]) - 1
        dinv = 1.0 / tp._diag_of(self.csr)
        rng = np.random.default_rng(N + 2)
        self.R = np.stack([oracle.csr_spmv(*self.csr, rng.uniform(-1, 1, N))
                           for _ in range(8)], axis=1)
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.M, self.numpy_apply = {}, {}
        for sym, A in self.A.items():
            sgs = host.SgsPreconditioner(exec_, A)
            ilu = host.Ilu0Preconditioner(exec_, A)
            colours = sgs.colors()
            assert np.array_equal(ilu.colors(), colours)
            sweeps = ts.Sweeps(self.csr, N, colours, sym)
            ref = ic.Ilu0Ref(self.csr, N, colours, False)
            fac = ref.factor()
            self.M[("sgs", sym)], self.M[("ilu0", sym)] = sgs, ilu
            self.numpy_apply[("sgs", sym)] = (
                lambda r, s=sweeps: s.apply(dinv, r))
            self.numpy_apply[("ilu0", sym)] = (
                lambda r, ref=ref, fac=fac: ref.apply(fac, r))
        self.d_r = exec_.alloc(N * 8 + 2)
        self.d_z = exec_.alloc(N * 8 + 2 * G + 2)
        self.d_r1, self.d_z1 = exec_.alloc(N), exec_.alloc(N)

    def single(self, M, r):
        """sgs_apply on one vector, on the GPU"""
        e = self.exec_
        e.copy_from_host(self.d_r1, r)
        e.copy_from_host(self.d_z1, np.full(self.N, SENTINEL))
        host.sgs_apply(e, M, self.d_r1, self.d_z1)
        return e.copy_to_host(self.d_z1, self.N)

    def block(self, M, nrhs, r_off, z_off):
        """sgs_apply_block on the first nrhs columns -> Z[N, nrhs]; guards
        checked"""
        e, N = self.exec_, self.N
        R = np.ascontiguousarray(self.R[:, :nrhs])
        e.copy_from_host(self.d_r + 8 * r_off, R)
        e.copy_from_host(self.d_z, np.full(N * 8 + 2 * G + 2, SENTINEL))
        lo = G + z_off
        host.sgs_apply_block(e, M, self.d_r + 8 * r_off, self.d_z + 8 * lo, nrhs)
        buf = e.copy_to_host(self.d_z, N * 8 + 2 * G + 2)
        assert np.all(buf[:lo] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[lo + N * nrhs:] == SENTINEL), (self.name, "guard behind")
        back = e.copy_to_host(self.d_r + 8 * r_off, N * nrhs)
        assert np.array_equal(back, R.reshape(-1)), (self.name, "R changed")
        return buf[lo:lo + N * nrhs].reshape(N, nrhs)

    def close(self):
        for M in self.M.values():
            M.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_r, self.d_z, self.d_r1, self.d_z1):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Problem(exec_, comm, name)
        return made[name]
    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("kind", ["sgs", "ilu0"])
@pytest.mark.parametrize("name", NAMES)
def test_apply_block_equals_apply_per_column(problems, name, kind):
    P = problems(name)
    if name == "ragged3001":
        assert P.M[("sgs", False)].num_colors() >= 24
    for sym in (False, True):
        M = P.M[(kind, sym)]
        want = [P.numpy_apply[(kind, sym)](P.R[:, c]) for c in range(8)]
        for c in range(8):  # the single-vector sweep on the GPU, once per column
            assert np.array_equal(P.single(M, P.R[:, c]), want[c]), (name, kind, c)
        for nrhs in NRHS:
            for r_off, z_off in OFFSETS:
                Z = P.block(M, nrhs, r_off, z_off)
                for c in range(nrhs):
                    assert np.array_equal(Z[:, c], want[c]), (
                        name, kind, sym, nrhs, r_off, z_off, c)


def test_bad_nrhs_and_overlap_are_refused_and_write_nothing(problems):
    P = problems("poisson11")
    e, N, M = P.exec_, P.N, P.M[("sgs", False)]
    size = N * 8 + 2 * G + 2
    e.copy_from_host(P.d_z, np.full(size, SENTINEL))
    e.copy_from_host(P.d_r, np.full(N * 8 + 2, SENTINEL))
    for nrhs in (0, 9, -1):
        with pytest.raises(host.SpmvHostError, match="nrhs"):
            host.sgs_apply_block(e, M, P.d_r, P.d_z, nrhs)
    for nrhs in (1, 4):
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.sgs_apply_block(e, M, P.d_z, P.d_z, nrhs)
        with pytest.raises(host.SpmvHostError, match="overlaps"):  # one double
            host.sgs_apply_block(e, M, P.d_z, P.d_z + 8 * (N * nrhs - 1), nrhs)
    e.synchronize()
    assert np.all(e.copy_to_host(P.d_z, size) == SENTINEL)
    assert np.all(e.copy_to_host(P.d_r, N * 8 + 2) == SENTINEL)
    # next to each other, not sharing a byte: accepted
    e.copy_from_host(P.d_z, np.ascontiguousarray(P.R[:, :4]))
    host.sgs_apply_block(e, M, P.d_z, P.d_z + 8 * N * 4, 4)
    Z = e.copy_to_host(P.d_z + 8 * N * 4, N * 4).reshape(N, 4)
    assert np.array_equal(Z[:, 3], P.numpy_apply[("sgs", False)](P.R[:, 3]))
