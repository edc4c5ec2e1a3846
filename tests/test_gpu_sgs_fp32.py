"""SgsOptions::values = fp32: sweep plans that keep their off-diagonal values as
float (SgsPreconditioner and Ilu0Preconditioner, values="fp32").

The definition is exact, so everything but the whole solves is bit for bit
(special_values.same_bits: NaN as a class, the sign of a zero counts; outputs
prefilled with NaN or a sentinel): the stored value is the fp64 value rounded to
nearest-even, and the sweeps compute acc = acc + (double)v32 * z[col] in the
entries' order -- the bits of the fp64 sweep on the widened values.  The
restatement is sgs_layout.sweep on val.astype(float32).astype(float64) with the
dinv of the fp64 object.

  kernel    mcgs_sweep_kernel<float> alone through spmv_hip_mcgs_plan_create_ex
            on the hand-coloured layout-edge cases of sgs_kernel_cases.py, on
            values that are NOT exact in fp32 (benign * (1 + k 2^-30), seeded
            gaussians) -- with the mutant check that the sweep on the unrounded
            values differs --, and on in-range special values (Inf / NaN in r
            and in the values, signed zeros);
  block     column c of mcgs_apply_block == mcgs_apply on column c of the
            narrowed plan, nrhs 1, 2, 3, 4, 8, R / Z aligned and 8 bytes off;
  export    widened-rounded values entry for entry, value_bits, plan_bytes;
  range     values out of fp32's range: SPMV_HIP_ERANGE and no plan;
  objects   three setups agree (host, device natural, colors=), SGS and ILU(0),
            both storages; exact matrices keep the bits of the fp64 object;
            ILU(0): factor() unchanged, apply on rounded l~ / u~, refactor,
            "fp32 range" from the constructor and from refactor;
  solves    pcg_sgs, pcg_block, gmres, minres with the fp32 object: converged,
            true residual (fp64 Matrix::mult) <= 10 max(rtol, that of the fp64
            object) -- the bar of test_gpu_gmres.py / test_gpu_minres.py with
            the fp64 object as the reference --, iterations <= 2 x the fp64
            object's (a cap against a broken preconditioner, not a measurement;
            the CPU restatement gives 28 / 28 and 9 / 9, test_sgs_fp32_host.py);
  ranks     the fp32 object on each rank's diagonal block == the one-rank
            object built from that block."""
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
from spmv_amd import _lib, hip, host
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)
from test_gpu_sgs_kernels import _same
from test_sgs_fp32_host import nonsymmetric, range_count_ref, rounded

pytestmark = pytest.mark.gpu

G = 16
GUARD = -7.25e77
NRHS = (1, 2, 3, 4, 8)
ERANGE = -4
SENTINEL = tp.SENTINEL


# ---- values that are not exact in fp32 -------------------------------------------------
def _ulp30(case):
    va = case.benign_values()
    k = np.arange(case.nnz)
    return va * (1.0 + (1 + k % 97) * 2.0 ** -30)


def _gauss(case):
    off = np.random.default_rng(case.n).standard_normal(case.nnz)
    return case._with_diagonal(off, 1.0 + (np.arange(case.n) % 4) / 4.0)


def _nonfinite_values(case):
    """in range all the same: zeros of both signs, an Inf and a NaN among the
    entries convert as IEEE says"""
    va = _ulp30(case)
    off = np.flatnonzero(~case.on)
    va[off[0::40]] = -0.0
    va[off[10::40]] = 0.0
    va[off[len(off) // 2]] = np.inf
    va[off[len(off) // 3]] = -np.inf
    va[off[len(off) // 5]] = np.nan
    return va


def _recipe(case, rname):
    """-> (values, r, z0, the unrounded sweep must differ)"""
    recs = case.recipes()
    if rname == "ulp30":
        return _ulp30(case), case.benign_r(), np.full(case.n, np.nan), True
    if rname == "gauss":
        r = np.random.default_rng(case.n + 1).standard_normal(case.n)
        return _gauss(case), r, np.full(case.n, np.nan), True
    if rname == "poison":  # Inf, -Inf, NaN in r; z prefilled with Inf / NaN
        return _ulp30(case), recs["poison"].r, recs["poison"].z0, False
    if rname == "negzero":
        va = recs["negzero"].va * (1.0 + 2.0 ** -30)
        return va, recs["negzero"].r, recs["negzero"].z0, False
    return _nonfinite_values(case), case.benign_r(), np.full(case.n, np.nan), False


RECIPES = ("ulp30", "gauss", "poison", "negzero", "nonfinite_values")


class _Plans:
    """the narrowed plan of (case, recipe) from the HOST description with the
    unrounded values, and the restatement's layouts"""

    def __init__(self, ctx, case, rname):
        self.case = case
        self.va, self.r, self.z0, self.mutant = _recipe(case, rname)
        l, u, _ = case.parts_values(self.va)
        with np.errstate(all="ignore"):
            self.dinv = 1.0 / case.diag_of(self.va)
        self.wide = sl.with_values(case.lay, l, u)
        self.narrow = sl.with_values(case.lay, rounded(l), rounded(u))
        assert range_count_ref(l) == range_count_ref(u) == 0
        self.struct, self.keep = sl.mcgs_host(self.wide, self.dinv)
        self.plan, count = C.c_void_p(), C.c_int64(-1)
        hip.call("spmv_hip_mcgs_plan_create_ex", ctx.h,
                 C.cast(C.pointer(self.struct), C.c_void_p), 32,
                 C.byref(self.plan), C.byref(count))
        assert count.value == 0
        self.ctx = ctx

    def close(self):
        self.ctx.stream_sync()
        hip.call("spmv_hip_mcgs_plan_destroy", self.plan)


def _apply(ctx, plan, n, d_r, d_z, r, z0, off):
    for buf, data in ((d_r, r), (d_z, z0)):
        img = np.full(n + 2 * G + 1, GUARD)
        img[G + off:G + off + n] = data
        buf.write(img)
    hip.call("spmv_hip_mcgs_apply_f64", ctx.h, plan, None, d_r.at(G + off),
             d_z.at(G + off), None)
    ctx.stream_sync()
    z_back = d_z.numpy()
    assert np.all(z_back[:G + off] == GUARD) and np.all(z_back[G + off + n:] == GUARD)
    assert sv.same_bits(d_r.numpy()[G + off:G + off + n], np.asarray(r, np.float64))
    return z_back[G + off:G + off + n].copy()


def _combos(recipes):
    return [pytest.param(name, rname, id=f"{name}-{rname}")
            for name in kc.cases() for rname in recipes]


# ---- 3. the kernel alone ----------------------------------------------------------------------
@pytest.mark.parametrize("name,rname", _combos(RECIPES))
def test_sweep_on_a_narrowed_plan(ctx, name, rname):
    case = kc.cases()[name]
    P = _Plans(ctx, case, rname)
    n = case.n
    d_r, d_z = (ctx.empty(n + 2 * G + 1, np.float64) for _ in range(2))
    try:
        bits = C.c_int()
        hip.call("spmv_hip_mcgs_plan_value_bits", P.plan, C.byref(bits))
        assert bits.value == 32
        want = sl.sweep(P.narrow, P.dinv, P.r, P.z0)
        if P.mutant:  # the test can tell the two apart
            assert not sv.same_bits(sl.sweep(P.wide, P.dinv, P.r, P.z0), want)
        for off in (0, 1):
            z = _apply(ctx, P.plan, n, d_r, d_z, P.r, P.z0, off)
            _same(z, want, (name, rname, off))
            assert np.array_equal(np.isfinite(z), np.isfinite(want))
    finally:
        P.close()
        d_r.free()
        d_z.free()


# ---- 4. the block form ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.cases()))
def test_block_sweep_on_a_narrowed_plan(ctx, name):
    case = kc.cases()[name]
    P = _Plans(ctx, case, "gauss")
    n = case.n
    # every column another r and prefill: a lane that mixed columns up would show
    cols = [_recipe(case, r)[1:3] for r in ("gauss", "ulp30", "poison", "negzero")]
    size = n * max(NRHS) + 2 * G + 1
    d_r, d_z = ctx.empty(size, np.float64), ctx.empty(size, np.float64)
    d_r1, d_z1 = (ctx.empty(n + 2 * G + 1, np.float64) for _ in range(2))
    try:
        single = [_apply(ctx, P.plan, n, d_r1, d_z1, r, z0, 0) for r, z0 in cols]
        _same(single[0], sl.sweep(P.narrow, P.dinv, *cols[0]), (name, "single"))
        for nrhs in NRHS:
            pick = [c % len(cols) for c in range(nrhs)]
            R = np.stack([np.asarray(cols[c][0], np.float64) for c in pick], 1)
            Z0 = np.stack([np.asarray(cols[c][1], np.float64) for c in pick], 1)
            for off in (0, 1):
                lo, hi = G + off, G + off + n * nrhs
                for buf, data in ((d_r, R), (d_z, Z0)):
                    img = np.full(size, GUARD)
                    img[lo:hi] = data.reshape(-1)
                    buf.write(img)
                hip.call("spmv_hip_mcgs_apply_block_f64", ctx.h, P.plan, None,
                         d_r.at(lo), d_z.at(lo), nrhs, None)
                ctx.stream_sync()
                r_back, z_back = d_r.numpy(), d_z.numpy()
                what = (name, nrhs, off)
                for img in (r_back, z_back):
                    assert np.all(img[:lo] == GUARD) and np.all(img[hi:] == GUARD), what
                assert sv.same_bits(r_back[lo:hi], R.reshape(-1)), what
                Z = z_back[lo:hi].reshape(n, nrhs)
                for c, s in enumerate(pick):
                    _same(np.ascontiguousarray(Z[:, c]), single[s], what + (c,))
    finally:
        P.close()
        for b in (d_r, d_z, d_r1, d_z1):
            b.free()


# ---- 5. export, width and bytes -----------------------------------------------------------
def _export(plan):
    sizes = np.zeros(10, np.int64)
    hip.call("spmv_hip_mcgs_plan_sizes", plan, sizes.ctypes.data_as(C.c_void_p))
    out, structs = {}, []
    for h, name in enumerate(("before", "after")):
        ent, lent = int(sizes[3 + 3 * h]), int(sizes[5 + 3 * h])
        out[name] = dict(val=np.full(ent, np.nan), long_val=np.full(lent, np.nan))
        s = sl._McgsPart()
        if ent:
            s.val = out[name]["val"].ctypes.data_as(C.c_void_p)
        if lent:
            s.long_val = out[name]["long_val"].ctypes.data_as(C.c_void_p)
        structs.append(s)
    hip.call("spmv_hip_mcgs_plan_export", plan, None, None, None,
             C.cast(C.pointer(structs[0]), C.c_void_p),
             C.cast(C.pointer(structs[1]), C.c_void_p))
    return sizes, out


@pytest.mark.parametrize("name", list(kc.cases()))
def test_export_width_and_bytes(ctx, name):
    case = kc.cases()[name]
    P = _Plans(ctx, case, "gauss")
    plan64 = C.c_void_p()
    hip.call("spmv_hip_mcgs_plan_create", ctx.h,
             C.cast(C.pointer(P.struct), C.c_void_p), C.byref(plan64))
    try:
        sizes, got = _export(P.plan)
        sizes64, got64 = _export(plan64)
        stored = 0
        for h in ("before", "after"):
            for k in ("val", "long_val"):
                want = P.narrow[h]["sliced"][k]
                assert sv.same_bits(got[h][k], want), (name, h, k)
                assert sv.same_bits(got64[h][k], P.wide[h]["sliced"][k]), (name, h, k)
                assert not sv.same_bits(got[h][k], got64[h][k]) or len(want) == 0
                stored += len(want)
        assert np.array_equal(sizes[:9], sizes64[:9])
        b32, b64, bits = C.c_int64(), C.c_int64(), C.c_int()
        hip.call("spmv_hip_mcgs_plan_bytes", P.plan, C.byref(b32))
        hip.call("spmv_hip_mcgs_plan_bytes", plan64, C.byref(b64))
        # the formula of include/spmv_hip.h
        assert stored == sizes[3] + sizes[5] + sizes[6] + sizes[8] > 0
        assert b32.value == b64.value - 4 * stored == sizes[9]
        hip.call("spmv_hip_mcgs_plan_value_bits", plan64, C.byref(bits))
        assert bits.value == 64
        # value_bits = 64 through the _ex entry: the plan of mcgs_plan_create
        again, count = C.c_void_p(), C.c_int64(-1)
        hip.call("spmv_hip_mcgs_plan_create_ex", ctx.h,
                 C.cast(C.pointer(P.struct), C.c_void_p), 64, C.byref(again),
                 C.byref(count))
        hip.call("spmv_hip_mcgs_plan_bytes", again, C.byref(b32))
        assert b32.value == b64.value and count.value == 0
        hip.call("spmv_hip_mcgs_plan_destroy", again)
    finally:
        P.close()
        hip.call("spmv_hip_mcgs_plan_destroy", plan64)


@pytest.mark.parametrize("rname", ["overflow_before", "subnormal"])
def test_values_out_of_range_make_no_plan(ctx, rname):
    """the project's overflow (+-M near DBL_MAX) and subnormal recipes leave
    fp32's range: counted on the device, SPMV_HIP_ERANGE, nothing allocated"""
    case = kc.cases()["rows_of_64_65_127_128_129_192"]
    rec = case.recipes()[rname]
    l, u, _ = case.parts_values(rec.va)
    want = range_count_ref(l) + range_count_ref(u)
    assert want > 0
    with np.errstate(all="ignore"):
        dinv = 1.0 / case.diag_of(rec.va)
    struct, keep = sl.mcgs_host(sl.with_values(case.lay, l, u), dinv)
    live0 = C.c_int64()
    _lib.hip.spmv_hip_plan_live_allocations(C.byref(live0))
    plan, count = C.c_void_p(), C.c_int64(-1)
    rc = _lib.hip.spmv_hip_mcgs_plan_create_ex(
        ctx.h, C.cast(C.pointer(struct), C.c_void_p), 32, C.byref(plan),
        C.byref(count))
    assert rc == ERANGE and not plan.value and count.value == want
    live1 = C.c_int64()
    _lib.hip.spmv_hip_plan_live_allocations(C.byref(live1))
    assert live1.value == live0.value


# ---- 6 / 7. the objects -------------------------------------------------------------------
def _matrix(name):
    if name == "poisson12":
        return tp._csr("poisson12")
    return ts.ragged_spd(2001, 11)


class _Objects:
    def __init__(self, exec_, comm, name):  # noqa: F811
        self.exec_, self.csr = exec_, _matrix(name)
        self.N = N = len(self.csr[0]) - 1
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.r = oracle.csr_spmv(*self.csr,
                                 np.random.default_rng(N + 3).uniform(-1, 1, N))
        self.d_r, self.d_z = exec_.alloc(N), exec_.alloc(N)

    def apply(self, M):
        e = self.exec_
        e.copy_from_host(self.d_r, self.r)
        e.copy_from_host(self.d_z, np.full(self.N, SENTINEL))
        host.sgs_apply(e, M, self.d_r, self.d_z)
        return e.copy_to_host(self.d_z, self.N)

    def close(self):
        for A in self.A.values():
            A.close()
        self.exec_.free(self.d_r), self.exec_.free(self.d_z)


@pytest.fixture(scope="module")
def objects(exec_, comm):  # noqa: F811
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Objects(exec_, comm, name)
        return made[name]
    yield get
    for o in made.values():
        o.close()


def _same_arrays(a, b, what):
    for k in ("perm", "color_start", "dinv"):
        assert sv.same_bits(a[k], b[k]) if k == "dinv" else np.array_equal(a[k], b[k]), (what, k)
    for h in ("before", "after"):
        for k, _ in host.SgsPreconditioner._PART_KEYS:
            x, y = a[h][k], b[h][k]
            same = sv.same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)
            assert same, (what, h, k)


@pytest.mark.parametrize("cls", ["sgs", "ilu0"])
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", ["poisson12", "ragged2001"])
def test_three_setups_agree(objects, name, symmetric, cls):
    O = objects(name)
    make = host.SgsPreconditioner if cls == "sgs" else host.Ilu0Preconditioner
    A, e = O.A[symmetric], O.exec_
    Ms = [make(e, A, setup="host", values="fp32")]
    try:
        Ms.append(make(e, A, setup="device", order="natural", values="fp32"))
        Ms.append(make(e, A, setup="device", colors=Ms[0].colors(), values="fp32"))
        M64 = make(e, A)
        Ms.append(M64)
        assert [M.value_bits for M in Ms] == [32, 32, 32, 64]
        arrays = [M.plan_arrays() for M in Ms]
        z = [O.apply(M) for M in Ms]
        for i in (1, 2):
            _same_arrays(arrays[i], arrays[0], (name, symmetric, cls, i))
            assert np.array_equal(z[i], z[0]), (name, symmetric, cls, i)
        # the narrowed plan is the fp64 plan with its values rounded, dinv as it is
        stored = 0
        for h in ("before", "after"):
            for k in ("val", "long_val"):
                assert sv.same_bits(arrays[0][h][k], rounded(arrays[3][h][k]))
                stored += len(arrays[0][h][k])
        assert sv.same_bits(arrays[0]["dinv"], arrays[3]["dinv"])
        assert Ms[0].plan_bytes() == M64.plan_bytes() - 4 * stored
        # ... and the sweep is the restatement on those arrays
        lay = dict(n=O.N, num_colors=Ms[0].num_colors(), perm=arrays[0]["perm"],
                   color_start=arrays[0]["color_start"],
                   before=dict(sliced=arrays[0]["before"]),
                   after=dict(sliced=arrays[0]["after"]))
        want = sl.sweep(lay, arrays[0]["dinv"], O.r, np.full(O.N, np.nan))
        assert np.array_equal(z[0], want)
        # 6 and -1 are exact -- also for ILU(0) HERE: with two colours the
        # elimination changes only the pivots, l~ = u~ = -1, and dinv~ is fp64
        exact = name == "poisson12"
        assert np.array_equal(z[0], z[3]) == exact, (name, cls)
    finally:
        for M in Ms:
            M.close()


def test_exact_matrices_keep_their_bits(objects, comm):  # noqa: F811
    """Poisson 12^3 has the values 6 and -1: the fp32 object IS the fp64 one,
    in sgs_apply and in the whole pcg_sgs history"""
    O = objects("poisson12")
    e, N = O.exec_, O.N
    d_x = e.alloc(N)
    for sym in (False, True):
        M32 = host.SgsPreconditioner(e, O.A[sym], values="fp32")
        M64 = host.SgsPreconditioner(e, O.A[sym])
        try:
            assert np.array_equal(O.apply(M32), O.apply(M64))
            runs = []
            for M in (M32, M64):
                e.copy_from_host(O.d_r, O.r)
                e.copy_from_host(d_x, np.full(N, SENTINEL))
                k, hist = host.pcg_sgs(comm, e, O.A[sym], M, O.d_r, d_x, 200, 1e-10)
                runs.append((k, hist[:k + 1].copy(), e.copy_to_host(d_x, N)))
            assert runs[0][0] == runs[1][0] < 200
            assert np.array_equal(runs[0][1], runs[1][1])
            assert np.array_equal(runs[0][2], runs[1][2])
        finally:
            M32.close()
            M64.close()
    e.free(d_x)


# ---- 8. ILU(0) ----------------------------------------------------------------------------------
def _ilu_matrix():
    """about 1 000 rows, nonsymmetric, strictly diagonally dominant, inexact
    values, two hub rows of about 500 entries (the long-row path)"""
    return nonsymmetric(ts.ragged_spd(1001, 5))


def _ilu_restatement(ref, lay, fac, r):
    l, u, d = fac
    dinv = np.zeros(ref.n)
    dinv[ref.perm] = 1.0 / d
    return sl.sweep(sl.with_values(lay, rounded(l), rounded(u)), dinv, r,
                    np.full(ref.n, np.nan))


def test_ilu0_factor_apply_refactor_and_range(exec_, comm):  # noqa: F811
    e = exec_
    csr = _ilu_matrix()
    rp, ci, va = csr
    N = len(rp) - 1
    assert np.diff(rp).max() > 64
    r = oracle.csr_spmv(*csr, np.random.default_rng(8).uniform(-1, 1, N))
    d_r, d_z = e.alloc(N), e.alloc(N)

    def apply(M):
        e.copy_from_host(d_r, r)
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.ilu0_apply(e, M, d_r, d_z)
        return e.copy_to_host(d_z, N)

    def matrix(values):
        return host.Matrix.create_matrix(comm, e, rp, ci, values, N, N, [], [],
                                         False, host.P2P_NONBLOCKING)

    A = matrix(va)
    M = host.Ilu0Preconditioner(e, A, values="fp32")
    M64 = host.Ilu0Preconditioner(e, A)
    made = [A, M, M64]
    try:
        ref = ic.Ilu0Ref(csr, N, M.colors(), False)
        lay = sl.layout(ref)
        fac = ref.factor()
        for got, want in zip(M.factor(), fac):  # the factorisation stays fp64
            assert np.array_equal(got, want)
        assert M.value_bits == 32 and M.negative_pivots() == 0
        want = _ilu_restatement(ref, lay, fac, r)
        z = apply(M)
        assert np.array_equal(z, want)
        assert not np.array_equal(z, apply(M64))  # the factor is not fp32-exact
        assert not np.array_equal(want, ref.apply(fac, r))
        stored = sum(len(M.plan_arrays()[h][k]) for h in ("before", "after")
                     for k in ("val", "long_val"))
        assert M.plan_bytes() == M64.plan_bytes() - 4 * stored
        # refactor with new values rounds again
        va2 = va * (1.0 + 0.125 * np.cos(np.arange(len(va))) ** 2)
        on = ci == tp._row_of(rp)
        va2[on] = va[on] * 1.25
        A2 = matrix(va2)
        made.append(A2)
        M.refactor(A2)
        fac2 = ref.factor(va2, tp._diag_of((rp, ci, va2)))
        for got, w in zip(M.factor(), fac2):
            assert np.array_equal(got, w)
        assert np.array_equal(apply(M), _ilu_restatement(ref, lay, fac2, r))
        # one l~ of a row of the LAST colour overflows fp32: only its own pivot
        # feels it, which stays finite
        B = ref.parts[0]
        last = int(ref.n - 1)  # the last position wears the last colour
        assert B["ptr"][last + 1] > B["ptr"][last]
        bad = va.copy()
        bad[B["src"][B["ptr"][last]]] = 1e39
        facb = ref.factor(bad, tp._diag_of((rp, ci, bad)))
        assert range_count_ref(facb[0]) + range_count_ref(facb[1]) >= 1
        assert np.all(np.isfinite(facb[2])) and np.all(facb[2] != 0.0)
        Ab = matrix(bad)
        made.append(Ab)
        with pytest.raises(host.SpmvHostError, match="fp32 range"):
            host.Ilu0Preconditioner(e, Ab, values="fp32")
        with pytest.raises(host.SpmvHostError, match="fp32 range"):
            host.Ilu0Preconditioner(e, Ab, setup="device", order="natural",
                                    values="fp32")
        host.Ilu0Preconditioner(e, Ab).close()  # fine in fp64
        with pytest.raises(host.SpmvHostError, match="fp32 range"):
            M.refactor(Ab)
        with pytest.raises(host.SpmvHostError, match="fp32 range"):
            host.ilu0_apply(e, M, d_r, d_z)  # unusable until a good refactor
        M.refactor(A)
        assert np.array_equal(apply(M), want)
        # a subnormal-rounding off-diagonal raises for SGS too, on both setups
        tiny = va.copy()
        tiny[np.flatnonzero(~on)[7]] = 1e-42
        At = matrix(tiny)
        made.append(At)
        for kw in (dict(), dict(setup="device"), dict(setup="device", order="natural")):
            with pytest.raises(host.SpmvHostError, match="fp32 range"):
                host.SgsPreconditioner(e, At, values="fp32", **kw)
        host.SgsPreconditioner(e, At).close()
    finally:
        for obj in reversed(made):
            obj.close()
        e.free(d_r), e.free(d_z)


# ---- 9. whole solves -------------------------------------------------------------------------
def _true_residual(e, A, d_x, d_y, x, b):
    """||b - A x|| / ||b|| with A x from the fp64 Matrix::mult"""
    e.copy_from_host(d_x, x)
    A.col_map().update(d_x)
    A.mult(d_x, d_y)
    return float(np.linalg.norm(b - e.copy_to_host(d_y, len(b))) / np.linalg.norm(b))


@pytest.mark.parametrize("solver", ["pcg_sgs", "pcg_block", "gmres", "minres"])
def test_whole_solves_with_the_fp32_object(exec_, comm, solver):  # noqa: F811
    """the unstructured matrix: on Poisson the fp32 object is the fp64 one and
    the test would be vacuous"""
    e, rtol, kmax = exec_, 1e-10, 200
    csr = ts.ragged_spd(2001, 11)
    if solver == "gmres":
        csr = nonsymmetric(csr)
    N = len(csr[0]) - 1
    nrhs = 3 if solver == "pcg_block" else 1
    rng = np.random.default_rng(N + 9)
    B = np.stack([oracle.csr_spmv(*csr, rng.uniform(-1, 1, N)) for _ in range(nrhs)], 1)
    A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], False,
                                  host.P2P_NONBLOCKING)
    d_b, d_x = e.alloc(N * nrhs), e.alloc(N * nrhs)
    d_t, d_y = e.alloc(N), e.alloc(N)
    Ms = {}
    try:
        out = {}
        for width in ("fp64", "fp32"):
            M = Ms[width] = host.SgsPreconditioner(e, A, values=width)
            e.copy_from_host(d_b, np.ascontiguousarray(B))
            e.copy_from_host(d_x, np.full(N * nrhs, SENTINEL))
            if solver == "pcg_sgs":
                k, hist = host.pcg_sgs(comm, e, A, M, d_b, d_x, kmax, rtol)
                ks, rel = [k], [hist[k] / hist[0]]
            elif solver == "pcg_block":
                its, hist, _ = host.pcg_block(comm, e, A, d_b, d_x, nrhs, kmax,
                                              rtol, sgs=M)
                ks = [int(k) for k in its]
                rel = [hist[c, k] / hist[c, 0] for c, k in enumerate(ks)]
            elif solver == "gmres":
                k, hist, status = host.gmres(comm, e, A, d_b, d_x, 30, kmax, rtol,
                                             sgs=M)
                assert status == 0
                ks, rel = [k], [hist[k] / hist[0]]
            else:
                k, hist, status = host.minres(comm, e, A, d_b, d_x, kmax, rtol,
                                              sgs=M)
                assert status == 0
                ks, rel = [k], [hist[k] / hist[0]]
            X = e.copy_to_host(d_x, N * nrhs).reshape(N, nrhs)
            res = [_true_residual(e, A, d_t, d_y, np.ascontiguousarray(X[:, c]),
                                  B[:, c]) for c in range(nrhs)]
            out[width] = (ks, rel, res)
            print(solver, width, "k", ks, "recurrence", rel, "true residual", res)
            assert all(k < kmax for k in ks) and all(v < rtol for v in rel)
        assert Ms["fp32"].value_bits == 32
        for c in range(nrhs):
            k64, k32 = out["fp64"][0][c], out["fp32"][0][c]
            assert k32 <= 2 * k64, (solver, c, k32, k64)
            assert out["fp32"][2][c] <= 10 * max(rtol, out["fp64"][2][c]), (solver, c)
    finally:
        for M in Ms.values():
            M.close()
        A.close()
        for p in (d_b, d_x, d_t, d_y):
            e.free(p)


# ---- 10. two ranks -----------------------------------------------------------------------------
def test_two_ranks_equal_the_one_rank_object_of_the_block(exec_, comm):  # noqa: F811
    """ranks as threads (as test_gpu_sgs.py runs them), the scaled Poisson
    matrix of 8^3 in two slabs: the fp32 object on a rank's diagonal block has
    the bits of the one-rank fp32 object built from that block alone"""
    from thread_world import ThreadWorld
    world = 2
    (rp, ci, va), _ = tp._slab_inputs(8)
    N = len(rp) - 1
    r_glob = oracle.csr_spmv(rp, ci, va, np.random.default_rng(2).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    want = {}
    for rank in range(world):  # the one-rank objects, here
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, _ = oracle.localise_rows(rp, ci, va, r0, r1)
        lrp, lci, lva = np.asarray(lrp), np.asarray(lci), np.asarray(lva)
        own = lci < M
        brp = np.concatenate([[0], np.cumsum(np.bincount(
            tp._row_of(lrp)[own], minlength=M))]).astype(np.int32)
        assert not np.array_equal(rounded(lva[own]), lva[own])
        d_r, d_z = exec_.alloc(M), exec_.alloc(M)
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, brp, lci[own], lva[own], M, M,
                                          [], [], sym, host.P2P_NONBLOCKING)
            for cls in (host.SgsPreconditioner, host.Ilu0Preconditioner):
                pre = cls(exec_, A, values="fp32")
                exec_.copy_from_host(d_r, r_glob[r0:r1])
                exec_.copy_from_host(d_z, np.full(M, SENTINEL))
                host.sgs_apply(exec_, pre, d_r, d_z)
                want[(rank, sym, cls.__name__)] = exec_.copy_to_host(d_z, M)
                pre.close()
            A.close()
        exec_.free(d_r), exec_.free(d_z)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        d_r, d_z = exec_.alloc(M), exec_.alloc(M)
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [], gh,
                                          sym, host.P2P_NONBLOCKING)
            for cls in (host.SgsPreconditioner, host.Ilu0Preconditioner):
                pre = cls(exec_, A, values="fp32")
                assert pre.value_bits == 32
                exec_.copy_from_host(d_r, r_glob[r0:r1])
                exec_.copy_from_host(d_z, np.full(M, SENTINEL))
                host.sgs_apply(exec_, pre, d_r, d_z)
                z = exec_.copy_to_host(d_z, M)
                assert np.array_equal(z, want[(rank, sym, cls.__name__)]), (
                    rank, sym, cls.__name__)
                pre.close()
            A.close()
        exec_.free(d_r), exec_.free(d_z)

    tw.run(rank_body, gpu=True)
