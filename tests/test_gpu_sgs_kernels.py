"""mcgs_sweep_kernel (hip/spmv_mcgs.hip) and ilu0_factor_kernel with its helpers
(hip/spmv_ilu0.hip) launched ALONE through the C ABI, on the cases and recipes
of sgs_kernel_cases.py: plans built from sgs_layout.py's arrays, so the colours
are the case's own and every case reaches the decision point it is named after
(test_sgs_kernel_cases_host.py proves that without a device).

Everything is bit for bit (special_values.same_bits: NaN as a class, the sign
of a zero counts), no tolerances, no solves:
  sweep   z against Ilu0Ref.apply on the matrix's own values; the set of
          non-finite entries equal to the reference's (a multiplied padding
          slot is 0 * the poisoned z[0]); r and z between guard words, z
          prefilled as the recipe says; with a workspace whose `done` flag is
          set (raised the way test_gpu_blas1_kernels.py raises it) z stays its
          prefill;
  factor  l~, u~, d~ of ilu0_get_factor against Ilu0Ref.factor, ilu0_pivots
          against the counts of the reference's pivots, the sweeps on the
          inner plan against Ilu0Ref.apply on that factor; then the benign
          values on the same plan: the counts back at 0, the benign factor."""
import ctypes as C

import numpy as np
import pytest

import sgs_kernel_cases as kc
import sgs_layout as sl
import special_values as sv
from spmv_amd import hip
from test_gpu_blas1_kernels import PcgWs

pytestmark = pytest.mark.gpu

G = 16  # guard doubles on either side of r and z
GUARD = -7.25e77


def _combos(which):
    return [pytest.param(name, rname, id=f"{name}-{rname}")
            for name, case in kc.cases().items()
            for rname, rec in case.recipes().items() if getattr(rec, which)]


class _Dev:
    """the device side of one case: the ILU(0) plan, vectors between guards"""

    def __init__(self, ctx, case):
        self.ctx, self.case, n = ctx, case, case.n
        self.struct, self.keep = sl.ilu0_host(case.lay, case.nnz)
        self.plan = C.c_void_p()
        hip.call("spmv_hip_ilu0_plan_create", ctx.h,
                 C.cast(C.pointer(self.struct), C.c_void_p), C.byref(self.plan))
        self.inner = C.c_void_p()
        hip.call("spmv_hip_ilu0_mcgs_plan", self.plan, C.byref(self.inner))
        self.values = ctx.empty(case.nnz, np.float64)
        self.diag = ctx.empty(n, np.float64)
        self.r = ctx.empty(n + 2 * G + 1, np.float64)
        self.z = ctx.empty(n + 2 * G + 1, np.float64)
        self._facs = {}

    def close(self):
        self.ctx.stream_sync()
        hip.call("spmv_hip_ilu0_plan_destroy", self.plan)
        for b in (self.values, self.diag, self.r, self.z):
            b.free()

    # -- references, computed once per set of values ---------------------------------
    def ref_factor(self, va):
        key = va.tobytes()
        if key not in self._facs:
            self._facs[key] = self.case.ref.factor(va, self.case.diag_of(va))
        return self._facs[key]

    # -- the sweeps ---------------------------------------------------------------------
    def sweep(self, plan, ws, r, z0, off=0):
        """-> z; r and z `off` doubles off 16-byte alignment, guards checked"""
        n, ctx = self.case.n, self.ctx
        for buf, data in ((self.r, r), (self.z, z0)):
            img = np.full(n + 2 * G + 1, GUARD)
            img[G + off:G + off + n] = data
            buf.write(img)
        hip.call("spmv_hip_mcgs_apply_f64", ctx.h, plan, ws, self.r.at(G + off),
                 self.z.at(G + off), None)
        ctx.stream_sync()
        r_back, z_back = self.r.numpy(), self.z.numpy()
        for img, what in ((r_back, "r"), (z_back, "z")):
            assert np.all(img[:G + off] == GUARD), (what, "guard in front")
            assert np.all(img[G + off + n:] == GUARD), (what, "guard behind")
        assert sv.same_bits(r_back[G + off:G + off + n], np.asarray(r, np.float64))
        return z_back[G + off:G + off + n].copy()

    def check_sweep(self, plan, rec, want, what):
        for off in (0, 1):
            z = self.sweep(plan, None, rec.r, rec.z0, off)
            _same(z, want, what + (off,))
            # exactly the reference's non-finite entries: no padding multiplied
            assert np.array_equal(np.isfinite(z), np.isfinite(want)), what

    # -- the factor -----------------------------------------------------------------------
    def factor(self, va):
        case, ctx = self.case, self.ctx
        self.values.write(va)
        self.diag.write(case.diag_of(va))
        hip.call("spmv_hip_ilu0_factor", ctx.h, self.plan, self.values.ptr,
                 self.diag.ptr, None)
        B, A = case.ref.parts
        l, u, d = np.zeros(len(B["src"])), np.zeros(len(A["src"])), np.zeros(case.n)
        hip.call("spmv_hip_ilu0_get_factor", ctx.h, self.plan,
                 *[a.ctypes.data_as(C.c_void_p) for a in (l, u, d)], None)
        bad, neg = C.c_int64(-1), C.c_int64(-1)
        hip.call("spmv_hip_ilu0_pivots", ctx.h, self.plan, C.byref(bad),
                 C.byref(neg), None)
        return (l, u, d), (bad.value, neg.value)


def _same(got, want, what):
    if not sv.same_bits(got, want):
        nan = np.isnan(want)
        bad = np.flatnonzero((np.isnan(got) != nan)
                             | (~nan & (sv.bits(got) != sv.bits(want))))
        raise AssertionError(
            f"{what}: {bad.size} of {len(want)} entries differ, first at "
            f"{bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


@pytest.fixture(scope="module")
def devs(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Dev(ctx, kc.cases()[name])
        return made[name]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def done_ws(ctx):
    w = PcgWs(ctx)
    w.raise_done()
    yield w
    w.close()


# ---- the sweep kernel alone ------------------------------------------------------------------
@pytest.mark.parametrize("name,rname", _combos("sweep"))
def test_sweep(ctx, devs, done_ws, name, rname):
    dev = devs(name)
    case = dev.case
    rec = case.recipes()[rname]
    l, u, d = fac = case.parts_values(rec.va)
    with np.errstate(all="ignore"):
        dinv = 1.0 / case.diag_of(rec.va)
    want = case.apply(fac, rec.r)
    struct, keep = sl.mcgs_host(sl.with_values(case.lay, l, u), dinv)
    plan = C.c_void_p()
    hip.call("spmv_hip_mcgs_plan_create", ctx.h,
             C.cast(C.pointer(struct), C.c_void_p), C.byref(plan))
    try:
        dev.check_sweep(plan, rec, want, (name, rname))
        # after `done` every launch returns at once: z is its prefill
        assert done_ws.done() == 1
        for z0 in (rec.z0, np.arange(1.0, case.n + 1.0)):
            z = dev.sweep(plan, done_ws.h, rec.r, z0)
            _same(z, np.asarray(z0, np.float64), (name, rname, "done"))
    finally:
        ctx.stream_sync()
        hip.call("spmv_hip_mcgs_plan_destroy", plan)


# ---- the factor kernels alone --------------------------------------------------------------
def _check_factor(dev, va, what, stated=None):
    want = dev.ref_factor(va)
    got, counts = dev.factor(va)
    for g, w, part in zip(got, want, ("l", "u", "d")):
        _same(g, w, what + (part,))
    assert counts == kc.pivot_counts(want[2]), what
    if stated is not None:
        assert counts == stated, what
    return want


@pytest.mark.parametrize("name,rname", _combos("factor"))
def test_factor(ctx, devs, name, rname):
    dev = devs(name)
    case = dev.case
    rec = case.recipes()[rname]
    fac = _check_factor(dev, rec.va, (name, rname), rec.pivots)
    if rname == "pivots":
        assert rec.pivots == kc.PIVOT_COUNTS and case.n == 256 * 3 + 17
    # the sweeps on the plan whose values and dinv the factor wrote
    dev.check_sweep(dev.inner, rec, case.apply(fac, rec.r), (name, rname, "apply"))
    if rname != "benign":  # the same plan again: the counts start at 0
        benign = case.recipes()["benign"]
        fac = _check_factor(dev, benign.va, (name, rname, "benign again"), (0, 0))
        z = dev.sweep(dev.inner, None, benign.r, benign.z0)
        _same(z, case.apply(fac, benign.r), (name, rname, "benign apply"))
