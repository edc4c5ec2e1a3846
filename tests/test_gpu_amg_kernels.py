"""The five kernels of hip/spmv_amg.hip launched ALONE through the C ABI
(spmv_hip_amg_*_f64) on the hand-built steps of amg_kernel_cases.py and compared
bit for bit (special_values.same_bits: NaN where and only where the restatement
has one) with its numpy restatements.

Every output lies between guard words and starts as the sentinel, every input is
read back and must be unchanged, and every case runs cached and non-temporal
(blas1_nt_min_elems at its default and at 1) on an executor of this module's
own.  The shapes are the smallest that reach each path: list lengths round a
wavefront, entry counts round a workgroup, one case beyond a pass of the grid
(its size taken from the device's CU count and asserted), two rounds of
amg_diag, one streaming unit and its neighbours, one wrap of the streaming
grid.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as ac
import amg_kernel_cases as kc
import test_gpu_amg as ta
import test_gpu_pcg as tp
from special_values import same_bits
from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

SENT, G = tp.SENTINEL, 16
NT_DEFAULT = tp.NT_DEFAULT
EINVAL = ta.EINVAL
STAT_WORDS = 257  # SPMV_HIP_AMG_STAT_WORDS
hip = _lib.hip


@pytest.fixture(scope="module")
def kexec():
    e = host.HipExecutor(0)
    yield e
    e.synchronize()
    e.close()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, kexec):
    _lib.call("spmv_hip_ctx_set_option", kexec.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", kexec.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


class Pool:
    """device memory of one test: guarded float64 vectors, plain index arrays
    and plans, all released by close()"""

    def __init__(self, e):
        self.e, self.ptrs, self.plans = e, [], []

    def vec(self, data, off=0):
        return Vec(self, np.asarray(data, np.float64), off)

    def out(self, n, off=0):
        return Vec(self, np.full(n, SENT), off)

    def raw(self, arr):
        """an array of any type as it is; never a NULL pointer"""
        arr = np.ascontiguousarray(arr)
        p = self.e.alloc(max(arr.nbytes, 8), np.uint8)
        self.ptrs.append(p)
        if arr.nbytes:
            self.e.copy_from_host(p, arr)
        return p

    def plan(self, step):
        arrays = {k: step[k] for k in ("agg", "member_ptr", "member", "src_ptr",
                                       "src", "xrow_ptr", "xrow_src")
                  if step[k] is not None}
        h = ta._AmgHost(**{k: step[k] for k in
                           ("fine_rows", "coarse_rows", "num_values",
                            "num_diagonal", "coarse_nnz")},
                        **{k: v.ctypes.data for k, v in arrays.items()})
        p = C.c_void_p()
        rc = hip.spmv_hip_amg_plan_create(self.e.context, C.byref(h), C.byref(p))
        assert rc == 0 and p.value, rc
        self.plans.append(p)
        return p

    def close(self):
        self.e.synchronize()
        for p in self.plans:
            assert hip.spmv_hip_amg_plan_destroy(p) == 0
        for p in self.ptrs:
            self.e.free(p)


class Vec:
    def __init__(self, pool, data, off):
        self.e, self.n, self.off, self.host = pool.e, len(data), off, data.copy()
        img = np.full(self.n + 2 * G + off, SENT)
        img[G + off:G + off + self.n] = data
        self.base = pool.raw(img)
        self.ptr = self.base + 8 * (G + off)

    def read(self, what):
        img = self.e.copy_to_host(self.base, self.n + 2 * G + self.off)
        lo = G + self.off
        assert np.all(img[:lo] == SENT), (what, "guard in front")
        assert np.all(img[lo + self.n:] == SENT), (what, "guard behind")
        return img[lo:lo + self.n].copy()

    def expect(self, want, what):
        got, want = self.read(what), np.asarray(want, np.float64)
        if not same_bits(got, want):
            bad = np.flatnonzero(~((got == want) & (np.signbit(got)
                                                    == np.signbit(want))
                                   | (np.isnan(got) & np.isnan(want))))
            raise AssertionError((what, f"{bad.size} of {self.n} differ, first at "
                                  f"{bad[0]}: got {got[bad[0]]!r}, want "
                                  f"{want[bad[0]]!r}"))

    def unchanged(self, what):
        self.expect(self.host, (what, "an input changed"))


@pytest.fixture
def pool(kexec):
    p = Pool(kexec)
    yield p
    p.close()


# ---- galerkin ------------------------------------------------------------------------------
def _galerkin(pool, case):
    ctx = pool.e.context
    plan = pool.plan(case.step)
    values = pool.vec(case.values)
    diagonal = pool.vec(case.diagonal) if case.diagonal is not None else None
    out = pool.out(case.step["coarse_nnz"])
    rc = hip.spmv_hip_amg_galerkin_f64(ctx, plan, values.ptr,
                                       diagonal.ptr if diagonal else None,
                                       out.ptr, None)
    assert rc == 0, case.name
    out.expect(kc.galerkin_ref(case.step, case.values, case.diagonal),
               ("galerkin", case.name))
    values.unchanged(case.name)
    if diagonal:
        diagonal.unchanged(case.name)


def test_galerkin_lists(pool, nt):
    for case in kc.galerkin_cases():
        _galerkin(pool, case)


def test_galerkin_beyond_one_pass_of_the_grid(pool, nt):
    cus = pool.e.num_cus
    case = kc.galerkin_wrap(cus)
    assert case.step["coarse_nnz"] > kc.grid_cap(cus) * kc.BLOCK
    _galerkin(pool, case)


# ---- diag ----------------------------------------------------------------------------------
def _stat(pool):
    ones = np.full(STAT_WORDS, 0xFFFFFFFFFFFFFFFF, np.uint64)
    return pool.vec(ones.view(np.float64))


def _diag(pool, case):
    ctx, n = pool.e.context, case.n
    d, dinv, stat = pool.out(n), pool.out(n), _stat(pool)
    if case.form == "general":
        rp, ci = pool.raw(case.rowptr), pool.raw(case.colind)
        values = pool.vec(case.values)
        rc = hip.spmv_hip_amg_diag_f64(ctx, None, n, n, rp, ci, values.ptr, None,
                                       d.ptr, dinv.ptr, stat.ptr, None)
        inputs = [values]
    else:
        plan = pool.plan(case.step)
        values, diagonal = pool.vec(case.values), pool.vec(case.diagonal)
        rc = hip.spmv_hip_amg_diag_f64(ctx, plan, n, n, None, None, values.ptr,
                                       diagonal.ptr, d.ptr, dinv.ptr, stat.ptr,
                                       None)
        inputs = [values, diagonal]
    assert rc == 0, case.name
    want_d, want_dinv, bad, gmax, _ = case.ref()
    words = stat.read(case.name).view(np.uint64)
    d.expect(want_d, ("d", case.name))
    dinv.expect(want_dinv, ("dinv", case.name))
    assert bad == case.bad
    assert int(words[0]) == bad, (case.name, int(words[0]), bad)
    if n == 0:  # the all-ones prefill is gone
        assert not np.any(words), case.name
    maxima = words[1:].view(np.float64)
    assert not np.any(np.isnan(maxima)) and np.all(maxima >= 0.0), case.name
    got = np.array([ac.nanless_max(maxima)])
    assert same_bits(got, np.array([gmax])), (case.name, got[0], gmax)
    for v in inputs:
        v.unchanged(case.name)


@pytest.mark.parametrize("variant", ["bad", "max_last"])
@pytest.mark.parametrize("form", ["general", "xrow"])
def test_diag(kexec, nt, form, variant):
    for case in kc.diag_cases():
        if case.form == form and case.name.split("-")[1] == variant:
            pool = Pool(kexec)
            try:
                _diag(pool, case)
            finally:
                pool.close()


# ---- restrict --------------------------------------------------------------------------------
def _restrict(pool, case):
    plan = pool.plan(case.step)
    r, w = pool.vec(case.r), pool.vec(case.w)
    rc_out = pool.out(case.step["coarse_rows"])
    rc = hip.spmv_hip_amg_restrict_f64(pool.e.context, plan, r.ptr, w.ptr,
                                       rc_out.ptr, None)
    assert rc == 0, case.name
    rc_out.expect(kc.restrict_ref(case.step, case.r, case.w),
                  ("restrict", case.name))
    r.unchanged(case.name), w.unchanged(case.name)


def test_restrict_aggregates(pool, nt):
    for case in kc.restrict_cases():
        _restrict(pool, case)


def test_restrict_beyond_one_pass_of_the_grid(pool, nt):
    cus = pool.e.num_cus
    case = kc.restrict_wrap(cus)
    assert case.step["coarse_rows"] > kc.grid_cap(cus) * kc.BLOCK
    _restrict(pool, case)


# ---- prolong ---------------------------------------------------------------------------------
def _prolong(pool, n, scales):
    step, e_h, z_h = kc.prolong_case(n)
    plan, e = pool.plan(step), pool.vec(e_h)
    for scale in scales:
        z = pool.vec(z_h)
        rc = hip.spmv_hip_amg_prolong_f64(pool.e.context, plan, float(scale),
                                          e.ptr, z.ptr, None)
        assert rc == 0, (n, scale)
        z.expect(kc.prolong_ref(step, scale, e_h, z_h), ("prolong", n, scale))
    e.unchanged(("prolong", n))


def test_prolong_lengths_and_scales(kexec, nt):
    for n in kc.STREAM_SIZES:
        pool = Pool(kexec)
        try:
            _prolong(pool, n, kc.SCALES)
        finally:
            pool.close()


def test_prolong_beyond_one_pass_of_the_grid(pool, nt):
    cus = pool.e.num_cus
    n = kc.stream_wrap(cus)
    assert n // 2 > kc.grid_cap(cus) * kc.UNIT
    _prolong(pool, n, (1.6,))


def test_prolong_refuses_unaligned_and_null(pool, nt):
    step, e_h, z_h = kc.prolong_case(2049)
    ctx, plan = pool.e.context, pool.plan(step)
    e, z, z1 = pool.vec(e_h), pool.vec(z_h), pool.vec(z_h, off=1)
    assert hip.spmv_hip_amg_prolong_f64(ctx, plan, 1.0, e.ptr, z1.ptr,
                                        None) == EINVAL
    assert hip.spmv_hip_amg_prolong_f64(ctx, plan, 1.0, None, z.ptr,
                                        None) == EINVAL
    assert hip.spmv_hip_amg_prolong_f64(ctx, plan, 1.0, e.ptr, None,
                                        None) == EINVAL
    assert hip.spmv_hip_amg_prolong_f64(ctx, None, 1.0, e.ptr, z.ptr,
                                        None) == EINVAL
    pool.e.synchronize()
    for v in (e, z, z1):
        v.unchanged("refused prolong")


# ---- post0 -----------------------------------------------------------------------------------
def _post0(pool, n, b0s):
    w_h, r_h, dinv_h, z_h = kc.post0_case(n)
    w, r, dinv = pool.vec(w_h), pool.vec(r_h), pool.vec(dinv_h)
    for b0 in b0s:
        want_d, want_z = kc.post0_ref(b0, w_h, r_h, dinv_h, z_h)
        for with_d in (True, False):
            z, d = pool.vec(z_h), pool.out(n)
            rc = hip.spmv_hip_amg_post0_f64(pool.e.context, n, float(b0), w.ptr,
                                            r.ptr, dinv.ptr,
                                            d.ptr if with_d else None, z.ptr,
                                            None)
            what = ("post0", n, b0, with_d)
            assert rc == 0, what
            z.expect(want_z, what)
            if with_d:
                d.expect(want_d, (what, "d"))
            else:
                d.unchanged(what)
    for v in (w, r, dinv):
        v.unchanged(("post0", n))


def test_post0_lengths_and_scales(kexec, nt):
    for n in kc.STREAM_SIZES:
        pool = Pool(kexec)
        try:
            _post0(pool, n, kc.SCALES)
        finally:
            pool.close()


def test_post0_beyond_one_pass_of_the_grid(pool, nt):
    cus = pool.e.num_cus
    n = kc.stream_wrap(cus)
    assert n // 2 > kc.grid_cap(cus) * kc.UNIT
    _post0(pool, n, (1.6,))


def test_post0_refuses_unaligned_and_null(pool, nt):
    n = 2049
    ctx = pool.e.context
    w_h, r_h, dinv_h, z_h = kc.post0_case(n)
    w, r, dinv, z = (pool.vec(a) for a in (w_h, r_h, dinv_h, z_h))
    d, z1 = pool.out(n), pool.vec(z_h, off=1)
    f = hip.spmv_hip_amg_post0_f64
    assert f(ctx, n, 1.0, None, r.ptr, dinv.ptr, d.ptr, z.ptr, None) == EINVAL
    assert f(ctx, n, 1.0, w.ptr, None, dinv.ptr, d.ptr, z.ptr, None) == EINVAL
    assert f(ctx, n, 1.0, w.ptr, r.ptr, None, d.ptr, z.ptr, None) == EINVAL
    assert f(ctx, n, 1.0, w.ptr, r.ptr, dinv.ptr, d.ptr, None, None) == EINVAL
    assert f(ctx, n, 1.0, w.ptr, r.ptr, dinv.ptr, d.ptr, z1.ptr, None) == EINVAL
    assert f(ctx, -1, 1.0, w.ptr, r.ptr, dinv.ptr, d.ptr, z.ptr, None) == EINVAL
    pool.e.synchronize()
    for v in (w, r, dinv, z, z1, d):
        v.unchanged("refused post0")
