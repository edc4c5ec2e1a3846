"""Every kernel of blas1_lsqr.hip launched ALONE through the C ABI, cached and
non-temporal (blas1_nt_min_elems), at 16-byte aligned and at 8-byte-offset
addresses, against the references of lsqr_cases.py.

Vectors lie between guard words (test_gpu_gmres_kernels.Guarded; the offset
vectors start one word into their row, that word is a guard too); inputs must
come back unchanged.  Lengths: 1, 63, 64, 65, 255, 256, 257, 1023, 1025 and
blas1_cases.small_lengths() (the edges of a workgroup's trip) on sets E and R,
and blas1_cases.wrap_lengths(dot_blocks), the first lengths at which the
grid-stride loop wraps, on set E.

  update_u, update_v (regular and first; uu from its partials and from the
      reducer's slot; beta == 0), update_xw (k == 0, a regular step, the last
      step, a step the state does not match): equality of bits
  the dot products of update_u and update_v + reduce: set E equality of bits;
      set R inside blas1_cases.sum_bound(blas1_cases.depth(n, dot_blocks))
  start, step: equality of bits with their restatements, driven with chosen
      scalars through every branch, vv from the slot and from the partials"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import lsqr_cases as lc
from spmv_amd import hip
from test_gpu_gmres_kernels import (Guarded, L, nt, peek, poke, vec,  # noqa: F401
                                    wraps_fit)

pytestmark = pytest.mark.gpu

SENT = bc.SENTINEL
KMAX = 8
UU, VV, HIST_R, HIST_AR, PART_UU, PART_VV, SCALARS = range(7)
NAMES = ("rtol", "ltol", "damp", "uu", "vv", "alpha", "beta", "phibar",
         "rhobar", "anorm2", "psi2", "ia", "ib", "t1", "t2")
EXTRA = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)


class Ws:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call("spmv_hip_lsqr_ws_create", ctx.h, KMAX, C.byref(self.h))
        self.reset()

    def reset(self, rtol=0.0, ltol=0.0, damp=0.0, kmax=KMAX):
        hip.call("spmv_hip_lsqr_ws_reset", self.h, float(rtol), float(ltol),
                 float(damp), kmax, None)

    def addr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        hip.call("spmv_hip_lsqr_ws_array", self.h, which, C.byref(p), C.byref(n))
        return p.value, n.value

    def set(self, which, values, at=0):
        poke(self.ctx, self.addr(which)[0] + 8 * at, values)

    def get(self, which):
        p, n = self.addr(which)
        return peek(self.ctx, p, n)

    def scalars(self):
        return dict(zip(NAMES, (float(v) for v in self.get(SCALARS))))

    def install(self, **kw):
        cur = self.get(SCALARS)
        for key, v in kw.items():
            cur[NAMES.index(key)] = v
        self.set(SCALARS, cur)

    def state(self, k=0, done=0):
        hip.call("spmv_hip_lsqr_ws_set_state", self.h, k, done, None)

    def words(self):
        out = np.zeros(5, np.int32)
        hip.call("spmv_hip_lsqr_ws_get_state", self.h,
                 out.ctypes.data_as(C.c_void_p), None)
        self.ctx.stream_sync()
        return dict(zip(("done", "kstop", "status", "k", "kmax"),
                        (int(v) for v in out)))

    def close(self):
        hip.call("spmv_hip_lsqr_ws_destroy", self.h)


@pytest.fixture(scope="module")
def ws(ctx):
    w = Ws(ctx)
    yield w
    w.close()


@pytest.fixture(params=[0, 1], ids=["aligned", "offset8"])
def off(request):
    return request.param


def call(name, *a):
    hip.call("spmv_hip_lsqr_" + name, *a)


class Vecs:
    """Guarded vectors of n doubles that start `off` words into their rows"""

    def __init__(self, ctx, rows, n, off):
        self.off, self.n = off, n
        pad = [np.concatenate([np.full(off, SENT), r]) for r in rows]
        self.g = Guarded(ctx, pad, n + off)

    def ptr(self, i):
        return self.g.row(i) + 8 * self.off

    def check(self, what, final=False, **rows):
        self.g.check(what, final=final, **{
            key: np.concatenate([np.full(self.off, SENT), r])
            for key, r in rows.items()})

    def free(self):
        self.g.free()


def cases(L):
    small = sorted(set(EXTRA) | {n for n in bc.small_lengths() if n})
    out = [(n, kind) for n in small for kind in ("E", "R")]
    if wraps_fit(L):
        out += [(n, "E") for n in bc.wrap_lengths(L)]
    return out


_EXACT = {}


def check_dot(got, a, kind, n, L, what):
    if kind == "E":
        assert float(got) == float(bc.exact_dot_int(a, a)), what
    else:  # (exact rational sums are slow: once for all instantiations)
        if what not in _EXACT:
            _EXACT[what] = bc.exact_dot(a, a)
        ex, sa = _EXACT[what]
        assert bc.sum_within(got, ex, sa, bc.depth(n, L)), what


def test_update_u(ctx, ws, L, nt, off):
    for n, kind in cases(L):
        what = ("update_u", n, kind)
        g = bc.stream_grid(n // 2, L)
        Av, utv = vec(kind, n, 1), vec(kind, n, 2)
        # E: coefficients that keep every entry an integer
        co = dict(ia=2.0, alpha=3.0, ib=1.0) if kind == "E" else dict(
            ia=0.8414709848, alpha=1.6487212707, ib=0.3678794412)
        src = Vecs(ctx, [Av], n, off)
        ut = Vecs(ctx, [utv], n, off)
        ws.reset()
        ws.install(**co)
        ws.set(PART_UU, np.full(L, SENT))
        before = ws.get(SCALARS)
        call("update_u_f64", ctx.h, ws.h, n, src.ptr(0), ut.ptr(0), None)
        t = lc.lsqr_update_u(Av, utv, **co)
        src.check(what, final=True), ut.check(what, r0=t)
        assert bc.same_bits(ws.get(SCALARS), before), what
        assert np.all(ws.get(PART_UU)[g:] == 0), what
        call("reduce", ctx.h, ws.h, UU, None)
        check_dot(ws.get(UU)[0], t, kind, n, L, what)
        # after `done`: nothing moves
        ws.set(PART_UU, np.full(L, SENT))
        ws.state(k=2, done=1)
        call("update_u_f64", ctx.h, ws.h, n, src.ptr(0), ut.ptr(0), None)
        call("reduce", ctx.h, ws.h, UU, None)
        ut.check(what, r0=t, final=True)
        assert np.all(ws.get(PART_UU) == SENT), what
        src.free(), ut.free()


def test_update_v(ctx, ws, L, nt, off):
    for n, kind in cases(L):
        g = bc.stream_grid(n // 2, L)
        Atu, vtv = vec(kind, n, 3), vec(kind, n, 4)
        # E: beta = 0.5, 1 / beta = 2, ia = 2: vn = 2 Atu - vt stays an integer
        uu, ia = (0.25, 2.0) if kind == "E" else (2.7182818285, 0.5772156649)
        src = Vecs(ctx, [Atu], n, off)
        # (a wrap length: one combination -- the trips of the loop do not depend
        # on where uu comes from)
        small = n <= 2 * bc.UNIT + 1
        for first, reduced in (((0, 0), (0, 1), (1, 0), (1, 1)) if small
                               else ((0, 0),)):
            what = ("update_v", n, kind, first, reduced)
            vt = Vecs(ctx, [vtv], n, off)
            ws.reset()
            ws.install(ia=ia, uu=uu if reduced else SENT)
            part = np.zeros(L)
            part[min(3, L - 1)] = SENT if reduced else uu
            ws.set(PART_UU, part)
            ws.set(PART_VV, np.full(L, SENT))
            call("update_v_f64", ctx.h, ws.h, n, src.ptr(0), vt.ptr(0), first,
                 reduced, None)
            t = lc.lsqr_update_v(Atu, vtv, uu, ia, first=bool(first))
            src.check(what), vt.check(what, r0=t, final=True)
            assert ws.scalars()["uu"] == uu, what
            assert np.all(ws.get(PART_VV)[g:] == 0), what
            call("reduce", ctx.h, ws.h, VV, None)
            check_dot(ws.get(VV)[0], t, kind, n, L, what[:3] + (first,))
            vt.free()
        if small:
            # beta == 0: vt stays, the partials are zero; after `done`: nothing
            vt = Vecs(ctx, [vtv], n, off)
            what = ("update_v", n, kind, "beta == 0")
            ws.reset()
            ws.install(ia=ia)
            ws.set(PART_UU, np.zeros(L))
            ws.set(PART_VV, np.full(L, SENT))
            call("update_v_f64", ctx.h, ws.h, n, src.ptr(0), vt.ptr(0), 0, 0, None)
            assert lc.lsqr_update_v(Atu, vtv, 0.0, ia) is None
            vt.check(what)
            assert np.all(ws.get(PART_VV) == 0), what
            ws.set(PART_UU, np.full(L, 1.0))
            ws.set(PART_VV, np.full(L, SENT))
            ws.state(k=2, done=1)
            call("update_v_f64", ctx.h, ws.h, n, src.ptr(0), vt.ptr(0), 0, 0, None)
            call("reduce", ctx.h, ws.h, VV, None)
            vt.check(what, final=True)
            assert np.all(ws.get(PART_VV) == SENT), what
            assert ws.scalars()["vv"] == 0.0 and ws.scalars()["uu"] == 0.0, what
            vt.free()
        src.check((n, kind), final=True)
        src.free()


def test_update_xw(ctx, ws, L, nt, off):
    for n, kind in cases(L):
        what = ("update_xw", n, kind)
        vtv, wv, xv = (vec(kind, n, s) for s in (5, 6, 7))
        co = dict(t1=4.0, t2=-2.0, ia=0.5) if kind == "E" else dict(
            t1=-0.3183098862, t2=1.4142135624, ia=0.7310585786)
        ro = Vecs(ctx, [vtv], n, off)

        def run(k_arg, k_state, done):
            bufs = Vecs(ctx, [wv, xv], n, off)
            ws.reset()
            ws.install(**co)
            ws.state(k=k_state, done=done)
            before = ws.get(SCALARS)
            call("update_xw_f64", ctx.h, ws.h, k_arg, n, ro.ptr(0), bufs.ptr(0),
                 bufs.ptr(1), None)
            assert bc.same_bits(ws.get(SCALARS), before), what
            ro.check(what)
            return bufs

        # a regular step
        x, w = lc.lsqr_update_xw(vtv, wv, xv, **co)
        b = run(3, 3, 0)
        b.check(what + ("regular",), r0=w, r1=x, final=True)
        b.free()
        if n > 2 * bc.UNIT + 1:  # (a wrap length: the trips are the same)
            ro.check(what, final=True)
            ro.free()
            continue
        # the step that stopped: x moves, w stays
        b = run(3, 3, 1)
        b.check(what + ("last",), r0=wv, r1=x, final=True)
        b.free()
        # k == 0: w alone
        b = run(0, 0, 0)
        b.check(what + ("k = 0",), r0=lc.lsqr_scale(vtv, co["ia"]), final=True)
        b.free()
        # the state's k is not the launch's (k is behind, or a launch behind the
        # stop), and k == 0 after `done`
        for k_arg, k_state, done in ((4, 3, 1), (4, 3, 0), (2, 3, 0), (0, 0, 1),
                                     (0, 2, 0)):
            b = run(k_arg, k_state, done)
            b.check(what + ("no-op", k_arg, k_state, done), final=True)
            b.free()
        ro.check(what, final=True)
        ro.free()


# ---- the scalar kernels -----------------------------------------------------------
def _feed_vv(ws, L, vv, reduced):
    """vv in the slot, or as three partials whose sum is exact"""
    part = np.full(L, SENT if reduced else 0.0)
    if not reduced:
        part[0] = part[min(5, L - 1)] = 0.25 * vv
        part[L - 1] += 0.5 * vv
    ws.set(PART_VV, part)
    ws.install(vv=vv if reduced else SENT)


@pytest.mark.parametrize("reduced", [0, 1])
def test_start_every_branch(ctx, ws, L, reduced):
    for uu, vv in ((12.25, 2.0), (2.0, 6.25), (0.0, 3.0), (4.0, 0.0),
                   (1e-300, 1e-300), (float("nan"), 1.0), (1.0, float("nan"))):
        ws.reset(rtol=1e-10)
        ws.set(HIST_R, np.full(KMAX + 1, SENT))
        ws.set(HIST_AR, np.full(KMAX + 1, SENT))
        ws.install(uu=uu)
        _feed_vv(ws, L, vv, reduced)
        call("start", ctx.h, ws.h, reduced, None)
        want = lc.lsqr_start(uu, vv)
        sc, wd = ws.scalars(), ws.words()
        hist_r, hist_ar = ws.get(HIST_R), ws.get(HIST_AR)
        what = ("start", uu, vv)
        assert wd["done"] == int(want["done"]), what
        assert wd["status"] == want["status"] and wd["k"] == 0, what
        assert wd["kstop"] == (0 if want["done"] else -1), what
        for got, ref in ((hist_r[0], want["hist_r0"]), (hist_ar[0],
                                                        want["hist_ar0"])):
            ref = SENT if ref is None else ref
            assert (math.isnan(ref) and math.isnan(got)) \
                or bc.same_bits([got], [ref]), what
        assert np.all(hist_r[1:] == SENT) and np.all(hist_ar[1:] == SENT), what
        if not want["done"]:
            for key in lc.STATE + ("ia", "ib"):
                assert (math.isnan(want[key]) and math.isnan(sc[key])) \
                    or bc.same_bits([sc[key]], [want[key]]), (what, key)
    # after `done`: nothing moves
    ws.reset()
    ws.install(uu=4.0, vv=4.0)
    ws.state(k=2, done=1)
    before = ws.get(SCALARS)
    call("start", ctx.h, ws.h, 1, None)
    assert bc.same_bits(ws.get(SCALARS), before)
    assert ws.get(HIST_R)[0] == 0.0 and ws.get(HIST_AR)[0] == 0.0


# (name, state in front, uu, vv, k, kmax, rtol, ltol, damp, hist0)
_FIRST = lc.lsqr_start(12.25, 2.0)
_MID = dict(alpha=1.7320508076, beta=0.9, phibar=0.0314159265,
            rhobar=-0.6180339887, anorm2=14.1421356237, psi2=0.0)
_MIDD = dict(_MID, psi2=0.0002718282)
STEPS = [
    ("the first step", {k: _FIRST[k] for k in lc.STATE}, 2.25, 0.75, 0, KMAX,
     1e-10, 1e-10, 0.0, 3.5),
    ("a regular step", _MID, 0.81, 1.25, 3, KMAX, 1e-10, 1e-10, 0.0, 3.5),
    ("a damped step", _MIDD, 0.81, 1.25, 3, KMAX, 1e-10, 1e-10, 0.5, 3.5),
    ("beta == 0", _MID, 0.0, 1.25, 3, KMAX, 1e-10, 1e-10, 0.0, 3.5),
    ("beta == 0, damped", _MIDD, 0.0, 1.25, 3, KMAX, 1e-10, 1e-10, 0.5, 3.5),
    ("alpha_n == 0", _MID, 0.81, 0.0, 3, KMAX, 1e-10, 1e-10, 0.0, 3.5),
    ("the rtol stop", _MID, 0.81, 1.25, 3, KMAX, 0.5, 0.0, 0.0, 3.5),
    ("the ltol stop", _MID, 0.81, 1.25, 3, KMAX, 0.0, 0.5, 0.0, 3.5),
    ("the ltol stop, damped", _MIDD, 0.81, 1.25, 3, KMAX, 0.0, 0.5, 0.5, 3.5),
    ("rtol before ltol", _MID, 0.81, 1.25, 3, KMAX, 0.5, 0.5, 0.0, 3.5),
    ("k == kmax", _MID, 0.81, 1.25, 3, 4, 1e-10, 1e-10, 0.0, 3.5),
    ("NaN goes on", _MID, float("nan"), 1.25, 3, KMAX, 1e-10, 1e-10, 0.0, 3.5),
    ("NaN ends at kmax", _MID, 0.81, float("nan"), 3, 4, 1e-10, 1e-10, 0.0, 3.5),
]
_STATUS = {"beta == 0": 2, "beta == 0, damped": 2, "alpha_n == 0": 2,
           "the ltol stop": 1, "the ltol stop, damped": 1}
_GO_ON = ("the first step", "a regular step", "a damped step", "NaN goes on")


@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("case", STEPS, ids=[c[0] for c in STEPS])
def test_step_every_branch(ctx, ws, L, case, reduced):
    name, st, uu, vv, k, kmax, rtol, ltol, damp, hist0 = case
    ws.reset(rtol=rtol, ltol=ltol, damp=damp, kmax=kmax)
    hist_in = np.full(KMAX + 1, SENT)
    hist_in[0] = hist0
    ws.set(HIST_R, hist_in)
    ws.set(HIST_AR, np.full(KMAX + 1, SENT))
    ws.install(uu=uu, **{key: SENT for key in lc.COEFS}, **st)
    _feed_vv(ws, L, vv, reduced)
    ws.state(k=k)
    before = ws.scalars()
    call("step", ctx.h, ws.h, reduced, None)
    want = lc.lsqr_step(st, uu, vv, hist0, k, kmax, rtol, ltol, damp)
    sc, wd = ws.scalars(), ws.words()
    hist_r, hist_ar = ws.get(HIST_R), ws.get(HIST_AR)
    print(name, want)
    assert wd["done"] == int(want["done"]) and wd["k"] == want["k"] == k + 1, name
    assert wd["status"] == want["status"], name
    assert wd["kstop"] == (want["k"] if want["done"] else -1), name
    for got, ref, first in ((hist_r, want["res"], hist0), (hist_ar, want["ares"],
                                                           SENT)):
        full = np.full(KMAX + 1, SENT)
        full[0] = first
        full[k + 1] = got[k + 1] if math.isnan(ref) else ref
        assert not math.isnan(ref) or math.isnan(got[k + 1]), name
        assert bc.same_bits(got, full), name
    assert bc.same_bits([sc["vv"]], [vv]) or math.isnan(vv), name
    for key in NAMES[5:]:
        # what the restatement did not reach keeps its bits
        ref = want.get(key, before[key])
        # (a NaN's sign and payload are not the recurrence's business)
        assert (math.isnan(ref) and math.isnan(sc[key])) \
            or bc.same_bits([sc[key]], [ref]), (name, key)
    assert _STATUS.get(name, 0) == want["status"]
    assert want["done"] == (name not in _GO_ON)
    if name.startswith("NaN"):  # (uu: through beta into res; vv: into ares)
        assert math.isnan(want["res"] if math.isnan(uu) else want["ares"])
        assert want["status"] == 0
    if "damped" in name:
        assert want["psi2"] > st["psi2"]


def test_step_after_done_and_bad_arguments(ctx, ws):
    ws.reset()
    ws.install(uu=1.0, vv=1.0, **_MID)
    ws.state(k=2, done=1)
    before = ws.get(SCALARS)
    call("step", ctx.h, ws.h, 1, None)
    call("step", ctx.h, ws.h, 0, None)
    assert bc.same_bits(ws.get(SCALARS), before)
    assert ws.words() == dict(done=1, kstop=2, status=0, k=2, kmax=KMAX)
    assert np.all(ws.get(HIST_R) == 0.0) and np.all(ws.get(HIST_AR) == 0.0)
    # a step at k == kmax has no room in the histories: it stops, nothing moves
    ws.reset(kmax=3)
    ws.install(uu=1.0, vv=1.0, **_MID)
    ws.state(k=3)
    call("step", ctx.h, ws.h, 1, None)
    assert ws.words() == dict(done=1, kstop=3, status=0, k=3, kmax=3)
    assert np.all(ws.get(HIST_R) == 0.0)
    from spmv_amd._lib import SpmvHipError
    buf = ctx.empty(16, np.float64)
    p, q, r = buf.at(0), buf.at(4), buf.at(8)
    for name, args in (
            ("update_xw_f64", (ctx.h, ws.h, KMAX + 1, 4, p, q, r, None)),
            ("update_xw_f64", (ctx.h, ws.h, 1, 4, p, p, r, None)),  # w == vt
            ("update_xw_f64", (ctx.h, ws.h, 1, 4, p, q, q, None)),  # x == w
            ("update_xw_f64", (ctx.h, ws.h, 1, 4, p + 4, q, r, None)),
            ("update_u_f64", (ctx.h, ws.h, 4, p, p, None)),  # Av == ut
            ("update_v_f64", (ctx.h, ws.h, 4, p, p, 0, 0, None)),
            ("update_v_f64", (ctx.h, ws.h, -1, p, q, 0, 0, None)),
            ("reduce", (ctx.h, ws.h, 7, None)),
            ("ws_reset", (ws.h, 0.0, 0.0, 0.0, KMAX + 1, None))):
        with pytest.raises(SpmvHipError):
            call(name, *args)
    buf.free()
