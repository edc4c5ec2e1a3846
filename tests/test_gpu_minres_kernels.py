"""Every kernel of blas1_minres.hip launched ALONE through the C ABI, cached and
non-temporal (blas1_nt_min_elems), against the references of minres_cases.py.

Vectors lie between guard words (test_gpu_gmres_kernels.Guarded); inputs must
come back unchanged, write-only buffers start as the sentinel.  Lengths:
blas1_cases.small_lengths() on sets E and R and blas1_cases.wrap_lengths
(dot_blocks) on set E.

  init, update_r (with a dinv, without one, state k == 0; alfa from its
      partials and from the reducer's slot), update_xwv (k == 0, a regular
      step, the last step, a step the state does not match): equality of bits
  the dot products of init and update_r + reduce: set E equality of bits; set R
      inside blas1_cases.sum_bound(blas1_cases.depth(n, dot_blocks))
  start, step: equality of bits with their restatements, driven with chosen
      scalars through every branch"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import minres_cases as mc
from spmv_amd import hip
from test_gpu_gmres_kernels import (Guarded, L, nt, peek, poke, vec,  # noqa: F401
                                    wraps_fit)

pytestmark = pytest.mark.gpu

SENT = bc.SENTINEL
KMAX = 8
ALFA, RY, HIST, PART_ALFA, PART_RY, SCALARS = range(6)
NAMES = ("rtol", "alfa", "ry", "beta", "oldb", "dbar", "epsln", "phibar", "cs",
         "sn", "bob", "oldeps", "delta", "inv_gamma", "phi", "inv_beta")


class Ws:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call("spmv_hip_minres_ws_create", ctx.h, KMAX, C.byref(self.h))
        self.reset()

    def reset(self, rtol=0.0, kmax=KMAX):
        hip.call("spmv_hip_minres_ws_reset", self.h, float(rtol), kmax, None)

    def addr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        hip.call("spmv_hip_minres_ws_array", self.h, which, C.byref(p),
                 C.byref(n))
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
        hip.call("spmv_hip_minres_ws_set_state", self.h, k, done, None)

    def words(self):
        out = np.zeros(5, np.int32)
        hip.call("spmv_hip_minres_ws_get_state", self.h,
                 out.ctypes.data_as(C.c_void_p), None)
        self.ctx.stream_sync()
        return dict(zip(("done", "kstop", "status", "k", "kmax"),
                        (int(v) for v in out)))

    def close(self):
        hip.call("spmv_hip_minres_ws_destroy", self.h)


@pytest.fixture(scope="module")
def ws(ctx):
    w = Ws(ctx)
    yield w
    w.close()


def call(name, *a):
    hip.call("spmv_hip_minres_" + name, *a)


def cases(L):
    out = [(n, kind) for n in bc.small_lengths() if n for kind in ("E", "R")]
    if wraps_fit(L):
        out += [(n, "E") for n in bc.wrap_lengths(L)]
    return out


_EXACT = {}


def check_dot(got, a, b, kind, n, L, what):
    if kind == "E":
        assert float(got) == float(bc.exact_dot_int(a, b)), what
    else:  # (exact rational sums are slow: once for both instantiations)
        if what not in _EXACT:
            _EXACT[what] = bc.exact_dot(a, b)
        ex, sa = _EXACT[what]
        assert bc.sum_within(got, ex, sa, bc.depth(n, L)), what


def test_init_and_update_r(ctx, ws, L, nt):
    for n, kind in cases(L):
        g = bc.stream_grid(n // 2, L)
        Av, r1v, r2v = (vec(kind, n, s) for s in (1, 2, 3))
        dv = vec("d" + kind, n, 0)
        # E: coefficients that keep every entry an integer
        alfa, beta, bob = (6.0, 2.0, 2.0) if kind == "E" else (
            0.8414709848, 1.6487212707, 0.3678794412)
        src = Guarded(ctx, [Av, r2v, dv], n)
        for dinv in (None, dv):
            what = (n, kind, dinv is not None)
            d_ptr = src.row(2) if dinv is not None else None
            y = Guarded(ctx, [np.full(n, SENT)], n)
            # -- init: y = dinv * r2, partials of r2.y
            ws.reset()
            ws.set(PART_RY, np.full(L, SENT))
            call("init_f64", ctx.h, ws.h, n, src.row(1), d_ptr,
                 y.ptr if dinv is not None else None, None)
            y0 = mc.minres_init(r2v, dinv)
            src.check(what)
            y.check(what, **({"r0": y0} if dinv is not None else {}))
            assert np.all(ws.get(PART_RY)[g:] == 0), what
            call("reduce", ctx.h, ws.h, RY, None, None)
            # (set E with a dinv: r2 * (dinv * r2) stays an integer)
            check_dot(ws.get(RY)[0], r2v, y0, kind, n, L, what + ("init",))
            # -- update_r: regular step and the first one; alfa from the
            #    partials (the sum of one nonzero entry is that entry) and
            #    from the slot
            # (a wrap length: one combination per preconditioner -- the trips
            # of the loop do not depend on where alfa comes from)
            small = n <= 2 * bc.UNIT + 1
            for first, reduced in (((False, 0), (False, 1), (True, 0), (True, 1))
                                   if small else ((dinv is None, 0),)):
                if True:
                    r1 = Guarded(ctx, [r1v], n)
                    poke(ctx, y.ptr, np.full(n, SENT))
                    ws.reset()
                    ws.install(beta=beta, bob=bob,
                               alfa=alfa if reduced else SENT)
                    part = np.zeros(L)
                    part[min(3, L - 1)] = SENT if reduced else alfa
                    ws.set(PART_ALFA, part)
                    ws.set(PART_RY, np.full(L, SENT))
                    ws.state(k=0 if first else 3)
                    call("update_r_f64", ctx.h, ws.h, n, src.row(0), r1.ptr,
                         src.row(1), d_ptr, y.ptr if dinv is not None else None,
                         reduced, None, 1, None)
                    t, yy = mc.minres_update_r(Av, r1v, r2v, dinv, alfa, beta,
                                               bob, first)
                    w2 = what + (first, reduced)
                    src.check(w2), r1.check(w2, r0=t)
                    y.check(w2, **({"r0": yy} if dinv is not None else {}))
                    assert ws.scalars()["alfa"] == alfa, w2
                    assert np.all(ws.get(PART_RY)[g:] == 0), w2
                    call("reduce", ctx.h, ws.h, RY, None, None)
                    check_dot(ws.get(RY)[0], t, yy, kind, n, L, w2)
                    r1.free()
            # -- without the dot (a preconditioner of its own follows): the
            #    partials stay; after `done`: nothing moves
            r1 = Guarded(ctx, [r1v], n)
            ws.reset()
            ws.install(beta=beta, bob=bob, alfa=alfa)
            ws.set(PART_RY, np.full(L, SENT))
            ws.state(k=2)
            call("update_r_f64", ctx.h, ws.h, n, src.row(0), r1.ptr, src.row(1),
                 None, None, 1, None, 0, None)
            t, _ = mc.minres_update_r(Av, r1v, r2v, None, alfa, beta, bob, False)
            r1.check(what, r0=t)
            assert np.all(ws.get(PART_RY) == SENT), what
            ws.state(k=2, done=1)
            call("update_r_f64", ctx.h, ws.h, n, src.row(0), r1.ptr, src.row(1),
                 None, None, 1, None, 1, None)
            call("init_f64", ctx.h, ws.h, n, src.row(1), None, None, None)
            call("reduce", ctx.h, ws.h, RY, None, None)
            r1.check(what, r0=t, final=True)
            assert np.all(ws.get(PART_RY) == SENT), what
            assert ws.scalars()["ry"] == 0.0, what
            r1.free(), y.free()
        src.check((n, kind), final=True)
        src.free()


def test_update_xwv(ctx, ws, L, nt):
    for n, kind in cases(L):
        what = (n, kind)
        vv, w1v, w2v, xv, yv = (vec(kind, n, s) for s in (4, 5, 6, 7, 8))
        co = dict(oldeps=2.0, delta=-1.0, inv_gamma=0.5, phi=4.0, inv_beta=0.25) \
            if kind == "E" else dict(oldeps=0.5403023059, delta=-1.4142135624,
                                     inv_gamma=0.7310585786, phi=-0.3183098862,
                                     inv_beta=1.2020569032)
        ro = Guarded(ctx, [w2v, yv], n)

        def run(k_arg, k_state, done):
            bufs = Guarded(ctx, [vv, w1v, xv], n)
            ws.reset()
            ws.install(**co)
            ws.state(k=k_state, done=done)
            before = ws.get(SCALARS)
            call("update_xwv_f64", ctx.h, ws.h, k_arg, n, bufs.row(0),
                 bufs.row(1), ro.row(0), bufs.row(2), ro.row(1), None)
            assert bc.same_bits(ws.get(SCALARS), before), what
            ro.check(what)
            return bufs

        # a regular step
        w, x, v = mc.minres_update_xwv(vv, w1v, w2v, xv, yv, **co)
        b = run(3, 3, 0)
        b.check(what + ("regular",), r0=v, r1=w, r2=x, final=True)
        b.free()
        # the step that stopped: x and w move, v stays
        b = run(3, 3, 1)
        b.check(what + ("last",), r0=vv, r1=w, r2=x, final=True)
        b.free()
        # k == 0: v alone
        b = run(0, 0, 0)
        b.check(what + ("k = 0",), r0=mc.minres_scale(yv, co["inv_beta"]),
                final=True)
        b.free()
        # the state's k is not the launch's (a step that stopped without an
        # iterate, or a launch behind the stop), and k == 0 after `done`
        for k_arg, k_state, done in ((4, 3, 1), (4, 3, 0), (2, 3, 0), (0, 0, 1),
                                     (0, 2, 0)):
            b = run(k_arg, k_state, done)
            b.check(what + ("no-op", k_arg, k_state, done), final=True)
            b.free()
        ro.check(what, final=True)
        ro.free()


# ---- the scalar kernels -----------------------------------------------------------
def _state_of(sc):
    return {key: sc[key] for key in mc.STATE}


def test_start_every_branch(ctx, ws):
    for ry in (12.25, 2.0, 0.0, -1.0, 1e-300, float("nan")):
        ws.reset(rtol=1e-10)
        ws.set(HIST, np.full(KMAX + 1, SENT))
        ws.install(ry=ry)
        call("start", ctx.h, ws.h, None)
        want = mc.minres_start(ry)
        sc, wd, hist = ws.scalars(), ws.words(), ws.get(HIST)
        what = ("start", ry)
        assert wd["done"] == int(want["done"]), what
        assert wd["status"] == want["status"] and wd["k"] == 0, what
        assert wd["kstop"] == (0 if want["done"] else -1), what
        if want["hist0"] is None:
            assert hist[0] == SENT, what
        else:
            assert bc.same_bits([hist[0]], [want["hist0"]]), what
        assert np.all(hist[1:] == SENT), what
        if not want["done"]:
            for key in mc.STATE + ("inv_beta",):
                assert bc.same_bits([sc[key]], [want[key]]), (what, key)
    # after `done`: nothing moves
    ws.reset()
    ws.install(ry=4.0)
    ws.state(k=2, done=1)
    before = ws.get(SCALARS)
    call("start", ctx.h, ws.h, None)
    assert bc.same_bits(ws.get(SCALARS), before)
    assert ws.get(HIST)[0] == 0.0


# (name, state in front, alfa, ry, k, kmax, rtol, hist0) -> every branch
_FIRST = mc.minres_start(12.25)
_MID = dict(beta=1.7320508076, oldb=0.9, dbar=-0.6180339887, epsln=0.4142135624,
            phibar=0.0314159265, cs=0.8660254038, sn=0.5)
STEPS = [
    ("the first step", _state_of(_FIRST), 0.75, 2.25, 0, KMAX, 1e-10, 3.5),
    ("a regular step", _MID, -1.25, 0.81, 3, KMAX, 1e-10, 3.5),
    ("ry < 0", _MID, -1.25, -1e-30, 3, KMAX, 1e-10, 3.5),
    ("gamma == 0", dict(_MID, dbar=0.0), 0.0, 0.0, 3, KMAX, 1e-10, 3.5),
    ("beta == 0", _MID, -1.25, 0.0, 3, KMAX, 1e-10, 3.5),
    ("the stop", _MID, -1.25, 0.81, 3, KMAX, 0.5, 3.5),
    ("k == kmax", _MID, -1.25, 0.81, 3, 4, 1e-10, 3.5),
    ("NaN goes on", _MID, float("nan"), 0.81, 3, KMAX, 1e-10, 3.5),
    ("NaN ends at kmax", _MID, float("nan"), 0.81, 3, 4, 1e-10, 3.5),
]


@pytest.mark.parametrize("case", STEPS, ids=[c[0] for c in STEPS])
def test_step_every_branch(ctx, ws, case):
    name, st, alfa, ry, k, kmax, rtol, hist0 = case
    ws.reset(rtol=rtol, kmax=kmax)
    hist_in = np.full(KMAX + 1, SENT)
    hist_in[0] = hist0
    ws.set(HIST, hist_in)
    ws.install(alfa=alfa, ry=ry, **{key: SENT for key in mc.COEFS}, **st)
    ws.state(k=k)
    before = ws.scalars()
    call("step", ctx.h, ws.h, None)
    want = mc.minres_step(st, alfa, ry, hist0, k, kmax, rtol)
    sc, wd, hist = ws.scalars(), ws.words(), ws.get(HIST)
    print(name, want)
    assert wd["done"] == int(want["done"]) and wd["k"] == want["k"], name
    assert wd["status"] == want["status"], name
    assert wd["kstop"] == (want["k"] if want["done"] else -1), name
    hist_want = hist_in.copy()
    if want["res"] is not None:
        hist_want[k + 1] = want["res"]
    if want["res"] is not None and math.isnan(want["res"]):
        assert math.isnan(hist[k + 1]), name
        hist_want[k + 1] = hist[k + 1]
    assert bc.same_bits(hist, hist_want), name
    for key in NAMES[3:]:
        # what the restatement did not reach keeps its bits
        ref = want.get(key, before[key])
        # (a NaN's sign and payload are not the recurrence's business)
        assert (math.isnan(ref) and math.isnan(sc[key])) \
            or bc.same_bits([sc[key]], [ref]), (name, key)
    assert {"ry < 0": 2, "gamma == 0": 3, "beta == 0": 1}.get(name, 0) \
        == want["status"]
    assert want["done"] == (name not in ("the first step", "a regular step",
                                         "NaN goes on"))
    if name.startswith("NaN"):
        assert math.isnan(want["res"]) and want["status"] == 0


def test_step_after_done_and_bad_arguments(ctx, ws):
    ws.reset()
    ws.install(alfa=1.0, ry=1.0, **_MID)
    ws.state(k=2, done=1)
    before = ws.get(SCALARS)
    call("step", ctx.h, ws.h, None)
    assert bc.same_bits(ws.get(SCALARS), before)
    assert ws.words() == dict(done=1, kstop=2, status=0, k=2, kmax=KMAX)
    assert np.all(ws.get(HIST) == 0.0)
    from spmv_amd._lib import SpmvHipError
    buf = ctx.empty(8, np.float64)
    p = buf.at(0)
    for name, args in (
            ("update_xwv_f64", (ctx.h, ws.h, KMAX + 1, 4, p, p, p, p, p, None)),
            ("update_xwv_f64", (ctx.h, ws.h, 1, 4, p, p, p, p, p, None)),  # w1 == w2
            ("update_xwv_f64", (ctx.h, ws.h, 1, 4, p + 8, p, p, p, p, None)),
            ("update_r_f64", (ctx.h, ws.h, 4, p, p, p, None, None, 1, None, 1,
                              None)),  # r1 == r2
            ("reduce", (ctx.h, ws.h, 7, None, None)),
            ("reduce", (ctx.h, ws.h, RY, p, None)),
            ("ws_reset", (ws.h, 0.0, KMAX + 1, None))):
        with pytest.raises(SpmvHipError):
            call(name, *args)
    buf.free()
