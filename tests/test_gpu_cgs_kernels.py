"""Every kernel of blas1_cgshift.hip launched ALONE through the C ABI, cached
and non-temporal (blas1_nt_min_elems), at 16-byte aligned and at 8-byte-offset
addresses, against the references of cgs_cases.py.

Vectors lie between guard words (test_gpu_gmres_kernels.Guarded; the offset
vectors start one word into their row, that word is a guard too); inputs, and
every column of X and PS that is not in the list `upd`, must come back with the
bytes that were uploaded.  Lengths: blas1_cases.small_lengths() (0 included)
and a few odd ones on sets E and R, blas1_cases.wrap_lengths(dot_blocks) on
set E.

  update_r (pq from its partials, with and without a second array, and from
      the slot; pq <= 0, pq NaN, done), update_xp (ns = 1, 2, 3, 5, 8; every
      shift, one shift, a compacted list, none; shifts that stop in this step;
      done; a k the state does not match): equality of bits
  the dot product of update_r + reduce: set E equality of bits; set R inside
      blas1_cases.sum_bound(blas1_cases.depth(n, dot_blocks))
  start, step: the whole device state against the restatement's, bit for bit,
      through both branches of the rtol test, pq <= 0, pq NaN, rrn == 0, kmax,
      rrn from the slot and from the partials"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import cgs_cases as cc
from spmv_amd import hip
from test_gpu_gmres_kernels import (Guarded, L, nt, peek, poke, vec,  # noqa: F401
                                    wraps_fit)

pytestmark = pytest.mark.gpu

SENT = bc.SENTINEL
KMAX = 8
PQ, RRN, HIST, PART_PQ, PART_RRN, SCALARS = range(6)
SINGLES = ("rtol", "pq", "rrn", "rr", "a_old", "b_old", "bn", "hist0")
ARRAYS = ("sigma", "zeta", "rho", "cx", "cp")
WORDS1 = ("done", "kstop", "status")
WORDS2 = ("k", "kmax", "ns", "n_act", "n_upd")
EXTRA = (63, 65, 257, 1023)


class Ws:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call("spmv_hip_cgs_ws_create", ctx.h, KMAX, C.byref(self.h))

    def reset(self, shifts=(0.0,), rtol=0.0, kmax=KMAX):
        sh = np.ascontiguousarray(shifts, np.float64)
        hip.call("spmv_hip_cgs_ws_reset", self.h, float(rtol), kmax, len(sh),
                 sh.ctypes.data_as(C.c_void_p), None)

    def addr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        hip.call("spmv_hip_cgs_ws_array", self.h, which, C.byref(p), C.byref(n))
        return p.value, n.value

    def set(self, which, values):
        poke(self.ctx, self.addr(which)[0], values)

    def get(self, which):
        p, n = self.addr(which)
        return peek(self.ctx, p, n)

    def hist(self):
        return self.get(HIST).reshape(cc.MAX_NS, KMAX + 1)

    def fetch(self):
        """the device state as a cgs_cases state dict"""
        d = self.get(SCALARS)
        st = {k: float(d[i]) for i, k in enumerate(SINGLES)}
        for j, k in enumerate(ARRAYS):
            st[k] = [float(v) for v in d[8 + 8 * j:16 + 8 * j]]
        w = np.zeros(32, np.int32)
        hip.call("spmv_hip_cgs_ws_get_words", self.h,
                 w.ctypes.data_as(C.c_void_p), None)
        self.ctx.stream_sync()
        w = [int(v) for v in w]
        st.update(zip(WORDS1, w[:3]))
        st["its"] = w[3:11]
        st.update(zip(WORDS2, w[11:16]))
        st["act"], st["upd"] = w[16:24], w[24:32]
        return st

    def install(self, st):
        d = [st[k] for k in SINGLES]
        for k in ARRAYS:
            d += list(st[k])
        self.set(SCALARS, np.array(d, np.float64))
        w = [st[k] for k in WORDS1] + list(st["its"]) + [st[k] for k in WORDS2] \
            + list(st["act"]) + list(st["upd"])
        w = np.array(w, np.int32)
        hip.call("spmv_hip_cgs_ws_set_words", self.h,
                 w.ctypes.data_as(C.c_void_p), None)

    def close(self):
        hip.call("spmv_hip_cgs_ws_destroy", self.h)


@pytest.fixture(scope="module")
def ws(ctx):
    w = Ws(ctx)
    yield w
    w.close()


@pytest.fixture(params=[0, 1], ids=["aligned", "offset8"])
def off(request):
    return request.param


def call(name, *a):
    hip.call("spmv_hip_cgs_" + name, *a)


class Vecs:
    """Guarded vectors of n doubles that start `off` words into their rows"""

    def __init__(self, ctx, rows, n, off, stride=None):
        self.off, self.n = off, n
        pad = [np.concatenate([np.full(off, SENT), r]) for r in rows]
        self.g = Guarded(ctx, pad, n + off, stride=stride)
        self.stride = self.g.stride

    def ptr(self, i):
        return self.g.row(i) + 8 * self.off

    def check(self, what, final=False, **rows):
        self.g.check(what, final=final, **{
            key: np.concatenate([np.full(self.off, SENT), r])
            for key, r in rows.items()})

    def free(self):
        self.g.free()


def cases(L):
    small = sorted(set(EXTRA) | set(bc.small_lengths()))
    out = [(n, kind) for n in small for kind in ("E", "R")]
    if wraps_fit(L):
        out += [(n, "E") for n in bc.wrap_lengths(L)]
    return out


def same_state(got, want, what):
    for key, ref in want.items():
        g = got[key]
        if isinstance(ref, list):
            for i, (a, b) in enumerate(zip(g, ref)):
                ok = a == b if isinstance(b, int) else (
                    (math.isnan(a) and math.isnan(b)) or bc.same_bits([a], [b]))
                assert ok, (what, key, i, a, b)
        elif isinstance(ref, int):
            assert g == ref, (what, key, g, ref)
        else:  # (a NaN's sign and payload are not the recurrence's business)
            assert (math.isnan(g) and math.isnan(ref)) \
                or bc.same_bits([g], [ref]), (what, key, g, ref)


_EXACT = {}


def check_dot(got, a, kind, n, L, what):
    if kind == "E":
        assert float(got) == float(bc.exact_dot_int(a, a)), what
    else:  # (exact rational sums are slow: once for all instantiations)
        if what not in _EXACT:
            _EXACT[what] = bc.exact_dot(a, a)
        ex, sa = _EXACT[what]
        assert bc.sum_within(got, ex, sa, bc.depth(n, L)), what


# ---- update_r ------------------------------------------------------------------------
def test_update_r(ctx, ws, L, nt, off):
    second = ctx.empty(L, np.float64)
    for n, kind in cases(L):
        g = bc.stream_grid(n // 2, L)
        qv, rv = vec(kind, n, 1), vec(kind, n, 2)
        rr, pq = (4.0, 2.0) if kind == "E" else (1.6487212707, 0.7310585786)
        src = Vecs(ctx, [qv], n, off)
        small = n <= 2 * bc.UNIT + 1
        # (a wrap length: one combination -- the trips of the loop do not
        # depend on where pq comes from)
        for mode in (("partials", "two arrays", "slot") if small
                     else ("partials",)):
            what = ("update_r", n, kind, mode)
            r = Vecs(ctx, [rv], n, off)
            ws.reset()
            st = ws.fetch()
            st["rr"] = rr
            st["pq"] = pq if mode == "slot" else SENT
            ws.install(st)
            part = np.zeros(L)
            part[min(3, L - 1)] = SENT if mode == "slot" else (
                pq if mode == "partials" else 0.5 * pq)
            ws.set(PART_PQ, part)
            part2 = np.zeros(L)
            part2[L - 1] = 0.5 * pq
            ctx.copy_h2d(second.at(0), part2)
            ws.set(PART_RRN, np.full(L, SENT))
            call("update_r_f64", ctx.h, ws.h, n, src.ptr(0), r.ptr(0),
                 second.at(0) if mode == "two arrays" else None,
                 int(mode == "slot"), None)
            st["pq"] = pq
            t = cc.cgs_update_r(st, qv, rv)
            src.check(what), r.check(what, r0=t, final=True)
            same_state(ws.fetch(), st, what)
            assert np.all(ws.get(PART_RRN)[g:] == 0), what
            call("reduce", ctx.h, ws.h, RRN, None, None)
            check_dot(ws.get(RRN)[0], t, kind, n, L, what[:3])
            r.free()
        if small:
            # pq <= 0, pq NaN, and `done`: nothing is written
            for pq_bad, done in ((0.0, 0), (-1.0, 0), (float("nan"), 0),
                                 (pq, 1)):
                what = ("update_r", n, kind, pq_bad, done)
                r = Vecs(ctx, [rv], n, off)
                ws.reset()
                st = ws.fetch()
                st.update(rr=rr, pq=pq_bad, done=done, kstop=0 if done else -1)
                ws.install(st)
                ws.set(PART_RRN, np.full(L, SENT))
                call("update_r_f64", ctx.h, ws.h, n, src.ptr(0), r.ptr(0), None,
                     1, None)
                assert cc.cgs_update_r(st, qv, rv) is None
                r.check(what, final=True)
                assert np.all(ws.get(PART_RRN) == SENT), what
                same_state(ws.fetch(), st, what)
                r.free()
        src.check((n, kind), final=True)
        src.free()
    second.free()


# ---- update_xp -----------------------------------------------------------------------
def _lists(ns):
    """(name, upd) for a width: every shift, one shift, a compacted list with
    shifts that stop in this step, none"""
    out = [("all", [s | 8 for s in range(ns)]),
           ("one", [(ns - 1) | 8]),
           ("one stops", [ns // 2]),
           ("none", [])]
    mask = [s for s in range(ns) if 0b10110 >> s & 1]
    if len(mask) > 1:  # shifts 1, 2, 4: the middle one stops
        out.append(("0b10110", [s | (0 if i == 1 else 8)
                                for i, s in enumerate(mask)]))
    if ns > 1:
        out.append(("all stop", list(range(ns))))
    return out


def test_update_xp(ctx, ws, L, nt, off):
    for n, kind in cases(L):
        small = n <= 2 * bc.UNIT + 1
        rv, pv = vec(kind, n, 3), vec(kind, n, 4)
        ro = Vecs(ctx, [rv], n, off)
        widths = (1, 2, 3, 5, 8) if n in (3, bc.UNIT + 1) else (
            (3, 8) if small else (2,))
        for ns in widths:
            xs = [np.roll(vec(kind, n, 5), s) for s in range(ns)]
            pss = [np.roll(vec(kind, n, 6), s) for s in range(ns)]
            # an odd stride where the vectors are offset anyway
            stride = (n + off + 1) // 2 * 2 + (3 if off and n % 2 else 2)
            lists = _lists(ns) if small else _lists(ns)[:1]
            runs = [(name, upd, 3, 3, 0) for name, upd in lists]
            if small and ns == 3:
                full = lists[0][1]
                runs += [("done", full, 3, 3, 1), ("k behind", full, 4, 3, 0),
                         ("k ahead", full, 2, 3, 0)]
            for name, upd, k_arg, k_state, done in runs:
                what = ("update_xp", n, kind, ns, name)
                p = Vecs(ctx, [pv], n, off)
                X = Vecs(ctx, xs, n, off, stride=stride)
                PS = Vecs(ctx, pss, n, off, stride=stride)
                ws.reset(shifts=[float(s) for s in range(ns)])
                st = ws.fetch()
                if kind == "E":
                    co = dict(bn=2.0, zeta=[-1.0, 2.0] * 4, cx=[2.0, -4.0] * 4,
                              cp=[4.0, 0.5, 1.0, -2.0] * 2)
                else:
                    co = dict(bn=0.6180339887,
                              zeta=list(bc.round_vec(8, 91) / 1024.0),
                              cx=list(bc.round_vec(8, 92) / 1024.0),
                              cp=list(bc.round_vec(8, 93) / 1024.0))
                st.update(co, k=k_state, done=done, kstop=k_state if done else -1,
                          n_upd=len(upd), upd=upd + [0] * (8 - len(upd)))
                ws.install(st)
                call("update_xp_f64", ctx.h, ws.h, k_arg, n, ro.ptr(0), p.ptr(0),
                     X.ptr(0), X.stride, PS.ptr(0), PS.stride, None)
                pn, Xn, PSn = cc.cgs_update_xp(st, k_arg, rv, pv, np.array(xs),
                                               np.array(pss))
                moved = {s & 7 for s in upd} if k_arg == k_state else set()
                withp = {s & 7 for s in upd if s & 8} \
                    if k_arg == k_state and not done else set()
                for s in range(ns):  # the restatement itself leaves them alone
                    assert s in moved or bc.same_bits(Xn[s], xs[s]), what
                    assert s in withp or bc.same_bits(PSn[s], pss[s]), what
                ro.check(what)
                p.check(what, r0=pn, final=True)
                # columns that are not named come back as uploaded
                X.check(what, final=True,
                        **{"r%d" % s: Xn[s] for s in sorted(moved)})
                PS.check(what, final=True,
                         **{"r%d" % s: PSn[s] for s in sorted(withp)})
                same_state(ws.fetch(), st, what)
                p.free(), X.free(), PS.free()
        ro.check((n, kind), final=True)
        ro.free()


# ---- the scalar kernels -----------------------------------------------------------
def _feed_rrn(ws, st, L, rrn, reduced):
    """rrn in the slot, or as three partials whose sum is exact"""
    part = np.full(L, SENT if reduced else 0.0)
    if not reduced:
        part[0] = part[min(5, L - 1)] = 0.25 * rrn
        part[L - 1] += 0.5 * rrn
    ws.set(PART_RRN, part)
    st["rrn"] = rrn if reduced else SENT


@pytest.mark.parametrize("reduced", [0, 1])
def test_start_every_branch(ctx, ws, L, reduced):
    for rr in (12.25, 0.0, 1e-300, float("nan")):
        for shifts in (cc.SHIFTS1, cc.SHIFTS4, cc.SHIFTS8):
            ws.reset(shifts=shifts, rtol=1e-10)
            ws.set(HIST, np.full(8 * (KMAX + 1), SENT))
            st = ws.fetch()
            _feed_rrn(ws, st, L, rr, reduced)
            ws.install(st)
            call("start", ctx.h, ws.h, reduced, None)
            hist = np.full((8, KMAX + 1), SENT)
            cc.cgs_start(st, rr, hist)
            same_state(ws.fetch(), st, ("start", rr, shifts))
            assert np.array_equal(ws.hist(), hist, equal_nan=True)
            assert st["done"] == int(rr == 0.0)
    # after `done`: nothing moves
    ws.reset(shifts=cc.SHIFTS4)
    st = ws.fetch()
    st.update(done=1, kstop=2, k=2, rrn=4.0)
    ws.install(st)
    call("start", ctx.h, ws.h, 1, None)
    same_state(ws.fetch(), st, "start after done")
    assert np.all(ws.hist() == 0.0)


def _mid(shifts, **kw):
    """a state in the middle of a solve: k = 3, every second shift stopped"""
    st = cc.new_state(shifts, 1e-10, KMAX)
    ns = len(shifts)
    act = list(range(0, ns, 2)) if ns > 2 else list(range(ns))
    st.update(rr=0.81, pq=1.7320508076, a_old=0.5772156649, b_old=0.4142135624,
              hist0=3.5, k=3, n_act=len(act), act=act + [0] * (8 - len(act)),
              zeta=[0.9 / (1 + s) for s in range(ns)] + [0.0] * (8 - ns),
              rho=[0.8 / (1 + 0.5 * s) for s in range(ns)] + [0.0] * (8 - ns),
              its=[3 if s in act else 2 for s in range(ns)] + [0] * (8 - ns))
    st.update(kw)
    return st


# (name, state in front, rrn)
STEPS = [
    ("the first step", dict(cc.new_state(cc.SHIFTS4, 1e-10, KMAX), rr=12.25,
                            pq=3.0, hist0=3.5), 2.25),
    ("a regular step", _mid(cc.SHIFTS8), 0.49),
    ("some stop", _mid(cc.SHIFTS8, rtol=0.04), 0.49),
    ("all stop", _mid(cc.SHIFTS4, rtol=0.5), 0.49),
    ("one shift", _mid(cc.SHIFTS1), 0.49),
    ("pq == 0", _mid(cc.SHIFTS4, pq=0.0), 0.49),
    ("pq < 0", _mid(cc.SHIFTS4, pq=-2.0), 0.49),
    ("pq NaN", _mid(cc.SHIFTS4, pq=float("nan")), 0.49),
    ("rrn == 0", _mid(cc.SHIFTS4), 0.0),
    ("k + 1 == kmax", _mid(cc.SHIFTS4, kmax=4), 0.49),
    ("k == kmax", _mid(cc.SHIFTS4, kmax=3), 0.49),
    ("rrn NaN goes on", _mid(cc.SHIFTS4), float("nan")),
    ("zeta underflows", _mid((0.0, 1e6), rtol=0.0,
                             zeta=[0.9, 5e-324] + [0.0] * 6), 0.49),
]
_STATUS = {"pq == 0": 1, "pq < 0": 1, "pq NaN": 1}
_GO_ON = ("the first step", "a regular step", "some stop", "one shift",
          "rrn NaN goes on", "zeta underflows")


@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("case", STEPS, ids=[c[0] for c in STEPS])
def test_step_every_branch(ctx, ws, L, case, reduced):
    name, st0, rrn = case
    st = {k: (list(v) if isinstance(v, list) else v) for k, v in st0.items()}
    ws.reset(shifts=st["sigma"][:st["ns"]], rtol=st["rtol"], kmax=st["kmax"])
    ws.set(HIST, np.full(8 * (KMAX + 1), SENT))
    # what the step does not reach keeps its bits
    st.update(cx=[SENT] * 8, cp=[SENT] * 8, bn=SENT)
    _feed_rrn(ws, st, L, rrn, reduced)
    ws.install(st)
    n_act = st["n_act"]
    call("step", ctx.h, ws.h, reduced, None)
    hist = np.full((8, KMAX + 1), SENT)
    if name in _STATUS or name == "k == kmax":
        st["rrn"] = SENT if not reduced else rrn  # (never summed, never stored)
    cc.cgs_step(st, rrn, hist)
    print(name, st)
    got = ws.fetch()
    if name in _STATUS or name == "k == kmax":
        got["rrn"] = st["rrn"]
    same_state(got, st, name)
    assert np.array_equal(ws.hist(), hist, equal_nan=True), name
    assert st["status"] == _STATUS.get(name, 0)
    assert bool(st["done"]) == (name not in _GO_ON), name
    if name == "some stop":  # both branches of the rtol test in one step
        assert 0 < st["n_act"] < n_act == st["n_upd"]
    if name == "zeta underflows":
        assert st["zeta"][1] == 0.0 and st["n_act"] == 2


def test_after_done_and_bad_arguments(ctx, ws):
    ws.reset(shifts=cc.SHIFTS4)
    st = _mid(cc.SHIFTS4, done=1, kstop=3)
    ws.install(st)
    call("step", ctx.h, ws.h, 1, None)
    call("step", ctx.h, ws.h, 0, None)
    call("reduce", ctx.h, ws.h, PQ, None, None)
    same_state(ws.fetch(), st, "after done")
    assert np.all(ws.hist() == 0.0)
    from spmv_amd._lib import SpmvHipError
    buf = ctx.empty(64, np.float64)
    r, p, X, PS = buf.at(0), buf.at(4), buf.at(8), buf.at(32)
    sh = np.zeros(9)
    bad_words = np.zeros(32, np.int32)
    bad_words[13] = 4  # ns
    bad_words[12] = KMAX
    bad_words[15] = 1  # n_upd
    bad_words[24] = 4  # ... of a shift the reset does not have
    for name, args in (
            ("update_xp_f64", (ctx.h, ws.h, KMAX + 1, 4, r, p, X, 4, PS, 4, None)),
            ("update_xp_f64", (ctx.h, ws.h, 0, 4, r, p, X, 4, PS, 4, None)),
            ("update_xp_f64", (ctx.h, ws.h, 1, 4, r, p, X, 3, PS, 4, None)),
            ("update_xp_f64", (ctx.h, ws.h, 1, 4, r, p, X, 4, PS, 3, None)),
            ("update_xp_f64", (ctx.h, ws.h, 1, 4, r, r, X, 4, PS, 4, None)),
            ("update_xp_f64", (ctx.h, ws.h, 1, 4, r, p, X, 4, X, 4, None)),
            ("update_xp_f64", (ctx.h, ws.h, 1, 4, r + 4, p, X, 4, PS, 4, None)),
            ("update_r_f64", (ctx.h, ws.h, 4, r, r, None, 0, None)),
            ("update_r_f64", (ctx.h, ws.h, -1, r, p, None, 0, None)),
            ("reduce", (ctx.h, ws.h, 7, None, None)),
            ("reduce", (ctx.h, ws.h, RRN, r, None)),
            ("ws_reset", (ws.h, 0.0, KMAX + 1, 1, sh.ctypes.data, None)),
            ("ws_reset", (ws.h, 0.0, KMAX, 0, sh.ctypes.data, None)),
            ("ws_reset", (ws.h, 0.0, KMAX, 9, sh.ctypes.data, None)),
            ("ws_set_words", (ws.h, bad_words.ctypes.data, None))):
        with pytest.raises(SpmvHipError):
            call(name, *args)
    buf.free()
