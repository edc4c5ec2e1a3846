"""Every kernel of blas1_idrs.hip launched ALONE through the C ABI, cached and
non-temporal (blas1_nt_min_elems), at 16-byte aligned and at 8-byte-offset
addresses, against the references of idrs_cases.py, bit for bit.

Vectors lie between guard words (test_gpu_gmres_kernels.Guarded; the offset
vectors start one word into their row, that word is a guard too); inputs, and
every column of G and U outside the range a kernel lists, must come back with
the bytes that were uploaded.  Lengths: blas1_cases.small_lengths() (0
included) and a few odd ones on sets E and R, blas1_cases.wrap_lengths on set E.

  sign_dot, omega_dot, omega_update, update: the partial rows against the model
      of idrs_cases.sign_partials / cgs_cases.stream_partials (small lengths,
      bit for bit); on set E the reduced sums against exact integers
  prep (four modes, with and without dinv), update, omega_update: s = 1, 2, 3,
      5, 8 and q = 0, a middle value and s - 1; `done` set: nothing is written
  biortho (a zero, a NaN and an ordinary pivot), omega (tt = 0, tt = NaN, tr =
      0, |rho| on both sides of kappa), step (both branches of the rtol test,
      kmax, start, the om step): the whole device state against the
      restatement's, from the partials and from the slots"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import cgs_cases as cc
import idrs_cases as ic
from spmv_amd import hip
from test_gpu_gmres_kernels import (Guarded, L, nt, peek, poke, vec,  # noqa: F401
                                    wraps_fit)

pytestmark = pytest.mark.gpu

SENT = bc.SENTINEL
KMAX = 8
RED, HIST, PART, SCALARS = range(4)
R_H, R_RR, R_OM, R_HRR = range(4)
SINGLES = ("rtol", "kappa", "om", "rr", "hist0", "be")
ARRAYS = ("f", "c", "a")
WORDS = ("done", "kstop", "status", "k", "kmax", "s")
EXTRA = (63, 65, 257, 1023)
ROW0 = 12345
SQ = (1, 2, 3, 5, 8)


def qs(s):
    return sorted({0, s // 2, s - 1})


class Ws:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call("spmv_hip_idrs_ws_create", ctx.h, KMAX, C.byref(self.h))

    def reset(self, s=1, rtol=0.0, kmax=KMAX, kappa=0.7, seed=0):
        hip.call("spmv_hip_idrs_ws_reset", self.h, float(rtol), float(kappa),
                 kmax, s, seed, None)

    def addr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        hip.call("spmv_hip_idrs_ws_array", self.h, which, C.byref(p), C.byref(n))
        return p.value, n.value

    def set(self, which, values):
        poke(self.ctx, self.addr(which)[0], values)

    def get(self, which):
        p, n = self.addr(which)
        return peek(self.ctx, p, n)

    def part(self, L):
        return self.get(PART).reshape(ic.ROWS, L)

    def fetch(self):
        """the device state as an idrs_cases state dict"""
        d = self.get(SCALARS)
        st = {k: float(d[i]) for i, k in enumerate(SINGLES)}
        for j, k in enumerate(ARRAYS):
            st[k] = [float(v) for v in d[6 + 8 * j:14 + 8 * j]]
        st["red"] = [float(v) for v in d[30:41]]
        st["M"] = [[float(v) for v in d[41 + 8 * i:49 + 8 * i]] for i in range(8)]
        w = np.zeros(6, np.int32)
        hip.call("spmv_hip_idrs_ws_get_words", self.h,
                 w.ctypes.data_as(C.c_void_p), None)
        self.ctx.stream_sync()
        st.update(zip(WORDS, (int(v) for v in w)))
        return st

    def install(self, st):
        d = [st[k] for k in SINGLES]
        for k in ARRAYS:
            d += list(st[k])
        d += list(st["red"])
        for row in st["M"]:
            d += list(row)
        self.set(SCALARS, np.array(d, np.float64))
        w = np.array([st[k] for k in WORDS], np.int32)
        hip.call("spmv_hip_idrs_ws_set_words", self.h,
                 w.ctypes.data_as(C.c_void_p), None)

    def close(self):
        hip.call("spmv_hip_idrs_ws_destroy", self.h)


@pytest.fixture(scope="module")
def ws(ctx):
    w = Ws(ctx)
    yield w
    w.close()


@pytest.fixture(params=[0, 1], ids=["aligned", "offset8"])
def off(request):
    return request.param


def call(name, *a):
    hip.call("spmv_hip_idrs_" + name, *a)


class Vecs:
    """Guarded vectors of n doubles that start `off` words into their rows"""

    def __init__(self, ctx, rows, n, off):
        self.off, self.n = off, n
        pad = [np.concatenate([np.full(off, SENT), r]) for r in rows]
        self.g = Guarded(ctx, pad, n + off, stride=(n + off + 1) // 2 * 2)
        self.stride = self.g.stride

    def ptr(self, i):
        return self.g.row(i) + 8 * self.off

    def check(self, what, final=False, **rows):
        self.g.check(what, final=final, **{
            key: np.concatenate([np.full(self.off, SENT), r])
            for key, r in rows.items()})

    def free(self):
        self.g.free()


def cases(L, wrap=True):
    small = sorted(set(EXTRA) | set(bc.small_lengths()))
    out = [(n, kind) for n in small for kind in ("E", "R")]
    if wrap and wraps_fit(L):
        out += [(n, "E") for n in bc.wrap_lengths(L)]
    return out


def is_small(n):
    return n <= 2 * bc.UNIT + 1


def same_state(got, want, what):
    def eq(a, b):
        if isinstance(b, int):
            return a == b
        return (math.isnan(a) and math.isnan(b)) or bc.same_bits([a], [b])
    for key, ref in want.items():
        g = got[key]
        if key == "M":
            for i in range(8):
                for j in range(8):
                    assert eq(g[i][j], ref[i][j]), (what, key, i, j, g[i][j],
                                                    ref[i][j])
        elif isinstance(ref, list):
            for i, (a, b) in enumerate(zip(g, ref)):
                assert eq(a, b), (what, key, i, a, b)
        else:
            assert eq(g, ref), (what, key, g, ref)


def coef_state(ws, s, seed, **kw):
    """a reset state with small integers for c, a, om and be: on set E every
    result stays an integer"""
    ws.reset(s=s, seed=kw.pop("hash_seed", 0))
    st = ws.fetch()
    rng = np.random.default_rng(seed)
    st["c"] = [float(v) for v in rng.choice([-2.0, -1.0, 1.0, 2.0], 8)]
    st["a"] = [float(v) for v in rng.choice([-2.0, -1.0, 1.0, 2.0], 8)]
    st["om"], st["be"] = 2.0, -2.0
    st.update(kw)
    ws.install(st)
    return st


def columns(kind, n, s, base):
    return [np.roll(vec(kind, n, base + i % 5), i // 5 + 1) for i in range(s)]


def check_rows(ws, L, n, want_rows, what):
    """the partial rows named in want_rows (dict row -> array [L]) bit for bit;
    the other rows still hold the sentinel"""
    got = ws.part(L)
    for j in range(ic.ROWS):
        if j in want_rows:
            assert bc.same_bits(got[j], want_rows[j]), (what, "row", j)
        else:
            assert np.all(got[j] == SENT), (what, "row", j, "was written")


# ---- sign_dot -----------------------------------------------------------------------
def test_sign_dot(ctx, ws, L, nt, off):
    for n, kind in cases(L, wrap=off == 0):
        wv = vec(kind, n, 1)
        src = Vecs(ctx, [wv], n, off)
        for s in (SQ if is_small(n) and n in (0, 3, 1023, 2 * bc.UNIT + 1)
                  else (2,)):
            for ww in (0, 1):
                what = ("sign_dot", n, kind, s, ww)
                ws.reset(s=s, seed=s)
                ws.set(PART, np.full(ic.ROWS * L, SENT))
                call("sign_dot_f64", ctx.h, ws.h, n, ROW0, src.ptr(0), ww, None)
                P = ic.shadow_signs(ROW0, n, s, seed=s)
                if is_small(n):
                    rows = ic.sign_partials(wv, P, L, with_ww=bool(ww))
                    want = {j: rows[j] for j in range(s)}
                    if ww:
                        want[ic.ROW_RR] = rows[s]
                    check_rows(ws, L, n, want, what)
                call("reduce", ctx.h, ws.h, R_HRR if ww else R_H, None)
                red = ws.get(RED)
                if kind == "E":
                    for j in range(s):
                        assert red[j] == float(bc.exact_dot_int(P[j], wv)), what
                    if ww:
                        assert red[s] == float(bc.exact_dot_int(wv, wv)), what
        src.check(("sign_dot", n, kind), final=True)
        src.free()


def test_sign_dot_done(ctx, ws, L):
    wv = vec("R", 1023, 1)
    src = Vecs(ctx, [wv], 1023, 0)
    st = coef_state(ws, 3, 1, done=1, kstop=0)
    ws.set(PART, np.full(ic.ROWS * L, SENT))
    call("sign_dot_f64", ctx.h, ws.h, 1023, 0, src.ptr(0), 1, None)
    call("omega_dot_f64", ctx.h, ws.h, 1023, src.ptr(0), src.ptr(0), None)
    call("reduce", ctx.h, ws.h, R_HRR, None)
    check_rows(ws, L, 1023, {}, "done")
    same_state(ws.fetch(), st, "done")
    src.free()


# ---- prep ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_dinv", [False, True], ids=["none", "dinv"])
def test_prep(ctx, ws, L, nt, off, with_dinv):
    for n, kind in cases(L, wrap=off == 0):
        small = is_small(n)
        for s in (SQ if small and n in (0, 1, 3, 65, 1023, bc.UNIT + 1) else (2,)):
            rv = vec(kind, n, 2)
            dv = vec("d" + kind, n, 3) if with_dinv else None
            G, U = columns(kind, n, s, 10), columns(kind, n, s, 20)
            src = Vecs(ctx, [rv] + G + U + ([dv] if with_dinv else []), n, off)
            d_ptr = src.ptr(1 + 2 * s) if with_dinv else None
            for q in (qs(s) if small else (1,)):
                st = coef_state(ws, s, 7 * s + q)
                for mode in ((ic.FUSED, ic.STORE_V, ic.FROM_VH, ic.PLAIN) if small
                             else (ic.FUSED,)):
                    what = ("prep", n, kind, s, q, mode, with_dinv)
                    out = Vecs(ctx, [rv if mode == ic.FROM_VH else
                                     np.full(n, SENT)], n, off)
                    qq = s if mode == ic.PLAIN else q
                    call("prep_f64", ctx.h, ws.h, qq, mode, n,
                         out.ptr(0) if mode == ic.FROM_VH else src.ptr(0),
                         src.ptr(1), src.ptr(1 + s), src.stride, d_ptr,
                         out.ptr(0), None)
                    want = ic.idrs_prep(st, qq, mode, rv, G, U, dinv=dv, vh=rv)
                    out.check(what, r0=want, final=True)
                    out.free()
            # done: nothing is written
            if small and n:
                st = coef_state(ws, s, 3, done=1, kstop=0)
                out = Vecs(ctx, [np.full(n, SENT)], n, off)
                call("prep_f64", ctx.h, ws.h, 0, ic.FUSED, n, src.ptr(0),
                     src.ptr(1), src.ptr(1 + s), src.stride, d_ptr, out.ptr(0),
                     None)
                out.check(("prep done", n), final=True)
                out.free()
            src.check(("prep", n, kind, s), final=True)
            src.free()


# ---- update -------------------------------------------------------------------------
def test_update(ctx, ws, L, nt, off):
    for n, kind in cases(L, wrap=off == 0):
        small = is_small(n)
        for s in (SQ if small and n in (0, 1, 3, 65, 1023, bc.UNIT + 1) else (2,)):
            gv, uv = vec(kind, n, 4), vec(kind, n, 5)
            rv, xv = vec(kind, n, 6), vec(kind, n, 7)
            G, U = columns(kind, n, s, 10), columns(kind, n, s, 20)
            src = Vecs(ctx, [gv, uv], n, off)
            for q in (qs(s) if small else (1,)):
                for done in ((0, 1) if small and n else (0,)):
                    what = ("update", n, kind, s, q, done)
                    st = coef_state(ws, s, 5 * s + q, done=done,
                                    kstop=0 if done else -1)
                    ws.set(PART, np.full(ic.ROWS * L, SENT))
                    io = Vecs(ctx, G + U + [rv, xv], n, off)
                    call("update_f64", ctx.h, ws.h, q, n, src.ptr(0), src.ptr(1),
                         io.ptr(0), io.ptr(s), io.stride, io.ptr(2 * s),
                         io.ptr(2 * s + 1), None)
                    out = ic.idrs_update(st, q, gv, uv, G, U, rv, xv)
                    if out is None:
                        io.check(what, final=True)
                        check_rows(ws, L, n, {}, what)
                    else:
                        io.check(what, final=True, **{
                            f"r{q}": out[0], f"r{s + q}": out[1],
                            f"r{2 * s}": out[2], f"r{2 * s + 1}": out[3]})
                        if small:
                            check_rows(ws, L, n, {ic.ROW_RR: cc.stream_partials(
                                out[2], out[2], L)}, what)
                        call("reduce", ctx.h, ws.h, R_RR, None)
                        if kind == "E":
                            assert ws.get(RED)[s] == float(
                                bc.exact_dot_int(out[2], out[2])), what
                    same_state(ws.fetch(), dict(st, red=ws.fetch()["red"]), what)
                    io.free()
            src.check(("update", n, kind, s), final=True)
            src.free()


# ---- omega_dot, omega_update ----------------------------------------------------------
def test_omega_dot_and_update(ctx, ws, L, nt, off):
    for n, kind in cases(L, wrap=off == 0):
        small = is_small(n)
        tv, vv = vec(kind, n, 4), vec(kind, n, 5)
        rv, xv = vec(kind, n, 6), vec(kind, n, 7)
        src = Vecs(ctx, [tv, vv], n, off)
        for s in (SQ if small and n in (0, 3, 1023, bc.UNIT + 1) else (5,)):
            for done in ((0, 1) if small and n else (0,)):
                what = ("omega", n, kind, s, done)
                st = coef_state(ws, s, s, done=done, kstop=0 if done else -1,
                                hash_seed=9)
                ws.set(PART, np.full(ic.ROWS * L, SENT))
                io = Vecs(ctx, [rv, xv], n, off)
                call("omega_dot_f64", ctx.h, ws.h, n, src.ptr(0), io.ptr(0), None)
                want = {}
                if not done and small:
                    want = {ic.ROW_TR: cc.stream_partials(tv, rv, L),
                            ic.ROW_TT: cc.stream_partials(tv, tv, L)}
                if small:
                    check_rows(ws, L, n, want, what)
                if not done:
                    call("reduce", ctx.h, ws.h, R_OM, None)
                    if kind == "E":
                        red = ws.get(RED)
                        assert red[9] == float(bc.exact_dot_int(tv, rv)), what
                        assert red[10] == float(bc.exact_dot_int(tv, tv)), what
                call("omega_update_f64", ctx.h, ws.h, n, ROW0, src.ptr(0),
                     src.ptr(1), io.ptr(0), io.ptr(1), None)
                out = ic.idrs_omega_update(st, tv, vv, rv, xv)
                if out is None:
                    io.check(what, final=True)
                else:
                    io.check(what, final=True, r0=out[0], r1=out[1])
                    P = ic.shadow_signs(ROW0, n, s, seed=9)
                    if small:
                        rows = ic.sign_partials(out[0], P, L, with_ww=True)
                        want.update({j: rows[j] for j in range(s)})
                        want[ic.ROW_RR] = rows[s]
                        check_rows(ws, L, n, want, what)
                    call("reduce", ctx.h, ws.h, R_HRR, None)
                    if kind == "E":
                        red = ws.get(RED)
                        for j in range(s):
                            assert red[j] == float(
                                bc.exact_dot_int(P[j], out[0])), what
                        assert red[s] == float(
                            bc.exact_dot_int(out[0], out[0])), what
                io.free()
        src.check(("omega", n, kind), final=True)
        src.free()


# ---- the scalar kernels -----------------------------------------------------------------
def _state(ws, s, seed, **kw):
    """a state with a well-conditioned lower triangular M and random f, a, c"""
    ws.reset(s=s, rtol=kw.pop("rtol", 1e-3), kmax=kw.pop("kmax", KMAX))
    st = ws.fetch()
    rng = np.random.default_rng(seed)
    for i in range(8):
        for j in range(i + 1):
            st["M"][i][j] = float(rng.uniform(0.5, 2.0) if i == j
                                  else rng.uniform(-1, 1))
    st["f"] = [float(v) for v in rng.uniform(-1, 1, 8)]
    st["a"] = [float(v) for v in rng.uniform(-1, 1, 8)]
    st["c"] = [float(v) for v in rng.uniform(-1, 1, 8)]
    st.update(om=0.75, be=0.3, rr=2.0, hist0=4.0)
    st.update(kw)
    ws.install(st)
    return st


def _install_sums(ws, L, reduced, rows, slots):
    """rows: dict row -> value (spread over two partials); slots: dict slot ->
    value.  The other source holds the sentinel."""
    part = np.full((ic.ROWS, L), SENT)
    red = np.full(ic.ROWS, SENT)
    for j, v in rows.items():
        part[j] = 0.0
        if reduced:
            part[j] = SENT
        else:
            part[j, 0], part[j, L - 1] = 0.25 * v, 0.75 * v
    if reduced:
        for j, v in slots.items():
            red[j] = v
    ws.set(PART, part.reshape(-1))
    return red


def _split(v):
    """what sum_partials makes of 0.25 v in slot 0 and 0.75 v in slot L - 1"""
    return float(np.float64(0.25 * v) + np.float64(0.75 * v))


@pytest.mark.parametrize("reduced", [0, 1], ids=["partials", "slots"])
@pytest.mark.parametrize("s", SQ)
def test_biortho(ctx, ws, L, s, reduced):
    rng = np.random.default_rng(s)
    for q in qs(s):
        for pivot in ("ordinary", "zero", "nan"):
            what = ("biortho", s, q, pivot, reduced)
            st = _state(ws, s, 10 * s + q)
            h = [float(v) for v in rng.uniform(-2, 2, s)]
            if pivot == "nan":
                h[q] = float("nan")
            if pivot == "zero":  # h_q = sum a_j M[q][j] exactly: no a_j at all
                for j in range(q):
                    st["M"][q][j] = 0.0
                h[q] = 0.0
                ws.install(st)
            red = _install_sums(ws, L, reduced, dict(enumerate(h)),
                                dict(enumerate(h)))
            if reduced:
                st["red"] = [float(v) for v in red]
                ws.install(st)
            hist = ws.get(HIST)
            call("biortho", ctx.h, ws.h, q, reduced, None)
            ic.idrs_biortho(st, q, h if reduced else [_split(v) for v in h])
            assert st["done"] == (pivot != "ordinary") and \
                st["status"] == (pivot != "ordinary"), what
            got = ws.fetch()
            if not reduced:
                st["red"] = got["red"]
            same_state(got, st, what)
            assert bc.same_bits(ws.get(HIST), hist), what
    st = _state(ws, s, 1, done=1, kstop=3)
    call("biortho", ctx.h, ws.h, 0, 0, None)
    same_state(ws.fetch(), st, "biortho done")


@pytest.mark.parametrize("reduced", [0, 1], ids=["partials", "slots"])
def test_omega(ctx, ws, L, reduced):
    nan = float("nan")
    # rr = 2, kappa = 0.7: rho = tr / (sqrt(tt) sqrt(2))
    for name, tr, tt, status in (("tt zero", 1.0, 0.0, 2), ("tt nan", 1.0, nan, 2),
                                 ("tt negative", 1.0, -1.0, 2),
                                 ("tr zero", 0.0, 3.0, 2), ("tr nan", nan, 3.0, 2),
                                 ("rho above kappa", 2.4, 3.0, 0),
                                 ("rho below kappa", 0.3, 3.0, 0),
                                 ("rho negative below", -0.3, 3.0, 0),
                                 ("rho negative above", -2.4, 3.0, 0)):
        what = ("omega", name, reduced)
        st = _state(ws, 4, 3)
        red = _install_sums(ws, L, reduced, {ic.ROW_TR: tr, ic.ROW_TT: tt},
                            {ic.ROW_TR: tr, ic.ROW_TT: tt})
        if reduced:
            st["red"] = [float(v) for v in red]
            ws.install(st)
        call("omega", ctx.h, ws.h, reduced, None)
        ic.idrs_omega(st, tr if reduced else _split(tr),
                      tt if reduced else _split(tt))
        assert st["status"] == status and st["done"] == (status != 0), what
        if name == "rho below kappa":
            assert st["om"] > 0.3 / 3.0
        got = ws.fetch()
        if not reduced:
            st["red"] = got["red"]
        same_state(got, st, what)
    st = _state(ws, 4, 3, done=1, kstop=2)
    call("omega", ctx.h, ws.h, 0, None)
    same_state(ws.fetch(), st, "omega done")


@pytest.mark.parametrize("reduced", [0, 1], ids=["partials", "slots"])
@pytest.mark.parametrize("s", SQ)
def test_step(ctx, ws, L, s, reduced):
    rng = np.random.default_rng(100 + s)
    runs = []
    for q in [-1] + qs(s) + [s]:
        # hist0 = 4: rr = 2 goes on at rtol 1e-3 and stops at rtol 1
        runs += [(q, 2.0, 1e-3, 3, KMAX), (q, 2.0, 1.0, 3, KMAX),
                 (q, 2.0, 1e-3, KMAX - 1, KMAX), (q, float("nan"), 1e-3, 3, KMAX)]
    runs += [(-1, 0.0, 1e-3, 0, KMAX), (-1, 2.0, 1e-3, 0, 0),
             (0, 2.0, 1e-3, 2, 2)]
    for q, rr, rtol, k, kmax in runs:
        what = ("step", s, q, rr, rtol, k, kmax, reduced)
        st = _state(ws, s, 20 * s + q + 1, rtol=rtol, kmax=kmax,
                    k=0 if q < 0 else min(k, kmax))
        h = [float(v) for v in rng.uniform(-2, 2, s)]
        rows = dict(enumerate(h))
        rows[ic.ROW_RR] = rr
        slots = dict(enumerate(h))
        slots[s] = rr
        red = _install_sums(ws, L, reduced, rows, slots)
        if reduced:
            st["red"] = [float(v) for v in red]
            ws.install(st)
        hist = ws.get(HIST)
        call("step", ctx.h, ws.h, q, reduced, None)
        ic.idrs_step(st, q, h if reduced else [_split(v) for v in h],
                     rr if reduced else _split(rr), hist)
        got = ws.fetch()
        if not reduced:
            st["red"] = got["red"]
        same_state(got, st, what)
        assert bc.same_bits(ws.get(HIST), hist), what
    st = _state(ws, s, 1, done=1, kstop=3)
    hist = ws.get(HIST)
    call("step", ctx.h, ws.h, 0, 0, None)
    call("start", ctx.h, ws.h, 0, None)
    same_state(ws.fetch(), st, "step done")
    assert bc.same_bits(ws.get(HIST), hist)
