"""Every vector kernel of the five Krylov solvers launched ALONE through the C
ABI (include/spmv_hip.h) and compared with the references of blas1_cases.py:

  set E (exact integers) at every length, the wrap edges W - 1 .. W + unit + 3
        included (W = 2 * kU * kBlock * dot_partials_len doubles: the length at
        which a workgroup takes a second trip round its loop): equality of bits;
  set R (irrational) at the small edges: element-wise equality of bits with the
        unfused restatement; sums inside blas1_cases.sum_bound for the depth
        blas1_cases.depth reads off the kernels (no measured tolerance here).

Every vector lies between guard words, inputs must come back unchanged,
write-only buffers start as a sentinel, and each kernel runs cached and
non-temporal (blas1_nt_min_elems = default / 1).  Scalars are installed through
the workspace accessors; a partial array without an accessor is reached by
driving producer and consumer as a pair and reading the slot the consumer (or
the reducer) writes.
"""
import ctypes as C

import numpy as np
import pytest

import blas1_cases as bc
from spmv_amd import hip
from spmv_amd._lib import SpmvHipError

pytestmark = pytest.mark.gpu

G = 16            # guard doubles on either side of a vector
NT_DEFAULT = 1 << 24
KMAX = 4
SENT = bc.SENTINEL
EINVAL = -1       # SPMV_HIP_EINVAL


def peek(ctx, ptr, count, dtype=np.float64):
    out = np.empty(count, dtype)
    hip.call("spmv_hip_copy_d2h_async", ctx.h, out.ctypes.data_as(C.c_void_p),
             ptr, out.nbytes, None)
    ctx.stream_sync()
    return out


def poke(ctx, ptr, values):
    ctx.copy_h2d(ptr, np.ascontiguousarray(values, np.float64))


class Arena:
    """One device allocation cut into slots of `cap` doubles plus guards."""

    def __init__(self, ctx, cap, slots):
        self.ctx, self.cap = ctx, cap
        self.stride = (cap + 2 * G + 2 + 1) // 2 * 2
        self.buf = ctx.empty(self.stride * slots, np.float64)
        self.slots = slots

    def free(self):
        self.buf.free()


class Vecs:
    """The vectors of one kernel call: name -> slot, with what was uploaded."""

    def __init__(self, arena, n):
        self.ar, self.n, self.slot, self.host, self.off = arena, n, {}, {}, {}
        assert n <= arena.cap

    def _base(self, name):
        return self.ar.buf.at(self.slot[name] * self.ar.stride)

    def put(self, name, data, off=0):
        """upload `data` between guards (`off` = 1: 8 bytes off 16-byte
        alignment); returns the device address of element 0"""
        assert len(data) == self.n and name not in self.slot
        self.slot[name] = len(self.slot)
        assert self.slot[name] < self.ar.slots
        img = np.full(self.n + 2 * G + off, SENT)
        img[G + off:G + off + self.n] = data
        self.ar.ctx.copy_h2d(self._base(name), img)
        self.host[name], self.off[name] = np.array(data, np.float64), off
        return self.ar.buf.at(self.slot[name] * self.ar.stride + G + off)

    def out(self, name, off=0):
        """a write-only vector: starts as the sentinel"""
        return self.put(name, np.full(self.n, SENT), off)

    def expect(self, **want):
        """download every vector: guards intact, the named ones equal `want`
        bit for bit, all others as uploaded"""
        for name in self.slot:
            off = self.off[name]
            img = peek(self.ar.ctx, self._base(name), self.n + 2 * G + off)
            assert np.all(img[:G + off] == SENT), f"{name}: guard below hit"
            assert np.all(img[G + off + self.n:] == SENT), f"{name}: guard above hit"
            ref = want.get(name, self.host[name])
            got = img[G + off:G + off + self.n]
            if not bc.same_bits(got, ref):
                bad = np.flatnonzero(got.view(np.uint64)
                                     != np.ascontiguousarray(ref).view(np.uint64))
                raise AssertionError(
                    f"{name}: {bad.size} of {self.n} elements differ, first at "
                    f"{bad[0]}: got {got[bad[0]]!r}, want {ref[bad[0]]!r}")


@pytest.fixture(scope="module")
def L(ctx):
    return ctx.dot_partials_len


@pytest.fixture(scope="module")
def arena(ctx, L):
    cap = bc.wrap_lengths(L)[-1] if wraps_fit(L) else bc.small_lengths()[-1] + 8
    a = Arena(ctx, cap + 8, 8)
    yield a
    ctx.stream_sync()
    a.free()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, ctx):
    ctx.set_option("blas1_nt_min_elems", request.param)
    yield request.param
    ctx.set_option("blas1_nt_min_elems", NT_DEFAULT)


def wraps_fit(L):
    return bc.wrap_length(L) <= bc.WRAP_MAX


def lengths(L):
    """[(n, kind)]: set E everywhere, set R at the small edges.  The default
    threshold (2**24 doubles) keeps every length here cached; 1 makes every
    length >= 1 non-temporal.  A grid too large for the wrap edges leaves the
    small ones (test_wrap_edges_fit then skips with the reason)."""
    out = [(n, k) for n in bc.small_lengths() for k in ("E", "R")]
    return out + ([(n, "E") for n in bc.wrap_lengths(L)] if wraps_fit(L) else [])


def test_wrap_edges_fit(L):
    if not wraps_fit(L):
        pytest.skip(f"dot_partials_len = {L}: W = {bc.wrap_length(L)} doubles "
                    f"exceeds {bc.WRAP_MAX}; every test here ran its small "
                    "edges only, the wrap edges need a smaller grid")
    assert bc.wrap_lengths(L)[-1] < NT_DEFAULT  # cached at the default threshold


_POOL = {}


def vec(kind, n, seed):
    """slices of one pool per (kind, seed): a wrap-edge case costs no new
    random numbers"""
    key = (kind, seed)
    if key not in _POOL or len(_POOL[key]) < n:
        m = max(n, 2 * bc.UNIT + 1) if kind == "R" else max(n, 1 << 23)
        gen = {"E": bc.exact_vec, "R": bc.round_vec, "dE": bc.exact_dinv,
               "dR": bc.round_dinv}[kind]
        _POOL[key] = gen(m, seed)
    return _POOL[key][:n]


def dinv_of(kind, n):
    return vec("d" + kind, n, 0)


def check_sum(kind, got, a, b, d, roundings=1, what="sum"):
    """E: the integer itself.  R: the exact sum within the bound of depth d."""
    if kind == "E":
        want = bc.exact_dot_int(a, b)
        assert float(got) == float(want) and abs(want) < 2 ** 53, (what, got, want)
    else:
        ex, sa = bc.exact_dot(a, b)
        assert bc.sum_within(got, ex, sa, d, roundings), (
            what, got, float(ex), float(bc.sum_bound(d, sa, roundings)))


def one_nonzero(L, value, where=5):
    p = np.zeros(L)
    p[where % L] = value
    return p


# ---------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------
class Ws:
    """a solver workspace and the device addresses of its scalar slots"""
    prefix = None
    slots = ()  # accessor suffix -> doubles per k

    def __init__(self, ctx, *extra):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call(f"spmv_hip_{self.prefix}_ws_create", ctx.h, KMAX, *extra,
                 C.byref(self.h))
        self.width = dict(self.slots)
        self.reset(bc.RTOL_GO)

    def reset(self, rtol):
        hip.call(f"spmv_hip_{self.prefix}_ws_reset", self.h, float(rtol), None)

    def addr(self, which, k=None):
        p = C.c_void_p()
        name = f"spmv_hip_{self.prefix}_ws_{which}"
        if k is None:
            hip.call(name, self.h, C.byref(p))
        else:
            hip.call(name, self.h, k, C.byref(p))
        return p.value

    def set(self, which, k, *values):
        assert len(values) == self.width[which]
        poke(self.ctx, self.addr(which, k), values)

    def get(self, which, k):
        v = peek(self.ctx, self.addr(which, k), self.width[which])
        return v[0] if len(v) == 1 else v

    def history(self):
        return np.concatenate([peek(self.ctx, self.addr(w, 0),
                                    self.width[w] * (KMAX + 1))
                               for w in self.width])

    def done(self):
        return int(peek(self.ctx, self.addr("done_flag"), 1, np.int32)[0])

    def close(self):
        hip.call(f"spmv_hip_{self.prefix}_ws_destroy", self.h)


class CgWs(Ws):
    prefix, slots = "cg", (("rr", 1), ("pAp", 1))

    def install(self, s, rtol):
        """iteration k = 2 about to run its vector kernels"""
        self.reset(rtol)
        self.set("rr", 0, s["rr0"])
        self.set("pAp", 1, s["pAp_prev"])
        self.set("rr", 1, s["rr_prev"])
        self.set("pAp", 2, s["pAp"])
        self.set("rr", 2, s["rr_new"])

    def raise_done(self):
        """the legitimate way: reduce_pAp(k) finds that rr[k-1] met the tolerance"""
        self.reset(bc.RTOL_STOP)
        self.set("rr", 0, 1.0)
        self.set("rr", 1, 1.0)
        hip.call("spmv_hip_cg_reduce_pAp", self.ctx.h, self.h, 2, None)
        assert self.done() == 1


class PcgWs(Ws):
    prefix, slots = "pcg", (("rz_rr", 2), ("pAp", 1))

    def install(self, s, rtol):
        self.reset(rtol)
        self.set("rz_rr", 0, 1.0, s["rr0"])
        self.set("rz_rr", 1, s["rz_prev"], s["rr0"] * 2.0 ** 100)
        self.set("pAp", 2, s["pAp"])
        self.set("rz_rr", 2, s["rz_new"], s["rr_new"])

    def raise_done(self):
        self.reset(bc.RTOL_STOP)
        self.set("rz_rr", 0, 1.0, 1.0)
        self.set("rz_rr", 1, 1.0, 1.0)
        hip.call("spmv_hip_pcg_reduce_pAp", self.ctx.h, self.h, 2, None)
        assert self.done() == 1


class BicgWs(Ws):
    prefix, slots = "bicg", (("rv", 1), ("ts_tt", 2), ("rr_rho", 2))

    def install(self, s, rtol):
        self.reset(rtol)
        self.set("rr_rho", 0, s["rr0"], s["rr0"])
        self.set("rr_rho", 1, s["rr0"], s["rho_prev"])
        self.set("rv", 2, s["rv"])
        self.set("ts_tt", 2, s["ts"], s["tt"])
        self.set("rr_rho", 2, s["rr_new"], s["rho_new"])

    def raise_done(self):
        """update_s finds rr[0] == 0 (b = 0): stopped at k = 0.  n = 0: no
        vector is touched."""
        self.reset(bc.RTOL_GO)
        hip.call("spmv_hip_bicg_update_s_f64", self.ctx.h, self.h, 1, 0, None,
                 None, None, None, None, None)
        assert self.done() == 1


@pytest.fixture(scope="module")
def cgws(ctx):
    w = CgWs(ctx)
    yield w
    w.close()


@pytest.fixture(scope="module")
def pcgws(ctx):
    w = PcgWs(ctx)
    yield w
    w.close()


@pytest.fixture(scope="module")
def bicgws(ctx):
    w = BicgWs(ctx)
    yield w
    w.close()


MODES = ("go", "stop", "done")
# Where rr[k] is the device's own sum (producer / consumer pairs), the branch
# is set by the tolerance alone: 0 never stops; 2**40 stops any r of these
# sets (sqrt(rr[k] / rr[0]) < 2**28) while rr[k-1] = 2**100 rr[0] keeps the
# prologue's test of iteration k - 1 from firing (2**50 against 2**40).
PAIR_RTOL = {"go": 0.0, "stop": 2.0 ** 40, "done": 0.0}
BIG = 2.0 ** 100


def arm(ws, scal, mode, pair=False):
    """install the scalars of iteration 2 for a branch; returns (converged,
    snapshot of the history for `done`)"""
    if mode == "done":
        ws.raise_done()
        return False, ws.history()
    if pair:
        ws.install(scal, PAIR_RTOL[mode])
    else:
        ws.install(scal, bc.RTOL_STOP if mode == "stop" else bc.RTOL_GO)
    return mode == "stop", None


def untouched(ws, snap):
    assert bc.same_bits(ws.history(), snap), "a scalar moved after done"
    assert ws.done() == 1


# ---------------------------------------------------------------------------
# blas1.hip: plain dots, axpy, convert, residual
# ---------------------------------------------------------------------------
def test_dot_partial_and_reduce(ctx, arena, L, nt):
    part = ctx.empty(L, np.float64)
    res = ctx.empty(1, np.float64)
    for n, kind in lengths(L):
        x, y = vec(kind, n, 1), vec(kind, n, 2)
        V = Vecs(arena, n)
        px, py = V.put("x", x), V.put("y", y)
        part.write(np.full(L, SENT))
        res.write([SENT])
        hip.call("spmv_hip_dot_partial_f64", ctx.h, n, px, py, part.ptr, None)
        hip.call("spmv_hip_reduce_partials_f64", ctx.h, part.ptr, res.ptr, None)
        V.expect()
        p = part.numpy()
        g = bc.stream_grid(n // 2, L)
        assert np.all(p[g:] == 0) and not np.any(np.signbit(p[g:]))
        if kind == "E":
            assert sum(int(v) for v in p) == bc.exact_dot_int(x, y)
        check_sum(kind, res.numpy()[0], x, y, bc.depth(n, L))
        # x 8 bytes off 16-byte alignment: refused, nothing written
        if n:
            V2 = Vecs(arena, n)
            qx, qy = V2.put("x", x, off=1), V2.put("y", y)
            part.write(np.full(L, SENT))
            with pytest.raises(SpmvHipError) as err:
                hip.call("spmv_hip_dot_partial_f64", ctx.h, n, qx, qy, part.ptr,
                         None)
            assert err.value.code == EINVAL
            ctx.stream_sync()
            assert np.all(part.numpy() == SENT)
    part.free(), res.free()


def test_dot_one_hot(ctx, arena, L, nt):
    """x = e_i: the reduced dot is y_i in bits, every other product a zero"""
    part = ctx.empty(L, np.float64)
    res = ctx.empty(1, np.float64)
    big = bc.wrap_lengths(L)[-1] if wraps_fit(L) else 0
    for n in bc.small_lengths()[1:] + ([big] if big else []):
        y = vec("R" if n <= 2 * bc.UNIT + 1 else "E", n, 2)
        V = Vecs(arena, n)
        px, py = V.put("x", np.zeros(n)), V.put("y", y)
        prev = None
        for i in bc.onehot_indices(n, L):
            if prev is not None:
                poke(ctx, px + 8 * prev, [0.0])
            poke(ctx, px + 8 * i, [1.0])
            prev = i
            hip.call("spmv_hip_dot_partial_f64", ctx.h, n, px, py, part.ptr, None)
            hip.call("spmv_hip_reduce_partials_f64", ctx.h, part.ptr, res.ptr,
                     None)
            assert bc.same_bits(res.numpy(), y[i:i + 1]), (n, i)
    part.free(), res.free()


def test_axpy_convert_scale(ctx, arena, L, nt):
    for n, kind in lengths(L):
        s = bc.cheb_scalars(kind)
        x, y = vec(kind, n, 1), vec(kind, n, 2)
        for off in (0, 1):  # any alignment
            V = Vecs(arena, n)
            px, py = V.put("x", x, off), V.put("y", y)
            hip.call("spmv_hip_axpy_f64", ctx.h, n, s["a"], px, py, None)
            V.expect(y=bc.axpy(s["a"], x, y))
        for dinv in (None, dinv_of(kind, n)):
            V = Vecs(arena, n)
            pi, po = V.put("in", x, 1), V.out("out")
            pd = None if dinv is None else V.put("dinv", dinv)
            hip.call("spmv_hip_cheb_scale_f64", ctx.h, n, s["s"], pd, pi, po, None)
            V.expect(out=bc.cheb_scale(s["s"], dinv, x))
        if n <= 2 * bc.UNIT + 1:
            out = ctx.upload(np.full(n + 2, np.float32(SENT)), np.float32)
            V = Vecs(arena, n)
            px = V.put("x", x)
            hip.call("spmv_hip_convert_f64_f32", ctx.h, n, px, out.at(1), None)
            V.expect()
            o = out.numpy()
            assert o[0] == np.float32(SENT) and o[-1] == np.float32(SENT)
            assert np.array_equal(o[1:-1].view(np.uint32),
                                  x.astype(np.float32).view(np.uint32))
            out.free()


@pytest.mark.parametrize("respect_done", [0, 1])
def test_cg_residual(ctx, arena, L, nt, cgws, respect_done):
    for n, kind in lengths(L):
        b, Ax = vec(kind, n, 1), vec(kind, n, 2)
        for done in (False, True):
            if done:
                cgws.raise_done()
            else:
                cgws.reset(bc.RTOL_GO)
            poke(ctx, cgws.addr("partials"), np.full(L, SENT))
            V = Vecs(arena, n)
            pb, pa, pr = V.put("b", b, 1), V.put("Ax", Ax), V.out("r")
            hip.call("spmv_hip_cg_residual_f64", ctx.h, cgws.h, respect_done, n,
                     pb, pa, pr, None)
            part = peek(ctx, cgws.addr("partials"), L)
            if done and respect_done:
                V.expect()
                assert np.all(part == SENT)
                continue
            r = bc.cg_residual(b, Ax)
            V.expect(r=r)
            assert np.all(part[bc.rows_grid(n, L):] == 0)
            if kind == "E":
                assert sum(int(v) for v in part) == bc.exact_dot_int(r, r)
            if not done:  # the reducer is a no-op after done, by contract
                hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 3, None)
                check_sum(kind, cgws.get("rr", 3), r, r,
                          bc.depth(n, L, streaming=False))


# ---------------------------------------------------------------------------
# blas1.hip: cg
# ---------------------------------------------------------------------------
def test_cg_init_and_dot_rr(ctx, arena, L, nt, cgws):
    for n, kind in lengths(L):
        b = vec(kind, n, 1)
        cgws.reset(bc.RTOL_GO)
        poke(ctx, cgws.addr("partials"), np.full(L, SENT))
        V = Vecs(arena, n)
        pb = V.put("b", b, 1)
        pr, pp, px = V.out("r", 1), V.out("p"), V.out("x")
        hip.call("spmv_hip_cg_init_f64", ctx.h, cgws.h, n, pb, pr, pp, px, None)
        hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 0, None)
        V.expect(r=b, p=b, x=np.zeros(n))
        part = peek(ctx, cgws.addr("partials"), L)
        assert np.all(part[bc.rows_grid(n, L):] == 0)
        check_sum(kind, cgws.get("rr", 0), b, b, bc.depth(n, L, streaming=False))
        # the stand-alone r.r of k = 0
        poke(ctx, cgws.addr("partials"), np.full(L, SENT))
        V = Vecs(arena, n)
        pr = V.put("r", b)
        hip.call("spmv_hip_cg_dot_rr_f64", ctx.h, cgws.h, n, pr, None)
        hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 1, None)
        V.expect()
        part = peek(ctx, cgws.addr("partials"), L)
        assert np.all(part[bc.stream_grid(n // 2, L):] == 0)
        check_sum(kind, cgws.get("rr", 1), b, b, bc.depth(n, L))


@pytest.mark.parametrize("kernel", ["update_xr", "update_r"])
@pytest.mark.parametrize("mode", ["go", "done"])
def test_cg_update_r_side(ctx, arena, L, nt, cgws, kernel, mode):
    for n, kind in lengths(L):
        s = bc.cg_scalars(kind)
        p, Ap, x, r = (vec(kind, n, i) for i in (1, 2, 3, 4))
        _, snap = arm(cgws, s, mode)
        poke(ctx, cgws.addr("partials"), np.full(L, SENT))
        V = Vecs(arena, n)
        alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
        if kernel == "update_xr":
            a = [V.put("p", p), V.put("Ap", Ap), V.put("x", x), V.put("r", r)]
            want = dict(zip(("x", "r"), bc.cg_update_xr(alpha, p, Ap, x, r)))
        else:
            a = [V.put("Ap", Ap), V.put("r", r)]
            want = dict(r=bc.cg_update_r(alpha, Ap, r))
        hip.call(f"spmv_hip_cg_{kernel}_f64", ctx.h, cgws.h, 2, n, *a, None)
        part = peek(ctx, cgws.addr("partials"), L)
        if mode == "done":
            V.expect()
            assert np.all(part == SENT)
            untouched(cgws, snap)
            continue
        V.expect(**want)
        assert np.all(part[bc.stream_grid(n // 2, L):] == 0)
        hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 3, None)
        check_sum(kind, cgws.get("rr", 3), want["r"], want["r"], bc.depth(n, L))


@pytest.mark.parametrize("kernel", ["update_p", "update_xp", "flush_x"])
@pytest.mark.parametrize("mode", MODES)
def test_cg_update_p_side(ctx, arena, L, nt, cgws, kernel, mode):
    for n, kind in lengths(L):
        s = bc.cg_scalars(kind)
        r, x, p = (vec(kind, n, i) for i in (1, 2, 3))
        conv, snap = arm(cgws, s, mode)
        alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
        beta = bc.cg_beta(s["rr_new"], s["rr_prev"])
        V = Vecs(arena, n)
        if kernel == "update_p":
            a = [V.put("r", r), V.put("p", p)]
            want = dict(p=p if conv else bc.cg_update_p(beta, r, p))
        elif kernel == "update_xp":
            a = [V.put("r", r), V.put("x", x), V.put("p", p)]
            want = dict(zip(("x", "p"),
                            bc.cg_update_xp(alpha, beta, conv, r, x, p)))
        else:  # a P step's pending update, unless that step met the tolerance
            a = [V.put("p", p), V.put("x", x)]
            want = dict(x=x if conv else bc.axpy(alpha, p, x))
        hip.call(f"spmv_hip_cg_{kernel}_f64", ctx.h, cgws.h, 2, n, *a, None)
        if mode == "done":
            V.expect()
            untouched(cgws, snap)
        else:
            V.expect(**want)
            assert cgws.done() == 0  # raised by the next reduce_pAp alone


@pytest.mark.parametrize("two", [False, True], ids=["pAp", "pAp2"])
def test_cg_reducers(ctx, L, cgws, two):
    """partials -> pAp[k] / rr[k], and the done flag reduce_pAp raises"""
    p2 = ctx.empty(L, np.float64)
    for kind in ("E", "R"):
        a, b = vec(kind, L, 5), vec(kind, L, 6)
        cgws.reset(bc.RTOL_GO)
        cgws.set("rr", 0, 1.0)
        cgws.set("rr", 1, 1.0)
        poke(ctx, cgws.addr("partials"), a)
        p2.write(b)
        if two:
            hip.call("spmv_hip_cg_reduce_pAp2", ctx.h, cgws.h, 2, p2.ptr, None)
        else:
            hip.call("spmv_hip_cg_reduce_pAp", ctx.h, cgws.h, 2, None)
        terms = np.concatenate([a, b]) if two else a
        d = (2 if two else 1) * -(-L // bc.K_BLOCK) + 6 + 4
        check_sum(kind, cgws.get("pAp", 2), terms, np.ones(len(terms)), d,
                  roundings=0)
        assert cgws.done() == 0
        hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 2, None)
        check_sum(kind, cgws.get("rr", 2), a, np.ones(L),
                  -(-L // bc.K_BLOCK) + 10, roundings=0)
    # rr[1] met the tolerance: done, kstop = 1, pAp[2] not written
    cgws.reset(bc.RTOL_STOP)
    cgws.set("rr", 0, 1.0)
    cgws.set("rr", 1, 1.0)
    cgws.set("pAp", 2, SENT)
    hip.call("spmv_hip_cg_reduce_pAp", ctx.h, cgws.h, 2, None)
    flags = np.zeros(2, np.int32)
    hip.call("spmv_hip_cg_ws_read_async", cgws.h,
             flags.ctypes.data_as(C.c_void_p), None, 0, None)
    ctx.stream_sync()
    assert list(flags) == [1, 1] and cgws.get("pAp", 2) == SENT
    snap = cgws.history()
    hip.call("spmv_hip_cg_reduce_rr", ctx.h, cgws.h, 3, None)
    hip.call("spmv_hip_cg_reduce_pAp2", ctx.h, cgws.h, 3, p2.ptr, None)
    untouched(cgws, snap)
    p2.free()


@pytest.mark.parametrize("kernel", ["xp_cs", "p2_cs", "x2p_cs"])
@pytest.mark.parametrize("mode", MODES)
def test_cg_consumer_side(ctx, arena, L, nt, cgws, kernel, mode):
    """update_r_cs (producer of the r.r partials, which have no accessor) and
    one of its three consumers as a pair, iteration 2.  p.Ap arrives as
    partials with one non-zero entry per array, so pAp[2] is exact whatever
    the order; rr[2] is the device's own sum: held to its bound (E: exact),
    then taken as read for beta and the stopping test."""
    p2 = ctx.empty(L, np.float64)
    for n, kind in lengths(L):
        s = bc.cg_scalars(kind)
        if mode == "stop":  # same alpha; "go" keeps a beta of order 1
            s = dict(s, rr_prev=s["rr_prev"] * BIG, pAp=s["pAp"] * BIG)
        Ap, r, x, p, q = (vec(kind, n, i) for i in (1, 2, 3, 4, 5))
        conv, snap = arm(cgws, s, mode, pair=True)
        if mode != "done":
            cgws.set("pAp", 2, SENT)
            cgws.set("rr", 2, SENT)
        poke(ctx, cgws.addr("partials"), one_nonzero(L, s["pAp"] / 2, 5))
        p2.write(one_nonzero(L, s["pAp"] / 2, L - 1))
        alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
        alpha_prev = bc.cg_alpha(s["rr0"], s["pAp_prev"])
        V = Vecs(arena, n)
        pAp_, pr, px = V.put("Ap", Ap), V.put("r", r), V.put("x", x)
        pp = V.put("p", p)
        pq = V.put("q", q) if kernel == "x2p_cs" else (
            V.out("q") if kernel == "p2_cs" else None)
        hip.call("spmv_hip_cg_update_r_cs_f64", ctx.h, cgws.h, 2, n, pAp_, pr,
                 p2.ptr, None)
        if kernel == "xp_cs":
            hip.call("spmv_hip_cg_update_xp_cs_f64", ctx.h, cgws.h, 2, n, pr, px,
                     pp, None)
        elif kernel == "p2_cs":  # p_in = p, p_out = q
            hip.call("spmv_hip_cg_update_p2_cs_f64", ctx.h, cgws.h, 2, n, pr, px,
                     pp, pq, None)
        else:  # p_prev = q (written), p_cur = p
            hip.call("spmv_hip_cg_update_x2p_cs_f64", ctx.h, cgws.h, 2, n, pr,
                     px, pq, pp, None)
        if mode == "done":
            V.expect()
            untouched(cgws, snap)
            continue
        assert cgws.get("pAp", 2) == s["pAp"]
        rn = bc.cg_update_r(alpha, Ap, r)
        rr_new = cgws.get("rr", 2)
        check_sum(kind, rr_new, rn, rn, bc.depth(n, L))
        if n == 0:
            continue  # rr[2] = 0: beta and the test are 0 / x, nothing to move
        assert bc.converged(rr_new, s["rr0"], PAIR_RTOL[mode]) == conv
        beta = bc.cg_beta(rr_new, s["rr_prev"])
        if kernel == "xp_cs":
            xn, pn = bc.cg_update_xp(alpha, beta, conv, rn, x, p)
            V.expect(r=rn, x=xn, p=pn)
        elif kernel == "p2_cs":
            # x only when this iteration converges; then nothing is pending
            # and p_out is not written
            xn = bc.axpy(alpha, p, x) if conv else x
            qn = np.full(n, SENT) if conv else bc.cg_update_p(beta, rn, p)
            V.expect(r=rn, x=xn, q=qn)
        else:
            xn, qn = bc.cg_update_x2p(alpha_prev, alpha, beta, conv, rn, x, q, p)
            V.expect(r=rn, x=xn, q=qn)
    p2.free()


@pytest.mark.parametrize("family", ["cg", "pcg", "bicg", "cheb"])
def test_alpha_probe(ctx, arena, cgws, pcgws, bicgws, family):
    """generic scalars, x = 0, p = 1: x comes back as the device's alpha
    itself -- its square root and division against numpy's correctly rounded
    (sqrt(rr) * sqrt(rr)) / pAp, resp. the one division of the other families"""
    n = 3
    V = Vecs(arena, n)
    pr, px, pp = V.put("r", np.ones(n)), V.put("x", np.zeros(n)), \
        V.put("p", np.ones(n))
    rr, pap = 3.7000000000000002, 0.7310585786300049
    if family == "cg":
        cgws.reset(bc.RTOL_GO)
        cgws.set("rr", 0, 1.0), cgws.set("rr", 1, rr), cgws.set("pAp", 2, pap)
        cgws.set("rr", 2, 1.0)
        hip.call("spmv_hip_cg_update_xp_f64", ctx.h, cgws.h, 2, n, pr, px, pp,
                 None)
        want = bc.cg_alpha(rr, pap)
    elif family == "pcg":
        pd = V.put("dinv", np.ones(n))
        pcgws.install(dict(rr0=1.0, rz_prev=rr, pAp=pap, rz_new=1.0, rr_new=1.0),
                      bc.RTOL_GO)
        hip.call("spmv_hip_pcg_update_xp_f64", ctx.h, pcgws.h, 2, n, pr, pd, px,
                 pp, None)
        want = bc.pcg_alpha(rr, pap)
    elif family == "cheb":
        # cheb_update_xp: z = 0, so p comes back as beta; cheb_update_r and
        # sgs_update_r: r = 0, Ap = 1, so r comes back as -alpha
        rz_new = 1.9000000000000001
        pz = V.put("z", np.zeros(n))
        pcgws.install(dict(rr0=1.0, rz_prev=rr, pAp=pap, rz_new=rz_new,
                           rr_new=1.0), bc.RTOL_GO)
        hip.call("spmv_hip_cheb_update_xp_f64", ctx.h, pcgws.h, 2, n, pz, px, pp,
                 None)
        want = bc.pcg_alpha(rr, pap)
        assert bc.same_bits(peek(ctx, px, n), np.full(n, want))
        assert bc.same_bits(peek(ctx, pp, n),
                            np.full(n, bc.pcg_beta(rz_new, rr)))
        for name, extra in (("sgs_update_r", ()), ("cheb_update_r", None)):
            W = Vecs(arena, n)
            qa, qr = W.put("Ap", np.ones(n)), W.put("r", np.zeros(n))
            qz = W.out("z")
            if extra is None:
                hip.call("spmv_hip_cheb_update_r_f64", ctx.h, pcgws.h, 2, n, 1.0,
                         qa, None, qr, None, qz, None)
            else:
                hip.call("spmv_hip_sgs_update_r_f64", ctx.h, pcgws.h, 2, n, qa,
                         qr, None)
            assert bc.same_bits(peek(ctx, qr, n), np.full(n, -want)), name
        return
    else:
        pt = V.put("t", np.zeros(n))
        po = V.out("rout")
        bicgws.install(dict(rr0=1.0, rho_prev=rr, rv=pap, ts=0.0, tt=1.0,
                            rr_new=1.0, rho_new=1.0), bc.RTOL_GO)
        # ph = p (ones), s = r, omega = 0: x = 0 + alpha * 1 + 0 * s
        hip.call("spmv_hip_bicg_update_xr_f64", ctx.h, bicgws.h, 2, n, pp, None,
                 pr, pt, pr, px, po, None)
        want = bc.pcg_alpha(rr, pap)
    got = peek(ctx, px, n)
    assert bc.same_bits(got, np.full(n, want)), (got[0].hex(), float(want).hex())


# ---------------------------------------------------------------------------
# blas1_pcg.hip
# ---------------------------------------------------------------------------
def pcg_pair(ws, k):
    return ws.get("rz_rr", k)


def test_pcg_init(ctx, arena, L, nt, pcgws):
    for n, kind in lengths(L):
        b, dinv = vec(kind, n, 1), dinv_of(kind, n)
        pcgws.reset(bc.RTOL_GO)
        V = Vecs(arena, n)
        pb, pd = V.put("b", b, 1), V.put("dinv", dinv, 1)
        pr, pp, px = V.out("r"), V.out("p"), V.out("x")
        hip.call("spmv_hip_pcg_init_f64", ctx.h, pcgws.h, n, pb, pd, pr, pp, px,
                 None)
        hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 0, None)
        z = dinv * b
        V.expect(r=b, p=z, x=np.zeros(n))
        rz, rr = pcg_pair(pcgws, 0)
        d = bc.depth(n, L, streaming=False)
        check_sum(kind, rz, b, z, d)
        check_sum(kind, rr, b, b, d)


@pytest.mark.parametrize("cs", [False, True], ids=["plain", "cs"])
@pytest.mark.parametrize("mode", MODES)
def test_pcg_updates(ctx, arena, L, nt, pcgws, cs, mode):
    """update_r (+ reduce_rz_rr) then update_xp, or the consumer-side pair
    (whose r.z / r.r partials have no accessor: the pair 2 is observed)."""
    p2 = ctx.empty(L, np.float64)
    for n, kind in lengths(L):
        s = bc.pcg_scalars(kind)
        Ap, r, x, p = (vec(kind, n, i) for i in (1, 2, 3, 4))
        dinv = dinv_of(kind, n)
        conv, snap = arm(pcgws, s, mode, pair=True)
        if mode != "done":
            pcgws.set("rz_rr", 2, SENT, SENT)
            if cs:
                pcgws.set("pAp", 2, SENT)
        poke(ctx, pcgws.addr("partials"), one_nonzero(L, s["pAp"] / 2, 3))
        p2.write(one_nonzero(L, s["pAp"] / 2, L - 2))
        V = Vecs(arena, n)
        pa, pr, px, pp = V.put("Ap", Ap), V.put("r", r), V.put("x", x), \
            V.put("p", p)
        pd = V.put("dinv", dinv)
        if cs:
            hip.call("spmv_hip_pcg_update_r_cs_f64", ctx.h, pcgws.h, 2, n, pa, pd,
                     pr, p2.ptr, None)
            hip.call("spmv_hip_pcg_update_xp_cs_f64", ctx.h, pcgws.h, 2, n, pr,
                     pd, px, pp, None)
        else:
            hip.call("spmv_hip_pcg_update_r_f64", ctx.h, pcgws.h, 2, n, pa, pd,
                     pr, None)
            hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 2, None)
            hip.call("spmv_hip_pcg_update_xp_f64", ctx.h, pcgws.h, 2, n, pr, pd,
                     px, pp, None)
        if mode == "done":
            V.expect()
            untouched(pcgws, snap)
            continue
        if cs:
            assert pcgws.get("pAp", 2) == s["pAp"]
        alpha = bc.pcg_alpha(s["rz_prev"], s["pAp"])
        rn, zn = bc.pcg_update_r(alpha, Ap, dinv, r)
        rz, rr = pcg_pair(pcgws, 2)
        d = bc.depth(n, L)
        check_sum(kind, rz, rn, zn, d)
        check_sum(kind, rr, rn, rn, d)
        if n == 0:
            continue
        assert bc.converged(rr, s["rr0"], PAIR_RTOL[mode]) == conv
        xn, pn = bc.pcg_update_xp(alpha, bc.pcg_beta(rz, s["rz_prev"]), conv,
                                  rn, dinv, x, p)
        V.expect(r=rn, x=xn, p=pn)
    p2.free()


@pytest.mark.parametrize("two", [False, True], ids=["pAp", "pAp2"])
def test_pcg_reducers(ctx, L, pcgws, two):
    p2 = ctx.empty(L, np.float64)
    for kind in ("E", "R"):
        a, b = vec(kind, L, 5), vec(kind, L, 6)
        pcgws.install(bc.pcg_scalars(kind), bc.RTOL_GO)
        poke(ctx, pcgws.addr("partials"), a)
        p2.write(b)
        if two:
            hip.call("spmv_hip_pcg_reduce_pAp2", ctx.h, pcgws.h, 2, p2.ptr, None)
        else:
            hip.call("spmv_hip_pcg_reduce_pAp", ctx.h, pcgws.h, 2, None)
        terms = np.concatenate([a, b]) if two else a
        d = (2 if two else 1) * -(-L // bc.K_BLOCK) + 10
        check_sum(kind, pcgws.get("pAp", 2), terms, np.ones(len(terms)), d,
                  roundings=0)
        assert pcgws.done() == 0
    # rr[0] == 0 stops the solve at k = 0 (reduce_pAp(1)); pAp[1] stays
    pcgws.reset(bc.RTOL_GO)
    pcgws.set("pAp", 1, SENT)
    hip.call("spmv_hip_pcg_reduce_pAp", ctx.h, pcgws.h, 1, None)
    flags = np.zeros(2, np.int32)
    hip.call("spmv_hip_pcg_ws_read_async", pcgws.h,
             flags.ctypes.data_as(C.c_void_p), None, 0, None)
    ctx.stream_sync()
    assert list(flags) == [1, 0] and pcgws.get("pAp", 1) == SENT
    snap = pcgws.history()
    hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 2, None)
    hip.call("spmv_hip_pcg_reduce_pAp2", ctx.h, pcgws.h, 2, p2.ptr, None)
    untouched(pcgws, snap)
    p2.free()


# ---------------------------------------------------------------------------
# blas1_bicgstab.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "dinv"])
def test_bicg_init(ctx, arena, L, nt, bicgws, pre):
    for n, kind in lengths(L):
        b = vec(kind, n, 1)
        dinv = dinv_of(kind, n) if pre else None
        bicgws.reset(bc.RTOL_GO)
        V = Vecs(arena, n)
        pb = V.put("b", b, 1)
        pd = V.put("dinv", dinv, 1) if pre else None
        pr, ph_, pp, px = V.out("r"), V.out("rhat"), V.out("p"), V.out("x")
        pph = V.out("ph")
        hip.call("spmv_hip_bicg_init_f64", ctx.h, bicgws.h, n, pb, pd, pr, ph_,
                 pp, pph if pre else None, px, None)
        hip.call("spmv_hip_bicg_reduce_rr_rho", ctx.h, bicgws.h, 0, None)
        want = dict(r=b, rhat=b, p=b, x=np.zeros(n))
        if pre:
            want["ph"] = dinv * b
        V.expect(**want)
        rr, rho = bicgws.get("rr_rho", 0)
        d = bc.depth(n, L, streaming=False)
        check_sum(kind, rr, b, b, d)
        assert rr.tobytes() == rho.tobytes()  # both halves take the same sums


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "dinv"])
@pytest.mark.parametrize("cs", [False, True], ids=["plain", "cs"])
@pytest.mark.parametrize("mode", MODES)
def test_bicg_iteration(ctx, arena, L, nt, bicgws, pre, cs, mode):
    """One iteration's six passes, each checked on its own vectors: dot_rv ->
    [reduce_rv] update_s -> dot_ts_tt -> [reduce_ts_tt] update_xr ->
    [reduce_rr_rho] update_p.  No partial array of BiCGStab has an accessor:
    the plain form observes what the reducers install, the consumer-side form
    what the consumers store.  rv, ts, tt, rr, rho are the device's own sums,
    held to their bounds (E: exact integers), then taken as read."""
    sfx = "_cs" if cs else ""
    for n, kind in lengths(L):
        if n == 0:
            continue  # rhat.v = 0 is breakdown 1; n = 0 runs in test_bicg_init
        if kind == "E" and n > 2 * bc.UNIT + 1 and mode != "go":
            continue  # the branches do not depend on the length: wrap once
        s = bc.bicg_scalars(kind)
        rhat, v, r, t = (vec(kind, n, i) for i in (1, 2, 3, 4))
        dinv = dinv_of(kind, n) if pre else None
        conv, snap = arm(bicgws, s, mode, pair=True)
        rtol = PAIR_RTOL[mode]
        if kind == "E" and mode != "done":
            # rv[2] will be the integer rhat.v: rho[1] = 2 rv makes alpha 2
            s = dict(s, rho_prev=2.0 * bc.exact_dot_int(rhat, v))
            bicgws.set("rr_rho", 1, s["rr0"], s["rho_prev"])

        # -- dot_rv, update_s ------------------------------------------------
        V = Vecs(arena, n)
        prh, pv, pr = V.put("rhat", rhat), V.put("v", v), V.put("r", r)
        pd = V.put("dinv", dinv) if pre else None
        ps, psh = V.out("s"), V.out("sh")
        hip.call("spmv_hip_bicg_dot_rv_f64", ctx.h, bicgws.h, 2, n, prh, pv, None)
        if not cs:
            hip.call("spmv_hip_bicg_reduce_rv", ctx.h, bicgws.h, 2, None)
        elif mode != "done":
            bicgws.set("rv", 2, SENT)
        hip.call(f"spmv_hip_bicg_update_s{sfx}_f64", ctx.h, bicgws.h, 2, n, pr,
                 pv, pd, ps, psh if pre else None, None)
        if mode == "done":
            V.expect()
            untouched(bicgws, snap)
        rv = bicgws.get("rv", 2)
        if mode != "done":
            check_sum(kind, rv, rhat, v, bc.depth(n, L))
        if mode == "done":
            sv, sh = r, (dinv * r if pre else None)
        else:
            alpha = bc.pcg_alpha(s["rho_prev"], rv)
            sv, sh = bc.bicg_update_s(alpha, r, v, dinv)
            V.expect(s=sv, **({"sh": sh} if pre else {}))

        # -- dot_ts_tt, update_xr -----------------------------------------------
        ph, x = vec(kind, n, 5), vec(kind, n, 6)
        if kind == "E" and cs:
            # the consumer forms omega from its own sums: t on the even
            # elements, s = 4 t + w with w on the odd ones, so t.s = 4 t.t and
            # omega is 4 exactly (dot_ts_tt itself sees a generic t without cs)
            even = np.arange(n) % 2 == 0
            t = np.where(even, t, 0.0)
            sv = 4.0 * t + np.where(even, 0.0, vec(kind, n, 8))
            sh = dinv * sv if pre else None
        V = Vecs(arena, n)
        pt, ps = V.put("t", t), V.put("s", sv)
        psh = V.put("sh", sh) if pre else None
        pph, prh, px = V.put("ph", ph), V.put("rhat", rhat), V.put("x", x)
        pr = V.out("r")
        hip.call("spmv_hip_bicg_dot_ts_tt_f64", ctx.h, bicgws.h, 2, n, pt, ps,
                 None)
        d = bc.depth(n, L)

        def check_ts_tt():
            ts, tt = bicgws.get("ts_tt", 2)
            check_sum(kind, ts, t, sv, d)
            check_sum(kind, tt, t, t, d)

        if not cs:
            hip.call("spmv_hip_bicg_reduce_ts_tt", ctx.h, bicgws.h, 2, None)
            if mode != "done":
                check_ts_tt()
                if kind == "E":  # checked; now an omega of 4 keeps r integer
                    bicgws.set("ts_tt", 2, 8.0, 2.0)
        elif mode != "done":
            bicgws.set("ts_tt", 2, SENT, SENT)
        hip.call(f"spmv_hip_bicg_update_xr{sfx}_f64", ctx.h, bicgws.h, 2, n, pph,
                 psh, ps, pt, prh, px, pr, None)
        if not cs:
            hip.call("spmv_hip_bicg_reduce_rr_rho", ctx.h, bicgws.h, 2, None)
        if mode == "done":
            V.expect()
            untouched(bicgws, snap)
            rn = r
        elif cs:
            check_ts_tt()
        if mode != "done":
            omega = bc.bicg_omega(*bicgws.get("ts_tt", 2))
            xn, rn = bc.bicg_update_xr(alpha, omega, ph, sh, sv, t, x)
            V.expect(x=xn, r=rn)

        # -- update_p -------------------------------------------------------------
        p = vec(kind, n, 7)
        V = Vecs(arena, n)
        pr, pv, pp = V.put("r", rn), V.put("v", v), V.put("p", p)
        pd = V.put("dinv", dinv) if pre else None
        pph = V.out("ph")
        if cs and mode != "done":
            bicgws.set("rr_rho", 2, SENT, SENT)
        hip.call(f"spmv_hip_bicg_update_p{sfx}_f64", ctx.h, bicgws.h, 2, n, pr,
                 pv, pd, pp, pph if pre else None, None)
        if mode == "done":
            V.expect()
            untouched(bicgws, snap)
            continue
        rr, rho = bicgws.get("rr_rho", 2)
        check_sum(kind, rr, rn, rn, d)
        check_sum(kind, rho, rhat, rn, d)
        assert bc.converged(rr, s["rr0"], rtol) == conv
        flags = np.zeros(3, np.int32)
        hip.call("spmv_hip_bicg_ws_read_async", bicgws.h,
                 flags.ctypes.data_as(C.c_void_p), None, 0, None)
        ctx.stream_sync()
        if conv:  # x and r updated, p not; update_p raises done itself
            V.expect()
            assert list(flags) == [1, 2, 0]
        elif omega == 0.0 or rho == 0.0:
            # breakdown 2: no beta, p stays.  With one element r = s - (t s /
            # t t) t is zero by construction, so n = 1 ends here by right.
            V.expect()
            assert list(flags) == [1, 2, 2]
        else:
            beta = bc.bicg_beta(rho, s["rho_prev"], alpha, omega)
            pn, phn = bc.bicg_update_p(beta, omega, rn, v, dinv, p)
            V.expect(p=pn, **({"ph": phn} if pre else {}))
            assert list(flags)[0] == 0


# ---------------------------------------------------------------------------
# blas1_cheb.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "dinv"])
@pytest.mark.parametrize("last", [False, True], ids=["more", "last"])
def test_cheb_apply0_and_step(ctx, arena, L, nt, pcgws, pre, last):
    for n, kind in lengths(L):
        s = bc.cheb_scalars(kind)
        r, w, d0, z0 = (vec(kind, n, i) for i in (1, 2, 3, 4))
        dinv = dinv_of(kind, n) if pre else None
        V = Vecs(arena, n)
        pr = V.put("r", r)
        pd = V.put("dinv", dinv) if pre else None
        pdd, pz = V.out("d"), V.out("z")
        hip.call("spmv_hip_cheb_apply0_f64", ctx.h, n, s["b0"], pr, pd,
                 None if last else pdd, pz, None)
        t0 = bc.cheb_apply0(s["b0"], r, dinv)
        V.expect(z=t0, **({} if last else {"d": t0}))
        # a later step: without a workspace, and inside a solve (last: r.z)
        for ws in (None, pcgws):
            if ws is not None:
                ws.install(bc.pcg_scalars(kind), bc.RTOL_GO)
                ws.set("rz_rr", 3, SENT, SENT)
            V = Vecs(arena, n)
            pw, pr = V.put("w", w), V.put("r", r)
            pd = V.put("dinv", dinv) if pre else None
            pdd, pz = V.put("d", d0), V.put("z", z0)
            hip.call("spmv_hip_cheb_step_f64", ctx.h, None if ws is None else ws.h,
                     n, s["a"], s["b"], int(last), pw, pr, pd, pdd, pz, None)
            dn, zn = bc.cheb_step(s["a"], s["b"], w, r, dinv, d0, z0)
            V.expect(z=zn, **({} if last else {"d": dn}))
            if ws is not None and last:
                hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, ws.h, 3, None)
                check_sum(kind, pcg_pair(ws, 3)[0], r, zn, bc.depth(n, L))
        if kind == "E" and n == 513:  # after done: nothing moves
            pcgws.raise_done()
            V = Vecs(arena, n)
            pw, pr, pdd, pz = V.put("w", w), V.put("r", r), V.put("d", d0), \
                V.put("z", z0)
            hip.call("spmv_hip_cheb_step_f64", ctx.h, pcgws.h, n, s["a"], s["b"],
                     int(last), pw, pr, None, pdd, pz, None)
            V.expect()


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "dinv"])
@pytest.mark.parametrize("last", [False, True], ids=["more", "last"])
def test_cheb_init_and_update_r(ctx, arena, L, nt, pcgws, pre, last):
    for n, kind in lengths(L):
        s, ps_ = bc.cheb_scalars(kind), bc.pcg_scalars(kind)
        b, Ap = vec(kind, n, 1), vec(kind, n, 2)
        dinv = dinv_of(kind, n) if pre else None
        pcgws.reset(bc.RTOL_GO)
        V = Vecs(arena, n)
        pb = V.put("b", b, 1)
        pd = V.put("dinv", dinv, 1) if pre else None
        pr, px, pdd, pz = V.out("r"), V.out("x"), V.out("d"), V.out("z")
        hip.call("spmv_hip_cheb_init_f64", ctx.h, pcgws.h, n, s["b0"], pb, pd, pr,
                 px, None if last else pdd, pz, None)
        hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 0, None)
        t0 = bc.cheb_apply0(s["b0"], b, dinv)
        V.expect(r=b, x=np.zeros(n), z=t0, **({} if last else {"d": t0}))
        rz, rr = pcg_pair(pcgws, 0)
        d = bc.depth(n, L, streaming=False)
        check_sum(kind, rr, b, b, d)
        if last:
            check_sum(kind, rz, b, t0, d)
        for mode in ("go", "done"):
            _, snap = arm(pcgws, ps_, mode)
            V = Vecs(arena, n)
            pa, pr = V.put("Ap", Ap), V.put("r", b)
            pd = V.put("dinv", dinv) if pre else None
            pdd, pz = V.out("d"), V.out("z")
            hip.call("spmv_hip_cheb_update_r_f64", ctx.h, pcgws.h, 2, n, s["b0"],
                     pa, pd, pr, None if last else pdd, pz, None)
            if mode == "done":
                V.expect()
                untouched(pcgws, snap)
                continue
            hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 3, None)
            alpha = bc.pcg_alpha(ps_["rz_prev"], ps_["pAp"])
            rn = bc.cg_update_r(alpha, Ap, b)
            t0 = bc.cheb_apply0(s["b0"], rn, dinv)
            V.expect(r=rn, z=t0, **({} if last else {"d": t0}))
            rz, rr = pcg_pair(pcgws, 3)
            check_sum(kind, rr, rn, rn, bc.depth(n, L))
            if last:
                check_sum(kind, rz, rn, t0, bc.depth(n, L))


@pytest.mark.parametrize("mode", MODES)
def test_cheb_update_xp(ctx, arena, L, nt, pcgws, mode):
    for n, kind in lengths(L):
        s = bc.pcg_scalars(kind)
        z, x, p = (vec(kind, n, i) for i in (1, 2, 3))
        conv, snap = arm(pcgws, s, mode)
        V = Vecs(arena, n)
        pz, px, pp = V.put("z", z), V.put("x", x), V.put("p", p)
        hip.call("spmv_hip_cheb_update_xp_f64", ctx.h, pcgws.h, 2, n, pz, px, pp,
                 None)
        if mode == "done":
            V.expect()
            untouched(pcgws, snap)
            continue
        xn, pn = bc.cg_update_xp(bc.pcg_alpha(s["rz_prev"], s["pAp"]),
                                   bc.pcg_beta(s["rz_new"], s["rz_prev"]), conv,
                                   z, x, p)
        V.expect(x=xn, p=pn)


@pytest.mark.parametrize("mode", ["go", "done"])
def test_sgs_kernels(ctx, arena, L, nt, pcgws, mode):
    for n, kind in lengths(L):
        s = bc.pcg_scalars(kind)
        b, Ap, z = (vec(kind, n, i) for i in (1, 2, 3))
        if mode == "go":  # sgs_init has no stopping test: it starts a solve
            pcgws.reset(bc.RTOL_GO)
            V = Vecs(arena, n)
            pb, pr, px = V.put("b", b, 1), V.out("r"), V.out("x")
            hip.call("spmv_hip_sgs_init_f64", ctx.h, pcgws.h, n, pb, pr, px, None)
            hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 0, None)
            V.expect(r=b, x=np.zeros(n))
            check_sum(kind, pcg_pair(pcgws, 0)[1], b, b,
                      bc.depth(n, L, streaming=False))
        _, snap = arm(pcgws, s, mode)
        V = Vecs(arena, n)
        pa, pr, pz = V.put("Ap", Ap), V.put("r", b), V.put("z", z)
        hip.call("spmv_hip_sgs_update_r_f64", ctx.h, pcgws.h, 2, n, pa, pr, None)
        hip.call("spmv_hip_sgs_dot_rz_f64", ctx.h, pcgws.h, n, pr, pz, None)
        if mode == "done":
            V.expect()
            untouched(pcgws, snap)
            continue
        hip.call("spmv_hip_pcg_reduce_rz_rr", ctx.h, pcgws.h, 3, None)
        rn = bc.cg_update_r(bc.pcg_alpha(s["rz_prev"], s["pAp"]), Ap, b)
        V.expect(r=rn)
        rz, rr = pcg_pair(pcgws, 3)
        check_sum(kind, rr, rn, rn, bc.depth(n, L))
        check_sum(kind, rz, rn, z, bc.depth(n, L))


# ---------------------------------------------------------------------------
# blas1_block.hip
# ---------------------------------------------------------------------------
class CgbWs(Ws):
    prefix = "cgb"

    def __init__(self, ctx, nrhs):
        self.nrhs = nrhs
        self.slots = (("rr", nrhs), ("pAp", nrhs))
        super().__init__(ctx, nrhs)

    def state(self):
        st = np.zeros(17, np.int32)
        hip.call("spmv_hip_cgb_ws_read_async", self.h,
                 st.ctypes.data_as(C.c_void_p), 17, None, 0, None)
        self.ctx.stream_sync()
        return st

    def install(self, s, rtol, frozen=()):
        """iteration 3 about to run, the columns of `frozen` stopped in
        iteration 1 (reduce_pAp(2) finds their rr[1] below the tolerance)"""
        K = self.nrhs
        self.reset(rtol)
        col = lambda v, f: [f if c in frozen else v for c in range(K)]  # noqa: E731
        self.set("rr", 0, *col(s["rr0"], 1.0))
        self.set("rr", 1, *col(s["rr0"] * BIG, 2.0 ** -80))
        hip.call("spmv_hip_cgb_reduce_pAp", self.ctx.h, self.h, 2, None)
        self.set("pAp", 2, *col(s["pAp_prev"], 0.0))
        self.set("rr", 2, *col(s["rr_prev"], 0.0))
        self.set("pAp", 3, *col(s["pAp"], 0.0))
        self.set("rr", 3, *col(s["rr_new"], 0.0))
        st = self.state()
        assert [int(v) for v in st[1:1 + K]] == [int(c in frozen)
                                                 for c in range(K)]


def frozen_history_kept(ws, snap, frozen):
    """every rr[k][c], pAp[k][c] of a stopped column c as before the kernels"""
    now = ws.history().reshape(2, KMAX + 1, ws.nrhs)
    was = snap.reshape(2, KMAX + 1, ws.nrhs)
    for c in frozen:
        assert bc.same_bits(now[:, :, c], was[:, :, c]), f"column {c}"


@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 8])
def test_cgb_kernels(ctx, arena, L, nt, nrhs):
    """init, dot, update_r, update_xp and both reducers per column against the
    single-column references; with `frozen`, one column stopped beside a live
    neighbour (the same double2 at nrhs = 2, 4, 8): its x, r, p and history
    stay, the live columns match their references bit for bit."""
    ws = CgbWs(ctx, nrhs)
    K = nrhs
    cases = [(M, k) for M in bc.block_shapes(K, L, False) for k in ("E", "R")]
    frozen_at = {-(-513 // K)}
    if wraps_fit(L):
        cases += [(M, "E") for M in bc.block_shapes(K, L, True)]
        frozen_at.add(bc.block_shapes(K, L, True)[-1])
    for M, kind in cases:
        n = M * K
        s = bc.cg_scalars(kind)
        B, AP, X, P = (vec(kind, n, i) for i in (1, 2, 3, 4))
        col = lambda a, c: a[c::K]  # noqa: E731
        d_rows = bc.depth(M, L, streaming=False)
        d = max(bc.depth(n, L), d_rows)  # pair kernels: see blas1_cases.depth

        ws.reset(bc.RTOL_GO)
        V = Vecs(arena, n)
        pb, pr, pp, px = V.put("B", B, 1), V.out("R"), V.out("P"), V.out("X")
        hip.call("spmv_hip_cgb_init_f64", ctx.h, ws.h, M, pb, pr, pp, px, None)
        hip.call("spmv_hip_cgb_reduce_rr", ctx.h, ws.h, 0, None)
        V.expect(R=B, P=B, X=np.zeros(n))
        part = peek(ctx, ws.addr("partials"), L * K)
        assert np.all(part[bc.rows_grid(M, L) * K:] == 0)
        rr0 = np.atleast_1d(ws.get("rr", 0))
        for c in range(K):
            check_sum(kind, rr0[c], col(B, c), col(B, c), d_rows)

        for frozen in ((), (K // 2,)) if (M in frozen_at and K > 1) else ((),):
            live = [c for c in range(K) if c not in frozen]
            ws.install(s, bc.RTOL_GO, frozen)
            snap = ws.history()
            # -- dot + reduce_pAp (into slot 4, untouched so far) -------------
            V = Vecs(arena, n)
            pp, pa = V.put("P", P), V.put("AP", AP)
            poke(ctx, ws.addr("partials"), np.full(L * K, SENT))
            hip.call("spmv_hip_cgb_dot_f64", ctx.h, ws.h, M, pp, pa, None)
            hip.call("spmv_hip_cgb_reduce_pAp", ctx.h, ws.h, 4, None)
            V.expect()
            pap = np.atleast_1d(ws.get("pAp", 4))
            for c in range(K):
                if c in frozen:
                    assert pap[c] == 0.0  # keeps the zero of the reset
                else:
                    check_sum(kind, pap[c], col(P, c), col(AP, c), d)
            # -- update_r + reduce_rr --------------------------------------------
            V = Vecs(arena, n)
            pa, pr = V.put("AP", AP), V.put("R", B)
            hip.call("spmv_hip_cgb_update_r_f64", ctx.h, ws.h, 3, M, pa, pr, None)
            hip.call("spmv_hip_cgb_reduce_rr", ctx.h, ws.h, 4, None)
            alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
            Rn = B.copy()
            for c in live:
                Rn[c::K] = bc.cg_update_r(alpha, col(AP, c), col(B, c))
            V.expect(R=Rn)
            frozen_history_kept(ws, snap, frozen)
            rr4 = np.atleast_1d(ws.get("rr", 4))
            for c in range(K):
                if c in frozen:
                    assert rr4[c] == 0.0
                else:
                    check_sum(kind, rr4[c], col(Rn, c), col(Rn, c), d)
            # -- update_xp: go, then the converging iteration --------------------
            for stop in (False, True):
                ws.install(s, bc.RTOL_STOP if stop else bc.RTOL_GO, frozen)
                snap = ws.history()
                V = Vecs(arena, n)
                pr, px, pp = V.put("R", B), V.put("X", X), V.put("P", P)
                hip.call("spmv_hip_cgb_update_xp_f64", ctx.h, ws.h, 3, M, pr, px,
                         pp, None)
                Xn, Pn = X.copy(), P.copy()
                beta = bc.cg_beta(s["rr_new"], s["rr_prev"])
                for c in live:
                    Xn[c::K], Pn[c::K] = bc.cg_update_xp(
                        alpha, beta, stop, col(B, c), col(X, c), col(P, c))
                V.expect(X=Xn, P=Pn)
                frozen_history_kept(ws, snap, frozen)
    # all_done: nothing moves
    ws.install(bc.cg_scalars("E"), bc.RTOL_GO, tuple(range(K)))
    assert ws.state()[0] == 1
    snap = ws.history()
    M = 257
    n = M * K
    V = Vecs(arena, n)
    pa, pr, px, pp = (V.put(nm, vec("E", n, i))
                      for i, nm in enumerate(("AP", "R", "X", "P")))
    poke(ctx, ws.addr("partials"), np.full(L * K, SENT))
    hip.call("spmv_hip_cgb_dot_f64", ctx.h, ws.h, M, pp, pa, None)
    hip.call("spmv_hip_cgb_update_r_f64", ctx.h, ws.h, 3, M, pa, pr, None)
    hip.call("spmv_hip_cgb_update_xp_f64", ctx.h, ws.h, 3, M, pr, px, pp, None)
    hip.call("spmv_hip_cgb_reduce_rr", ctx.h, ws.h, 3, None)
    hip.call("spmv_hip_cgb_reduce_pAp", ctx.h, ws.h, 3, None)
    V.expect()
    assert np.all(peek(ctx, ws.addr("partials"), L * K) == SENT)
    assert bc.same_bits(ws.history(), snap)
    ws.close()


@pytest.mark.parametrize("nrhs", [2, 3], ids=["pair", "rows"])
def test_cgb_scalar_probe(ctx, arena, nrhs):
    """generic rr and pAp per column through col_nalpha and col_step: with
    R = 0, AP = 1 update_r returns -alpha_c; with X = 0, P = 1, R = 0 update_xp
    returns alpha_c in X and beta_c in P.  Against numpy's (sqrt(rr) *
    sqrt(rr)) / pAp and (sqrt(rr') * sqrt(rr')) / (sqrt(rr) * sqrt(rr))."""
    K, M = nrhs, 5
    n = M * K
    rr = [3.7000000000000002, 0.30000000000000004, 5.0999999999999996][:K]
    pap = [0.7310585786300049, 1.9000000000000001, 0.12300000000000001][:K]
    rr1 = [1.3, 2.2000000000000002, 0.69999999999999996][:K]
    ws = CgbWs(ctx, K)
    ws.reset(bc.RTOL_GO)  # iteration 1: rr[k-1] is rr[0]
    ws.set("rr", 0, *rr), ws.set("pAp", 1, *pap), ws.set("rr", 1, *rr1)
    alpha = np.array([bc.cg_alpha(a, b) for a, b in zip(rr, pap)])
    beta = np.array([bc.cg_beta(a, b) for a, b in zip(rr1, rr)])
    V = Vecs(arena, n)
    pa, pr = V.put("AP", np.ones(n)), V.put("R", np.zeros(n))
    hip.call("spmv_hip_cgb_update_r_f64", ctx.h, ws.h, 1, M, pa, pr, None)
    V.expect(R=np.tile(-alpha, M))
    V = Vecs(arena, n)
    pr, px, pp = V.put("R", np.zeros(n)), V.put("X", np.zeros(n)), \
        V.put("P", np.ones(n))
    hip.call("spmv_hip_cgb_update_xp_f64", ctx.h, ws.h, 1, M, pr, px, pp, None)
    V.expect(X=np.tile(alpha, M), P=np.tile(beta, M))
    ws.close()


def test_one_hot_cgb_dot_and_bicg_dot(ctx, arena, L, bicgws):
    """x = e_i through the two dot producers that have their own tails and
    epilogues: the reduced scalar is y_i in bits"""
    K, M = 2, bc.UNIT + 1
    n = M * K
    y = vec("R", n, 2)
    ws = CgbWs(ctx, K)
    ws.set("rr", 0, 1.0, 1.0)  # a column with rr[0] == 0 would stop at k = 1
    V = Vecs(arena, n)
    pp, pa = V.put("P", np.zeros(n)), V.put("AP", y)
    prev = None
    for i in bc.onehot_indices(n, L):
        if prev is not None:
            poke(ctx, pp + 8 * prev, [0.0])
        poke(ctx, pp + 8 * i, [1.0])
        prev = i
        hip.call("spmv_hip_cgb_dot_f64", ctx.h, ws.h, M, pp, pa, None)
        hip.call("spmv_hip_cgb_reduce_pAp", ctx.h, ws.h, 1, None)
        want = np.zeros(K)
        want[i % K] = y[i]
        assert bc.same_bits(ws.get("pAp", 1), want), i
    ws.close()
    n = 2 * bc.UNIT + 1
    y = vec("R", n, 3)
    bicgws.install(bc.bicg_scalars("R"), bc.RTOL_GO)
    V = Vecs(arena, n)
    pt, ps = V.put("t", np.zeros(n)), V.put("s", y)
    prev = None
    for i in bc.onehot_indices(n, L):
        if prev is not None:
            poke(ctx, pt + 8 * prev, [0.0])
        poke(ctx, pt + 8 * i, [1.0])
        prev = i
        hip.call("spmv_hip_bicg_dot_ts_tt_f64", ctx.h, bicgws.h, 2, n, pt, ps,
                 None)
        hip.call("spmv_hip_bicg_reduce_ts_tt", ctx.h, bicgws.h, 2, None)
        assert bc.same_bits(bicgws.get("ts_tt", 2), [y[i], 1.0]), i


def test_misaligned_vectors_are_refused(ctx, arena, L, cgws, pcgws, bicgws):
    """Every entry point whose header demands 16-byte alignment, each vector
    argument in turn 8 bytes off: SPMV_HIP_EINVAL, and no vector, partial or
    scalar is written.  The workspaces are armed, so a launch would show."""
    n, M = 513, 257
    cgbws = CgbWs(ctx, 2)
    cgws.install(bc.cg_scalars("E"), bc.RTOL_GO)
    pcgws.install(bc.pcg_scalars("E"), bc.RTOL_GO)
    bicgws.install(bc.bicg_scalars("E"), bc.RTOL_GO)
    cgbws.install(bc.cg_scalars("E"), bc.RTOL_GO)
    part = ctx.upload(np.full(L, SENT))
    V = Vecs(arena, 2 * M)  # 514 doubles: room for n = 513 one element off
    good = [V.put(f"v{i}", vec("E", 2 * M, i)) for i in range(7)]
    bad = V.put("off", vec("E", 2 * M, 7), off=1)
    c, p, b, g = cgws.h, pcgws.h, bicgws.h, cgbws.h
    table = [  # name, arguments before the vectors, vectors, arguments after
        ("dot_partial_f64", (n,), 2, (part.ptr,)),
        ("cg_dot_rr_f64", (c, n), 1, ()),
        ("cg_update_xr_f64", (c, 2, n), 4, ()),
        ("cg_update_p_f64", (c, 2, n), 2, ()),
        ("cg_update_r_f64", (c, 2, n), 2, ()),
        ("cg_update_xp_f64", (c, 2, n), 3, ()),
        ("cg_update_r_cs_f64", (c, 2, n), 2, (None,)),
        ("cg_update_xp_cs_f64", (c, 2, n), 3, ()),
        ("cg_update_p2_cs_f64", (c, 2, n), 4, ()),
        ("cg_update_x2p_cs_f64", (c, 2, n), 4, ()),
        ("cg_flush_x_f64", (c, 2, n), 2, ()),
        ("pcg_update_r_f64", (p, 2, n), 3, ()),
        ("pcg_update_xp_f64", (p, 2, n), 4, ()),
        ("pcg_update_r_cs_f64", (p, 2, n), 3, (None,)),
        ("pcg_update_xp_cs_f64", (p, 2, n), 4, ()),
        ("cheb_apply0_f64", (n, 2.0), 4, ()),
        ("cheb_step_f64", (p, n, 4.0, 2.0, 0), 5, ()),
        ("cheb_update_r_f64", (p, 2, n, 2.0), 5, ()),
        ("cheb_update_xp_f64", (p, 2, n), 3, ()),
        ("sgs_update_r_f64", (p, 2, n), 2, ()),
        ("sgs_dot_rz_f64", (p, n), 2, ()),
        ("bicg_dot_rv_f64", (b, 2, n), 2, ()),
        ("bicg_dot_ts_tt_f64", (b, 2, n), 2, ()),
        ("bicg_update_s_f64", (b, 2, n), 5, ()),
        ("bicg_update_s_cs_f64", (b, 2, n), 5, ()),
        ("bicg_update_xr_f64", (b, 2, n), 7, ()),
        ("bicg_update_xr_cs_f64", (b, 2, n), 7, ()),
        ("bicg_update_p_f64", (b, 2, n), 5, ()),
        ("bicg_update_p_cs_f64", (b, 2, n), 5, ()),
        ("cgb_dot_f64", (g, M), 2, ()),
        ("cgb_update_r_f64", (g, 3, M), 2, ()),
        ("cgb_update_xp_f64", (g, 3, M), 3, ()),
    ]
    snaps = [w.history() for w in (cgws, pcgws, bicgws, cgbws)]
    for w, width in ((cgws, 1), (pcgws, 1), (cgbws, 2)):
        poke(ctx, w.addr("partials"), np.full(L * width, SENT))
    for name, head, nvec, tail in table:
        for j in range(nvec):
            vecs = good[:nvec]
            vecs[j] = bad
            with pytest.raises(SpmvHipError) as err:
                hip.call("spmv_hip_" + name, ctx.h, *head, *vecs, *tail, None)
            assert err.value.code == EINVAL, (name, j)
    ctx.stream_sync()
    V.expect()
    assert np.all(part.numpy() == SENT)
    for w, snap in zip((cgws, pcgws, bicgws, cgbws), snaps):
        assert bc.same_bits(w.history(), snap) and w.done() == 0
    for w, width in ((cgws, 1), (pcgws, 1), (cgbws, 2)):
        assert np.all(peek(ctx, w.addr("partials"), L * width) == SENT)
    part.free()
    cgbws.close()
