"""Every kernel of blas1_gmres.hip launched ALONE through the C ABI, cached and
non-temporal (blas1_nt_min_elems), against the references of gmres_cases.py.

The basis lies in one allocation at a stride larger than n (the gap and the
guard words on either side hold a sentinel and must come back untouched), w and
the other vectors between guard words of their own; inputs must come back
unchanged, write-only buffers start as the sentinel.  Lengths:
blas1_cases.small_lengths() with the basis sizes 1, 2, 8 (the group), 9 and 64
on sets E and R, and blas1_cases.wrap_lengths(dot_blocks) on set E with the
basis size 9 (one full group and a group of one) -- a second trip of a
workgroup's loop does not depend on how many groups there are, and 64 vectors
of 32 MiB each would cost the suite minutes of uploads.

  multi_axpy, scale, combine, add, residual, diag: equality of bits
  multi_dot + reduce: set E equality of bits; set R inside
      blas1_cases.sum_bound(blas1_cases.depth(n, dot_blocks)) -- the depth is
      read off the kernel (gmres_cases.py), not measured (checked for one row
      of every group and the last row; w.w of the second pass for every basis
      size); a one-hot w picks v_i[e] for every i
  givens, solve_y, start: equality of bits with their restatements, driven
      with chosen scalars through every branch"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import gmres_cases as gc
from spmv_amd import hip
from spmv_amd._lib import SpmvHipError

pytestmark = pytest.mark.gpu

G = 16
NT_DEFAULT = 1 << 24
SENT = bc.SENTINEL
KMAX = 8
EINVAL = -1
H, CC, WW, CS, SN, GG, Y, RR, HIST, INV, PART, PART_WW = range(12)
M = gc.MAX_RESTART


def peek(ctx, ptr, count, dtype=np.float64):
    out = np.empty(count, dtype)
    hip.call("spmv_hip_copy_d2h_async", ctx.h, out.ctypes.data_as(C.c_void_p),
             ptr, out.nbytes, None)
    ctx.stream_sync()
    return out


def poke(ctx, ptr, values):
    values = np.ascontiguousarray(values, np.float64)
    if values.size:
        ctx.copy_h2d(ptr, values)


@pytest.fixture(scope="module")
def L(ctx):
    return ctx.dot_partials_len


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, ctx):
    ctx.set_option("blas1_nt_min_elems", request.param)
    yield request.param
    ctx.set_option("blas1_nt_min_elems", NT_DEFAULT)


class Ws:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        hip.call("spmv_hip_gmres_ws_create", ctx.h, KMAX, C.byref(self.h))
        self.reset()

    def reset(self, rtol=0.0, kmax=KMAX, restart=M):
        hip.call("spmv_hip_gmres_ws_reset", self.h, float(rtol), kmax, restart,
                 None)

    def addr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        hip.call("spmv_hip_gmres_ws_array", self.h, which, C.byref(p), C.byref(n))
        return p.value, n.value

    def set(self, which, values, at=0):
        poke(self.ctx, self.addr(which)[0] + 8 * at, values)

    def get(self, which, count=None, at=0):
        p, n = self.addr(which)
        full = peek(self.ctx, p, n)
        return full[at:] if count is None else full[at:at + count]

    def state(self, **kw):
        """install k, jn, done, finished"""
        hip.call("spmv_hip_gmres_ws_set_state", self.h, kw.get("k", 0),
                 kw.get("jn", 0), kw.get("done", 0), kw.get("finished", 0), None)

    def words(self):
        """dict(done, kstop, status, k, jn, finished)"""
        out = np.zeros(6, np.int32)
        hip.call("spmv_hip_gmres_ws_get_state", self.h,
                 out.ctypes.data_as(C.c_void_p), None)
        self.ctx.stream_sync()
        return dict(zip(("done", "kstop", "status", "k", "jn", "finished"),
                        (int(v) for v in out)))

    def scalars(self):
        """every double array of the state, for `nothing moved` checks"""
        return np.concatenate([self.get(w) for w in (H, CC, CS, SN, GG, Y, RR,
                                                     HIST, INV)])

    def close(self):
        hip.call("spmv_hip_gmres_ws_destroy", self.h)


@pytest.fixture(scope="module")
def ws(ctx):
    w = Ws(ctx)
    yield w
    w.close()


class Guarded:
    """vectors of n doubles `stride` apart between guard words"""

    def __init__(self, ctx, rows, n, stride=None):
        self.ctx, self.n = ctx, n
        self.stride = stride if stride is not None else (n + 1) // 2 * 2
        self.rows = [np.array(r, np.float64) for r in rows]
        self.count = len(self.rows)
        img = np.full(2 * G + self.count * self.stride, SENT)
        for i, r in enumerate(self.rows):
            img[G + i * self.stride:G + i * self.stride + n] = r
        self.img = img
        self.buf = ctx.empty(len(img), np.float64)
        ctx.copy_h2d(self.buf.at(0), img)
        self.ptr = self.buf.at(G)
        # the basis at a wrap length is hundreds of MiB: it is downloaded once,
        # by the last check (final=True), the small ones by every check
        self.lazy = len(img) > (1 << 22)

    def row(self, i):
        return self.buf.at(G + i * self.stride)

    def check(self, what, final=False, **rows):
        """guards and gaps intact; row i equals rows["r<i>"] where given, else
        what was uploaded"""
        if self.lazy and not final and not rows:
            return
        got = peek(self.ctx, self.buf.at(0), len(self.img))
        want = self.img.copy()
        for key, r in rows.items():
            i = int(key[1:])
            want[G + i * self.stride:G + i * self.stride + self.n] = r
        if not bc.same_bits(got, want):
            bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
            raise AssertionError(f"{what}: {bad.size} words differ, first at "
                                 f"{bad[0] - G}: got {got[bad[0]]!r}, want "
                                 f"{want[bad[0]]!r}")

    def free(self):
        self.buf.free()


_POOL = {}


def vec(kind, n, seed):
    key = (kind, seed)
    if key not in _POOL or len(_POOL[key]) < n:
        gen = {"E": bc.exact_vec, "R": bc.round_vec, "dR": bc.round_dinv,
               "dE": bc.exact_dinv}[kind]
        _POOL[key] = gen(max(n, 2 * bc.UNIT + 1), seed)
    return _POOL[key][:n]


_EXACT = {}


def exact_dot_cached(key, a, b):
    if key not in _EXACT:
        _EXACT[key] = bc.exact_dot(a, b)
    return _EXACT[key]


def wraps_fit(L):
    return bc.wrap_length(L) <= bc.WRAP_MAX


def cases(L):
    out = [(n, kind, nv) for n in bc.small_lengths() for kind in ("E", "R")
           for nv in gc.BASIS_SIZES]
    if wraps_fit(L):
        out += [(n, "E", 9) for n in bc.wrap_lengths(L)]
    return out


def coefs(kind, nv, seed):
    if kind == "E":
        return np.random.default_rng(seed).choice([-2.0, -1.0, 1.0, 2.0, 4.0], nv)
    return bc.round_vec(nv, 50 + seed) / 64.0


def basis(kind, n, nv):
    """nv vectors from a handful of pools (rotated, so rows differ)"""
    return [np.roll(vec(kind, n, 10 + i % 7), i // 7) for i in range(nv)]


def call(name, *a):
    hip.call("spmv_hip_gmres_" + name, *a)


def dot_rows(ctx, ws, V, w, nv, which=H):
    n = V.n
    call("multi_dot_f64", ctx.h, ws.h, n, V.ptr, V.stride, nv, w.ptr, None)
    call("reduce", ctx.h, ws.h, which, nv, None)
    return ws.get(which, nv)


def test_vector_kernels(ctx, ws, L, nt):
    for n, kind, nv in cases(L):
        what = (n, kind, nv)
        rows = basis(kind, n, nv)
        wv = vec(kind, n, 3)
        V = Guarded(ctx, rows, n, stride=(n + 1) // 2 * 2 + 2)
        w = Guarded(ctx, [wv], n)
        ws.reset()
        # -- multi_dot + reduce (first pass -> H)
        ws.set(H, np.full(M, SENT))
        ws.set(PART, np.full(M * L, SENT))
        got = dot_rows(ctx, ws, V, w, nv)
        V.check(what), w.check(what)
        part = ws.get(PART).reshape(M, L)
        g = bc.stream_grid(n // 2, L)
        assert np.all(part[:nv, g:] == 0) and np.all(part[nv:] == SENT), what
        assert np.all(ws.get(H, M - nv, nv) == SENT) if nv < M else True
        for i in range(nv):
            if kind == "E":
                assert float(got[i]) == float(bc.exact_dot_int(rows[i], wv)), what
            elif i % gc.GROUP == 0 or i == nv - 1:
                # one row of every group and the last row (exact rational sums
                # are slow; computed once for both instantiations)
                ex, sa = exact_dot_cached(("v.w", n, nv, i), rows[i], wv)
                assert bc.sum_within(got[i], ex, sa, bc.depth(n, L)), (what, i)
        # -- multi_axpy, first pass (coef = H)
        h = coefs(kind, nv, 1)
        c = coefs(kind, nv, 2)
        ws.set(H, h)
        ws.set(CC, c)
        call("multi_axpy_f64", ctx.h, ws.h, 0, n, V.ptr, V.stride, nv, w.ptr,
             None)
        w1 = gc.gmres_multi_axpy(rows, h, wv)
        V.check(what), w.check(what, r0=w1)
        assert bc.same_bits(ws.get(H, nv), h), what
        # -- second pass (coef = C ; H += C ; partials of w.w)
        ws.set(PART_WW, np.full(L, SENT))
        call("multi_axpy_f64", ctx.h, ws.h, 1, n, V.ptr, V.stride, nv, w.ptr,
             None)
        w2 = gc.gmres_multi_axpy(rows, c, w1)
        V.check(what), w.check(what, r0=w2)
        assert bc.same_bits(ws.get(H, nv), h + c), what
        assert bc.same_bits(ws.get(CC, nv), c), what
        pw = ws.get(PART_WW)
        assert np.all(pw[g:] == 0), what
        call("reduce", ctx.h, ws.h, WW, 1, None)
        ww = ws.get(WW)[0]
        if kind == "E":
            assert float(ww) == float(bc.exact_dot_int(w2, w2)), what
        else:
            ex, sa = exact_dot_cached(("w.w", n, nv), w2, w2)
            assert bc.sum_within(ww, ex, sa, bc.depth(n, L)), what
        # -- scale, out of place and in place
        inv = 0.25 if kind == "E" else 0.7310585786
        ws.set(INV, [inv])
        out = Guarded(ctx, [np.full(n, SENT)], n)
        call("scale_f64", ctx.h, ws.h, n, w.ptr, out.ptr, None)
        out.check(what, r0=gc.gmres_scale(inv, w2)), w.check(what, r0=w2)
        call("scale_f64", ctx.h, ws.h, n, out.ptr, out.ptr, None)
        out.check(what, r0=gc.gmres_scale(inv, gc.gmres_scale(inv, w2)))
        # -- combine (jn = nv), add, residual, diag
        y = coefs(kind, nv, 4)
        ws.set(Y, y)
        ws.state(k=1, jn=nv)
        poke(ctx, out.ptr, np.full(n, SENT))
        call("combine_f64", ctx.h, ws.h, n, V.ptr, V.stride, out.ptr, None)
        u = gc.gmres_combine(rows, y)
        V.check(what), out.check(what, r0=u)
        call("add_f64", ctx.h, ws.h, n, out.ptr, w.ptr, None)
        out.check(what, r0=u), w.check(what, r0=gc.gmres_add(u, w2))
        ws.state()
        bvec = Guarded(ctx, [vec(kind, n, 5), vec(kind, n, 6)], n)
        for ax in (None, bvec.row(1)):
            poke(ctx, out.ptr, np.full(n, SENT))
            call("residual_f64", ctx.h, ws.h, n, bvec.row(0), ax, out.ptr, None)
            r = gc.gmres_residual(bvec.rows[0], None if ax is None
                                  else bvec.rows[1])
            bvec.check(what), out.check(what, r0=r)
            call("reduce", ctx.h, ws.h, WW, 1, None)
            if kind == "E":
                assert float(ws.get(WW)[0]) == float(bc.exact_dot_int(r, r)), what
        dv = Guarded(ctx, [vec("d" + kind, n, 0)], n)
        call("diag_f64", ctx.h, n, dv.ptr, bvec.row(0), out.ptr, None)
        out.check(what, r0=gc.gmres_diag(dv.rows[0], bvec.rows[0]))
        dv.check(what), bvec.check(what), V.check(what, final=True)
        for b in (V, w, out, bvec, dv):
            b.free()


def test_multi_dot_one_hot(ctx, ws, L, nt):
    """w = e_i: the reduced dot is v_j[i] in bits for every j -- a dropped tail
    or a group boundary error moves one of them"""
    big = bc.wrap_lengths(L)[-1] if wraps_fit(L) else 0
    shapes = [(n, nv) for n in (3, 2 * bc.K_BLOCK + 1, 2 * bc.UNIT + 1)
              for nv in gc.BASIS_SIZES] + ([(big, 9)] if big else [])
    ws.reset()
    for n, nv in shapes:
        kind = "R" if n <= 2 * bc.UNIT + 1 else "E"
        rows = basis(kind, n, nv)
        V = Guarded(ctx, rows, n, stride=(n + 1) // 2 * 2 + 2)
        w = Guarded(ctx, [np.zeros(n)], n)
        prev = None
        for i in bc.onehot_indices(n, L):
            if prev is not None:
                poke(ctx, w.ptr + 8 * prev, [0.0])
            poke(ctx, w.ptr + 8 * i, [1.0])
            prev = i
            got = dot_rows(ctx, ws, V, w, nv, which=CC)
            want = np.array([r[i] for r in rows])
            assert bc.same_bits(got, want), (n, nv, i)
        V.free(), w.free()


def test_done_and_finished_freeze_the_kernels(ctx, ws, L, nt):
    n, nv = 2 * bc.UNIT + 1, 9
    rows = basis("R", n, nv)
    V = Guarded(ctx, rows, n, stride=n + 3)
    w = Guarded(ctx, [vec("R", n, 3)], n)
    out = Guarded(ctx, [np.full(n, SENT)], n)
    ws.reset()
    ws.set(H, coefs("R", M, 1)), ws.set(CC, coefs("R", M, 2))
    ws.set(Y, coefs("R", M, 4)), ws.set(INV, [0.5])
    ws.set(PART, np.full(M * L, SENT)), ws.set(PART_WW, np.full(L, SENT))
    ws.set(GG, coefs("R", M + 1, 6))
    # done, not finished: the Arnoldi kernels return at once ...
    ws.state(k=3, jn=nv, done=1)
    snap, words = ws.scalars(), ws.words()
    call("multi_dot_f64", ctx.h, ws.h, n, V.ptr, V.stride, nv, w.ptr, None)
    call("reduce", ctx.h, ws.h, H, nv, None)
    call("reduce", ctx.h, ws.h, WW, 1, None)
    for second in (0, 1):
        call("multi_axpy_f64", ctx.h, ws.h, second, n, V.ptr, V.stride, nv,
             w.ptr, None)
    call("givens", ctx.h, ws.h, 2, 0, None)
    call("start", ctx.h, ws.h, 0, 0, None)
    call("scale_f64", ctx.h, ws.h, n, w.ptr, out.ptr, None)
    V.check("done"), w.check("done"), out.check("done")
    assert bc.same_bits(ws.scalars(), snap) and ws.words() == words
    assert np.all(ws.get(PART) == SENT) and np.all(ws.get(PART_WW) == SENT)
    # ... the cycle end still runs ...
    call("combine_f64", ctx.h, ws.h, n, V.ptr, V.stride, out.ptr, None)
    u = gc.gmres_combine(rows, ws.get(Y, nv))
    out.check("cycle end", r0=u)
    call("add_f64", ctx.h, ws.h, n, out.ptr, w.ptr, None)
    x1 = gc.gmres_add(u, w.rows[0])
    w.check("cycle end", r0=x1)
    # ... the residual kernel behind it raises `finished` and writes nothing ...
    call("residual_f64", ctx.h, ws.h, n, V.row(0), V.row(1), out.ptr, None)
    out.check("residual after done", r0=u)
    assert ws.words() == dict(words, finished=1)
    assert np.all(ws.get(PART_WW) == SENT)
    # ... and after it the cycle end is a no-op too
    call("solve_y", ctx.h, ws.h, None)
    call("combine_f64", ctx.h, ws.h, n, V.ptr, V.stride, w.ptr, None)
    call("add_f64", ctx.h, ws.h, n, out.ptr, w.ptr, None)
    w.check("finished", r0=x1), out.check("finished", r0=u)
    assert bc.same_bits(ws.scalars(), snap)
    # jn == 0: combine and add leave u and x alone
    ws.state(k=0, jn=0)
    call("combine_f64", ctx.h, ws.h, n, V.ptr, V.stride, w.ptr, None)
    call("add_f64", ctx.h, ws.h, n, out.ptr, w.ptr, None)
    w.check("jn = 0", r0=x1)
    for b in (V, w, out):
        b.free()


# ---- the scalar kernels ----------------------------------------------------------
def _drive_givens(ctx, ws, L, j, h, ww, cs, sn, g, hist0, k, kmax, rtol, reduced):
    ws.reset(rtol=rtol, kmax=kmax)
    ws.set(H, list(h) + [SENT] * (M - len(h)))
    ws.set(CS, list(cs) + [SENT] * (M - len(cs)))
    ws.set(SN, list(sn) + [SENT] * (M - len(sn)))
    ws.set(GG, list(g) + [SENT] * (M + 1 - len(g)))
    ws.set(HIST, [hist0] + [SENT] * KMAX)
    ws.set(INV, [SENT])
    if reduced:
        ws.set(WW, [ww])
        ws.set(PART_WW, np.full(L, SENT))
    else:
        p = np.zeros(L)
        p[5 % L] = ww
        ws.set(PART_WW, p)
        ws.set(WW, [SENT])
    ws.state(k=k, jn=j)
    call("givens", ctx.h, ws.h, j, reduced, None)
    return gc.gmres_givens(j, h, ww, cs, sn, g, hist0, k, kmax, rtol)


GIVENS_CASES = {
    # name: (j, h, ww, cs, sn, g, hist0, k, kmax, rtol)
    "first column, |a| >= |b|": (0, [2.5], 1.44, [], [], [3.0], 3.0, 0, 8, 0.0),
    "|b| > |a|": (0, [0.3], 6.25, [], [], [3.0], 3.0, 0, 8, 0.0),
    "b == 0 is lucky": (0, [2.5], 0.0, [], [], [3.0], 3.0, 0, 8, 0.0),
    "R_jj == 0": (0, [0.0], 0.0, [], [], [3.0], 3.0, 0, 8, 0.0),
    "stop at rtol": (0, [2.5], 1.44, [], [], [3.0], 3.0, 0, 8, 0.9),
    "k == kmax": (0, [2.5], 1.44, [], [], [3.0], 3.0, 7, 8, 0.0),
    "third column": (2, [0.7310585786, -1.3247179572, 2.2360679775], 0.6180339887,
                     [0.8, 0.6], [0.6, -0.8], [1.1, -0.7, 0.4142135623], 3.0, 2,
                     8, 0.0),
    "third column, R_jj == 0 after rotation": (
        2, [0.0, 0.0, 0.0], 0.0, [0.8, 0.6], [0.6, -0.8], [1.1, -0.7, 0.4], 3.0,
        2, 8, 0.0),
}


@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("name", sorted(GIVENS_CASES))
def test_givens(ctx, ws, L, name, reduced):
    j, h, ww, cs, sn, g, hist0, k, kmax, rtol = GIVENS_CASES[name]
    want = _drive_givens(ctx, ws, L, j, h, ww, cs, sn, g, hist0, k, kmax, rtol,
                         reduced)
    words = ws.words()
    assert words["done"] == int(want["done"]), (name, words)
    assert (words["k"], words["jn"]) == (want["k"], want["jn"]), (name, words)
    assert words["status"] == (want["status"] if want["done"] else 0), name
    if want["done"]:
        assert words["kstop"] == want["k"], (name, words)
    col = ws.get(RR, j + 1, at=j * M)
    if want["col"] is None:
        # the column is discarded: rotations, g and the history stay
        assert bc.same_bits(ws.get(CS, j), cs[:j]), name
        assert bc.same_bits(ws.get(GG, j + 1), g), name
        assert ws.get(CS, 1, at=j)[0] == SENT and ws.get(HIST)[k + 1] == SENT
    else:
        assert bc.same_bits(col, want["col"]), (name, col, want["col"])
        assert bc.same_bits(ws.get(CS, j + 1), want["cs"]), name
        assert bc.same_bits(ws.get(SN, j + 1), want["sn"]), name
        assert bc.same_bits(ws.get(GG, j + 2), want["g"]), name
        assert bc.same_bits(ws.get(HIST, 1, at=want["k"]), [want["res"]]), name
    inv = ws.get(INV)[0]
    assert inv == (SENT if want["inv"] is None else want["inv"]), (name, inv)


def test_every_branch_is_covered():
    seen = set()
    for j, h, ww, cs, sn, g, hist0, k, kmax, rtol in GIVENS_CASES.values():
        st = gc.gmres_givens(j, h, ww, cs, sn, g, hist0, k, kmax, rtol)
        seen.add((st["status"], st["done"], st["col"] is None))
    assert seen == {(0, False, False), (0, True, False), (1, True, False),
                    (2, True, True)}


@pytest.mark.parametrize("jn", [0, 1, 2, 9, 64])
def test_solve_y(ctx, ws, jn):
    rng = np.random.default_rng(jn)
    R = np.triu(rng.uniform(-1, 1, (M, M))) + 3.0 * np.eye(M)
    g = rng.uniform(-1, 1, M + 1)
    ws.reset()
    ws.set(RR, R.T.ravel())  # R_il at [l * 64 + i]
    ws.set(GG, g)
    ws.set(Y, np.full(M, SENT))
    ws.state(k=1, jn=jn)
    call("solve_y", ctx.h, ws.h, None)
    y = ws.get(Y)
    assert bc.same_bits(y[:jn], gc.gmres_solve_y(R, g, jn)), jn
    assert np.all(y[jn:] == SENT)
    assert bc.same_bits(ws.get(RR), R.T.ravel()) and bc.same_bits(ws.get(GG), g)


@pytest.mark.parametrize("reduced", [0, 1])
def test_start(ctx, ws, L, reduced):
    def drive(rr, first, k):
        ws.reset()
        ws.set(GG, np.full(M + 1, SENT))
        ws.set(HIST, [SENT] * (KMAX + 1))
        ws.set(INV, [SENT])
        p = np.zeros(L)
        p[L - 1] = rr
        ws.set(PART_WW, np.full(L, SENT) if reduced else p)
        ws.set(WW, [rr if reduced else SENT])
        ws.state(k=k, jn=3)
        call("start", ctx.h, ws.h, first, reduced, None)
        return ws.words()

    w = drive(6.25, 1, 0)
    assert (w["done"], w["jn"], w["k"]) == (0, 0, 0)
    assert ws.get(HIST)[0] == 2.5 and ws.get(HIST)[1] == SENT
    g = ws.get(GG)
    assert g[0] == 2.5 and np.all(g[1:] == 0.0) and ws.get(INV)[0] == 1.0 / 2.5
    w = drive(2.0, 0, 5)
    assert (w["done"], w["jn"], w["k"]) == (0, 0, 5)
    assert ws.get(HIST)[0] == SENT  # only the first cycle writes the history
    assert ws.get(GG)[0] == math.sqrt(2.0)
    assert ws.get(INV)[0] == 1.0 / math.sqrt(2.0)
    # r.r == 0: the solve is over, x is the answer
    w = drive(0.0, 1, 0)
    assert w == dict(done=1, kstop=0, status=0, k=0, jn=0, finished=1)
    assert ws.get(HIST)[0] == 0.0 and ws.get(INV)[0] == SENT
    w = drive(0.0, 0, 5)
    assert (w["done"], w["kstop"], w["finished"]) == (1, 5, 1)


def test_refusals(ctx, ws, L):
    n = 64
    V = Guarded(ctx, basis("E", n, 2), n)
    w = Guarded(ctx, [vec("E", n, 3)], n)

    def refused(name, *a):
        with pytest.raises(SpmvHipError) as err:
            call(name, *a)
        assert err.value.code == EINVAL, name

    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr, V.stride, 0, w.ptr, None)
    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr, V.stride, M + 1, w.ptr, None)
    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr, n - 2, 2, w.ptr, None)
    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr, n + 1, 2, w.ptr, None)
    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr + 8, V.stride, 1, w.ptr, None)
    refused("multi_dot_f64", ctx.h, ws.h, n, V.ptr, V.stride, 2, w.ptr + 8, None)
    refused("multi_axpy_f64", ctx.h, ws.h, 0, n, V.ptr, V.stride, 2, w.ptr + 8,
            None)
    refused("reduce", ctx.h, ws.h, CS, 1, None)
    refused("reduce", ctx.h, ws.h, WW, 2, None)
    refused("givens", ctx.h, ws.h, M, 0, None)
    refused("scale_f64", ctx.h, ws.h, n, w.ptr + 8, w.ptr, None)
    refused("add_f64", ctx.h, ws.h, n, w.ptr, V.ptr + 8, None)
    refused("residual_f64", ctx.h, ws.h, n, w.ptr + 8, None, V.ptr, None)
    with pytest.raises(SpmvHipError):
        hip.call("spmv_hip_gmres_ws_reset", ws.h, 0.0, KMAX + 1, 5, None)
    with pytest.raises(SpmvHipError):
        hip.call("spmv_hip_gmres_ws_reset", ws.h, 0.0, KMAX, M + 1, None)
    ctx.stream_sync()
    V.check("refused"), w.check("refused")
    V.free(), w.free()
