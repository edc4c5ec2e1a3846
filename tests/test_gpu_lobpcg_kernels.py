"""Every kernel of hip/blas1_lobpcg.hip alone through the C ABI, bit for bit
against its numpy restatement in lobpcg_cases.py: nev in {1, 2, 3, 4, 8} (the
native widths and the run-time width), the edge and wrap lengths of
blas1_cases.py (block_shapes: M = 0, 1, 2, 3, the workgroup and unit edges of
the interleaved array, and for the row kernels the lengths around one trip of
the largest grid, at every nev) with the edges of a Gram chunk (64 rows) and of
a workgroup of rows (256) added, the Gram kernel's own wrap (more chunks than
workgroups), aligned and 8-byte-offset blocks, cached and non-temporal accesses,
masks none / one column / all but one, P absent, and the Rayleigh-Ritz kernel
on hand-built pencils through every branch."""
import ctypes as C

import numpy as np
import pytest

import blas1_cases as bc
import lobpcg_cases as lc
from spmv_amd import _lib
from test_gpu_pcg import exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

HIST, THETA, COEF, GRAM, GPART, RN, RPART = range(7)
KMAX = 4


class Ws:
    def __init__(self, exec_, nev, rtol=1e-6, atol=0.0, largest=False):  # noqa: F811
        self.e, self.nev, self.ctx = exec_, nev, exec_.context
        self.h = C.c_void_p()
        _lib.call("spmv_hip_lobpcg_ws_create", self.ctx, KMAX, nev,
                  C.byref(self.h))
        self.reset(rtol, atol, largest)

    def reset(self, rtol=1e-6, atol=0.0, largest=False):
        _lib.call("spmv_hip_lobpcg_ws_reset", self.h, rtol, atol, KMAX,
                  int(largest), None)

    def array(self, which):
        p, n = C.c_void_p(), C.c_int64()
        _lib.call("spmv_hip_lobpcg_ws_array", self.h, which, C.byref(p),
                  C.byref(n))
        return p.value, n.value

    def get(self, which, count=None):
        p, n = self.array(which)
        self.e.synchronize()
        return self.e.copy_to_host(p, n if count is None else count)

    def put(self, which, values):
        p, _ = self.array(which)
        self.e.copy_from_host(p, np.ascontiguousarray(values, np.float64))

    def set_state(self, active, has_p, it=0, done=0):
        _lib.call("spmv_hip_lobpcg_ws_set_state", self.h, active, has_p, it,
                  done, None)

    def state(self):
        words = np.zeros(8, np.int32)
        _lib.call("spmv_hip_lobpcg_ws_read_async", self.h,
                  words.ctypes.data_as(C.c_void_p), None, 0, None, None)
        self.e.synchronize()
        return dict(zip(("done", "kstop", "status", "it", "active", "has_p",
                         "restarts", "basis"), words.tolist()))

    def gram_grid(self, M):
        g = C.c_int()
        _lib.call("spmv_hip_lobpcg_gram_grid", self.h, M, C.byref(g))
        return g.value

    def close(self):
        _lib.call("spmv_hip_lobpcg_ws_destroy", self.h)


class Blocks:
    """device blocks of M * nev doubles between sentinels, `off` doubles into
    a 16-byte aligned allocation (0: aligned, 1: 8 bytes off)"""

    def __init__(self, exec_, arrays, off):  # noqa: F811
        self.e, self.off = exec_, off
        self.n = arrays[0].size
        self.base, self.ptr = [], []
        for a in arrays:
            buf = np.full(self.n + 4, lc_sentinel())
            buf[off:off + self.n] = a.ravel()
            p = exec_.alloc(self.n + 4)
            exec_.copy_from_host(p, buf)
            self.base.append(p)
            self.ptr.append(p + 8 * off)

    def get(self, i, shape):
        buf = self.e.copy_to_host(self.base[i], self.n + 4)
        assert np.all(buf[:self.off] == lc_sentinel())
        assert np.all(buf[self.off + self.n:] == lc_sentinel())
        return buf[self.off:self.off + self.n].reshape(shape).copy()

    def close(self):
        for p in self.base:
            self.e.free(p)


def lc_sentinel():
    return -777.25


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64),
                                                 b.view(np.uint64))


def same_values(a, b):
    """bits, but +0.0 and -0.0 alike (a sum started from 0.0 never gives -0.0,
    a product may)"""
    return np.array_equal(np.asarray(a) + 0.0, np.asarray(b) + 0.0, equal_nan=True)


def _data(M, nev, nblocks, seed, cancel=False):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nblocks):
        a = rng.uniform(-1.0, 1.0, (M, nev))
        if cancel:  # partial sums that cancel: a wrong order shows
            a *= np.ldexp(1.0, rng.integers(-20, 21, (M, 1)))
            a[1::2] = -a[::2][:a[1::2].shape[0]] * (1.0 + 2.0 ** -30)
        out.append(a)
    return out


EXTRA = [63, 64, 65, 255, 256, 257, 512, 1331]  # chunk and workgroup edges


def _partials_len(exec_):  # noqa: F811
    n = C.c_int()
    _lib.call("spmv_hip_dot_partials_len", exec_.context, C.byref(n))
    return n.value


def lengths(nev, L):
    """rows: blas1_cases' small edges for blocks of nev columns, M = 0 included"""
    return sorted(set(bc.block_shapes(nev, L, False)) | set(EXTRA))


def wrap_lengths(nev, L, slot):
    """rows around one trip of the largest grid, every fourth from `slot` on
    (a case stays short); none where blas1_cases skips the wrap edges"""
    if bc.wrap_length(L) > bc.WRAP_MAX:
        return []
    return bc.block_shapes(nev, L, True)[slot::4]


# ---- gram ---------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", lc.NEV)
def test_gram(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    for M in lengths(nev, _partials_len(exec_)):
        for nb, cancel in ((3, False), (1, False), (3, True)):
            d = _data(M, nev, 6, M + nev, cancel)
            B = Blocks(exec_, d, off)
            _lib.call("spmv_hip_lobpcg_gram_f64", ws.ctx, ws.h, M, nb, B.ptr[0],
                      B.ptr[1], B.ptr[2], B.ptr[3], B.ptr[4], B.ptr[5], None)
            _lib.call("spmv_hip_lobpcg_gram_reduce", ws.ctx, ws.h, M, nb, None)
            grid, m = ws.gram_grid(M), nb * nev
            assert grid == lc.gram_grid(M, ws.gram_grid(1 << 40))
            S = np.concatenate(d[:nb], axis=1)
            AS = np.concatenate(d[3:3 + nb], axis=1)
            want = lc.gram_partials(S, AS, grid)
            got = ws.get(GPART, grid * 2 * m * m).reshape(grid, 2, m, m)
            assert same_values(got, want), (M, nb, cancel)
            slot = ws.get(GRAM, 2 * m * m).reshape(2, m, m)
            assert same_values(slot, lc.gram_sum(want)), (M, nb, cancel)
            if cancel and M >= 255 and nev > 1:  # the order is visible
                other = np.triu(S.T @ AS)
                assert not np.array_equal(slot[1], other)
            B.close()
    ws.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", lc.NEV)
def test_gram_wraps_the_grid(exec_, nt, nev, off):  # noqa: F811
    """more chunks than workgroups: workgroup 0 takes a second chunk, the last
    chunk is a partial one"""
    ws = Ws(exec_, nev)
    cap = ws.gram_grid(1 << 40)
    M, m = 64 * cap + 65, 3 * nev
    d = _data(M, nev, 6, 7 + nev)
    B = Blocks(exec_, d, off)
    _lib.call("spmv_hip_lobpcg_gram_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    assert ws.gram_grid(M) == cap
    want = lc.gram_partials(np.concatenate(d[:3], axis=1),
                            np.concatenate(d[3:], axis=1), cap)
    got = ws.get(GPART, cap * 2 * m * m).reshape(cap, 2, m, m)
    assert same_values(got, want)
    B.close()
    ws.close()


# ---- rr -------------------------------------------------------------------------
def _spd_pencil(m, seed):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-1, 1, (m + 3, m))
    Gb = Q.T @ Q
    Ga = rng.uniform(-1, 1, (m, m))
    Ga = Ga + Ga.T
    return np.triu(Gb), np.triu(Ga)


def _run_rr(ws, gram, nb, active, has_p, largest=False, mode=0, advance=1,
            partials=None):
    ws.reset(largest=largest)
    ws.set_state(active, has_p)
    ws.put(COEF, np.full(3 * ws.nev * ws.nev, lc_sentinel()))
    if partials is None:
        ws.put(GRAM, gram)
        _lib.call("spmv_hip_lobpcg_rr", ws.ctx, ws.h, 0, nb, mode, 1, advance,
                  None)
    else:  # M = 65 rows: two workgroups' partials
        ws.put(GPART, partials)
        _lib.call("spmv_hip_lobpcg_rr", ws.ctx, ws.h, 65, nb, mode, 0, advance,
                  None)
    k = ws.nev
    return ws.state(), ws.get(THETA), ws.get(COEF, nb * k * k).reshape(nb * k, k)


def _check_rr(ws, gram, nb, active, has_p, what, largest=False, mode=0,
              partials=None):
    k = ws.nev
    want = lc.rr_ref(gram, k, nb, active, has_p, largest, mode)
    st, theta, coef = _run_rr(ws, gram, nb, active, has_p, largest, mode,
                              partials=partials)
    if not want["ok"]:
        assert (st["done"], st["status"], st["kstop"], st["it"]) == (1, 1, 0, 0), what
        assert np.all(coef == lc_sentinel()), what
        return want, st
    assert (st["done"], st["status"], st["it"]) == (0, 0, 1), (what, st)
    assert st["basis"] == want["basis"] and st["restarts"] == int(want["restart"]), what
    assert st["has_p"] == (1 if nb == 3 and mode == 0 else has_p), what
    assert same_bits(coef, want["coef"]), what
    if mode == 0:
        assert same_bits(theta, want["theta"]), what
    return want, st


@pytest.mark.parametrize("nev", lc.NEV)
def test_rr_on_random_pencils(exec_, nev):  # noqa: F811
    ws = Ws(exec_, nev)
    full = (1 << nev) - 1
    masks = sorted({full, 1, full & ~1} - {0})
    for nb in (1, 3):
        gram = np.stack(_spd_pencil(nb * nev, 10 * nev + nb))
        for active in masks:
            for has_p in (0, 1):
                for largest in (False, True):
                    want, _ = _check_rr(ws, gram, nb, active, has_p,
                                        (nev, nb, active, has_p, largest), largest)
                    assert want["ok"]
        _check_rr(ws, gram, nb, full, 1, (nev, nb, "orth"), mode=1)
    # the partials instead of the reduced slot: the same bits
    gram = np.stack(_spd_pencil(3 * nev, 99))
    parts = np.stack([gram * 0.25, gram * 0.75])
    summed = lc.gram_sum(parts)
    _check_rr(ws, summed, 3, full, 1, (nev, "partials"), partials=parts)
    ws.close()


def test_rr_against_dense_eigh(exec_):  # noqa: F811
    """the Ritz values against numpy's eigh of the whitened pencil: the Jacobi
    stop rule leaves off-diagonals below eps |diagonal|, each of the at most
    30 * m (m - 1) / 2 rotations an error of a few eps ||B||"""
    nev, m = 8, 24
    ws = Ws(exec_, nev)
    gb, ga = _spd_pencil(m, 5)
    st, theta, coef = _run_rr(ws, np.stack([gb, ga]), 3, 255, 1)
    Gb = gb + np.triu(gb, 1).T
    Ga = ga + np.triu(ga, 1).T
    L = np.linalg.cholesky(Gb)
    Bw = np.linalg.solve(L, np.linalg.solve(L, Ga).T).T
    lam = np.linalg.eigvalsh((Bw + Bw.T) / 2)
    eps = np.finfo(np.float64).eps
    bar = 30 * m * m * eps * np.linalg.norm(Bw) * np.linalg.cond(Gb)
    assert np.abs(theta - lam[:nev]).max() <= bar
    assert np.abs(coef.T @ Gb @ coef - np.eye(nev)).max() <= bar
    ws.close()


def test_rr_branches(exec_):  # noqa: F811
    nev, m = 2, 6
    ws = Ws(exec_, nev)
    eye = np.eye(m)
    # identity Gb, a repeated eigenvalue and zero off-diagonals (every rotation
    # of the diagonal Ga is skipped)
    ga = np.diag([3.0, 1.0, 1.0, 2.0, 5.0, 4.0])
    want, _ = _check_rr(ws, np.stack([eye, ga]), 3, 3, 1, "diagonal")
    assert np.array_equal(want["theta"], [1.0, 1.0])
    assert np.array_equal(np.nonzero(want["coef"][:, 0])[0], [1])  # ties by index
    want, _ = _check_rr(ws, np.stack([eye, ga]), 3, 3, 1, "largest", largest=True)
    assert np.array_equal(want["theta"], [5.0, 4.0])
    # one zero off-diagonal among non-zero ones
    ga2 = np.triu(np.random.default_rng(3).uniform(-1, 1, (m, m)))
    ga2[0, 1] = 0.0
    _check_rr(ws, np.stack([eye, ga2]), 3, 3, 1, "zero entry")
    # a pivot of exactly 0 in P: the restart path drops P and succeeds
    gb = eye.copy()
    gb[4, 5] = 1.0          # p_0 == p_1
    want, st = _check_rr(ws, np.stack([gb, ga2]), 3, 3, 1, "restart")
    assert want["ok"] and want["restart"] and st["basis"] == 0b001111
    # ... in W: status 1
    gb = eye.copy()
    gb[2, 3] = 1.0
    want, _ = _check_rr(ws, np.stack([gb, ga2]), 3, 3, 1, "status 1")
    assert not want["ok"]
    # the same column masked out: fine
    want, _ = _check_rr(ws, np.stack([gb, ga2]), 3, 1, 1, "masked")
    assert want["ok"] and want["basis"] == 0b010111
    # a NaN in Gb, in Ga
    for w in (0, 1):
        g = np.stack([eye, ga2])
        g[w, 0, 1] = np.nan
        want, _ = _check_rr(ws, g, 3, 3, 1, ("nan", w))
        assert not want["ok"]
    # a NaN in P alone: the restart path
    g = np.stack([eye, ga2])
    g[1, 4, 5] = np.nan
    want, _ = _check_rr(ws, g, 3, 3, 1, "nan in P")
    assert want["ok"] and want["restart"]
    # after done: nothing is written
    ws.reset()
    ws.set_state(3, 1, done=1)
    ws.put(COEF, np.full(12, lc_sentinel()))
    ws.put(GRAM, np.stack([eye, ga]))
    _lib.call("spmv_hip_lobpcg_rr", ws.ctx, ws.h, 0, 3, 0, 1, 1, None)
    assert np.all(ws.get(COEF) == lc_sentinel()) and ws.state()["it"] == 0
    ws.close()


# ---- update, residual, norms -------------------------------------------------------
def _check_update(ws, exec_, nev, M, off, active, has_p):  # noqa: F811
    gram = np.stack(_spd_pencil(3 * nev, M % 97 + active))
    want = lc.rr_ref(gram, nev, 3, active, has_p)
    _run_rr(ws, gram, 3, active, has_p)
    d = _data(M, nev, 6, M)
    B = Blocks(exec_, d, off)
    _lib.call("spmv_hip_lobpcg_update_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    X, P = lc.combine(d[:3], want["coef"], want["basis"], active, nev)
    AX, AP = lc.combine(d[3:], want["coef"], want["basis"], active, nev)
    what = (M, active, has_p)
    for i, ref in ((0, X), (2, P), (3, AX), (5, AP), (1, d[1]), (4, d[4])):
        assert same_values(B.get(i, (M, nev)), ref), (what, i)
    for c in range(nev):  # an inactive column's P is left alone
        if not (active >> c) & 1:
            assert same_bits(B.get(2, (M, nev))[:, c], d[2][:, c])
    B.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", lc.NEV)
def test_update(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    full = (1 << nev) - 1
    for M in lengths(nev, _partials_len(exec_)):
        masks = sorted({full, 1, full & ~1} - {0}) if M == 1331 else [full]
        for active in masks:
            for has_p in ((1, 0) if M in (65, 1331) else (1,)):
                _check_update(ws, exec_, nev, M, off, active, has_p)
    # one block: the prologue's X R^-1, AX untouched when absent
    M = 257
    gram = np.stack(_spd_pencil(nev, 4))
    want = lc.rr_ref(gram, nev, 1, full, 0, mode=1)
    _run_rr(ws, gram, 1, full, 0, mode=1, advance=0)
    d = _data(M, nev, 1, 11)
    B = Blocks(exec_, d, off)
    _lib.call("spmv_hip_lobpcg_update_f64", ws.ctx, ws.h, M, 1, B.ptr[0], None,
              None, None, None, None, None)
    X, _ = lc.combine(d, want["coef"], want["basis"], full, nev)
    assert same_values(B.get(0, (M, nev)), X)
    # after done the kernel returns at once
    ws.set_state(full, 0, done=1)
    _lib.call("spmv_hip_lobpcg_update_f64", ws.ctx, ws.h, M, 1, B.ptr[0], None,
              None, None, None, None, None)
    assert same_values(B.get(0, (M, nev)), X)
    B.close()
    ws.close()


@pytest.mark.parametrize("slot", range(4))
@pytest.mark.parametrize("nev", lc.NEV)
def test_update_wraps_the_grid(exec_, nt, nev, slot):  # noqa: F811
    """a thread takes a second row: every width, the run-time one included"""
    ws = Ws(exec_, nev)
    full = (1 << nev) - 1
    L = _partials_len(exec_)
    for M in wrap_lengths(nev, L, slot):
        assert M > 256 * L - 2
        _check_update(ws, exec_, nev, M, 0, full if slot else full & ~1 or full, 1)
    ws.close()


def _check_residual(ws, exec_, nev, M, off, with_dinv, L):  # noqa: F811
    full = (1 << nev) - 1
    rng = np.random.default_rng(M)
    theta = rng.uniform(0.5, 2.0, nev)
    X, AX = _data(M, nev, 2, M + 1)
    AX[:, 0] = X[:, 0] * theta[0] * (1.0 + 2.0 ** -40)  # column 0 meets its test
    dinv = rng.uniform(0.5, 2.0, M + 1)
    ws.reset(rtol=2.0 ** -20, atol=0.0)
    ws.set_state(full, 0, it=2)
    ws.put(THETA, theta)
    B = Blocks(exec_, [X, AX, np.zeros((M, nev)), np.zeros((M, nev))], off)
    d_dinv = exec_.alloc(M + 1)
    exec_.copy_from_host(d_dinv, dinv)
    _lib.call("spmv_hip_lobpcg_residual_f64", ws.ctx, ws.h, M, B.ptr[0],
              B.ptr[1], d_dinv if with_dinv else None, B.ptr[2], B.ptr[3],
              0, None)
    R, W, r2 = lc.residual_ref(X, AX, theta, dinv[:M] if with_dinv else None)
    assert same_values(B.get(2, (M, nev)), R), (M, with_dinv)
    assert same_values(B.get(3, (M, nev)), W), (M, with_dinv)
    grid = lc.rows_grid(M, L)
    parts = lc.rows_partials(r2, grid)
    got = ws.get(RPART).reshape(L, nev)
    assert same_values(got[:grid], parts) and np.all(got[grid:] == 0.0), M
    _lib.call("spmv_hip_lobpcg_norms", ws.ctx, ws.h, 0, 0, None)
    rn2 = lc.reduce_column(parts)
    assert same_values(ws.get(RN, nev), rn2), M
    hist = np.full((nev, KMAX + 1), -1.0)
    active, done = lc.norms_ref(rn2, theta, full, 2, KMAX, 2.0 ** -20, 0.0, hist)
    st = ws.state()
    assert st["active"] == active, (M, st)
    if M >= 63:  # column 0 alone has met its test
        assert active == full & ~1, (M, active)
    assert st["done"] == int(done) and st["it"] == 2
    got_hist = ws.get(HIST).reshape(KMAX + 1, nev)
    assert same_values(got_hist[2], hist[:, 2]), M
    assert np.all(got_hist[[0, 1, 3, 4]] == -1.0)
    exec_.free(d_dinv)
    B.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", lc.NEV)
def test_residual_and_norms(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    L = _partials_len(exec_)
    for M in lengths(nev, L):
        for with_dinv in (False, True):
            _check_residual(ws, exec_, nev, M, off, with_dinv, L)
    ws.close()


@pytest.mark.parametrize("slot", range(4))
@pytest.mark.parametrize("nev", lc.NEV)
def test_residual_wraps_the_grid(exec_, nt, nev, slot):  # noqa: F811
    ws = Ws(exec_, nev)
    L = _partials_len(exec_)
    for M in wrap_lengths(nev, L, slot):
        _check_residual(ws, exec_, nev, M, 0, bool(slot % 2), L)
    ws.close()


def test_norms_phases_and_final(exec_):  # noqa: F811
    """several ranks: phase 1 leaves the sums for the all-reduce, phase 2
    decides from the slot; final: the second half of the slot, `done`
    ignored, nothing else written; kmax ends the solve"""
    nev, M = 3, 300
    ws = Ws(exec_, nev)
    X, AX = _data(M, nev, 2, 1)
    theta = np.array([1.0, -2.0, 0.5])
    B = Blocks(exec_, [X, AX, np.zeros((M, nev))], 0)
    ws.reset(rtol=1e-9, atol=0.0)
    ws.set_state(7, 0, it=KMAX)
    ws.put(THETA, theta)
    _lib.call("spmv_hip_lobpcg_residual_f64", ws.ctx, ws.h, M, B.ptr[0], B.ptr[1],
              None, B.ptr[2], None, 0, None)
    _lib.call("spmv_hip_lobpcg_norms", ws.ctx, ws.h, 1, 0, None)
    _, _, r2 = lc.residual_ref(X, AX, theta)
    rn2 = lc.reduce_column(lc.rows_partials(r2, 2))
    assert same_values(ws.get(RN, nev), rn2)
    assert np.all(ws.get(HIST) == -1.0) and ws.state()["done"] == 0
    ws.put(RN, np.concatenate([2.0 * rn2, np.zeros(nev)]))  # "all-reduced"
    _lib.call("spmv_hip_lobpcg_norms", ws.ctx, ws.h, 2, 0, None)
    st = ws.state()
    assert (st["done"], st["kstop"], st["status"], st["active"]) == (1, KMAX, 0, 7)
    assert same_values(ws.get(HIST).reshape(KMAX + 1, nev)[KMAX], np.sqrt(2.0 * rn2))
    # after done: residual returns at once, the final pair still runs
    exec_.copy_from_host(B.ptr[2], np.full(M * nev, lc_sentinel()))
    _lib.call("spmv_hip_lobpcg_residual_f64", ws.ctx, ws.h, M, B.ptr[0], B.ptr[1],
              None, B.ptr[2], None, 0, None)
    assert np.all(B.get(2, (M, nev)) == lc_sentinel())
    _lib.call("spmv_hip_lobpcg_residual_f64", ws.ctx, ws.h, M, B.ptr[0], B.ptr[1],
              None, B.ptr[2], None, 1, None)
    _lib.call("spmv_hip_lobpcg_norms", ws.ctx, ws.h, 0, 1, None)
    rn = ws.get(RN)
    assert same_values(rn[nev:], rn2) and same_values(rn[:nev], 2.0 * rn2)
    B.close()
    ws.close()
