"""CgOptions::defer_x (one rank, consumer-side reductions): the x update of
iteration k waits for iteration k+1, p alternates between two buffers, and a
loop that ends on the first half of a pair is closed by a flush kernel.  Every
element still sees the parent sequence's operations in their order, so the
bar is bit equality with `defer_x=False` -- the sequence the other CG tests
hold to the oracle -- on x, on the residual history and on the returned k.

Each case runs the same solve twice on the same executor and workspace,
`defer_x=False` then `True`; x is overwritten with a sentinel before every
solve so that a kernel that did nothing cannot pass."""
import numpy as np
import pytest

import oracle
from spmv_amd import _lib, host, poisson

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24  # common.h: blas1_nt_min_elems


@pytest.fixture(scope="module")
def exec_():
    e = host.HipExecutor(0)
    yield e
    e.synchronize()
    e.close()


@pytest.fixture(scope="module")
def comm():
    c = host.Comm.self_comm()
    yield c
    c.close()


def _banded_spd(n):
    """Symmetric, strictly diagonally dominant band (offsets 1, 37, 600) with
    irrational values: n = 4097 is odd and two units of the streaming loop
    plus one element."""
    i = np.arange(n)
    rows, cols, vals = [i], [i], [6.0 + 0.3 * np.sin(i)]
    for d in (1, 37, 600):
        a, b = i[:-d], i[:-d] + d
        v = -(0.5 + 0.4 * np.cos((a + b).astype(np.float64)))
        rows += [a, b]
        cols += [b, a]
        vals += [v, v]
    rows, cols, vals = map(np.concatenate, (rows, cols, vals))
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return rp.astype(np.int64), cols[order].astype(np.int64), vals[order]


class _Problem:
    def __init__(self, exec_, comm, name):
        if name.startswith("poisson"):
            n = int(name[7:])
            rp, ci, va = poisson.poisson3d_csr(n)
            self.N = n ** 3
        else:
            self.N = int(name[6:])
            rp, ci, va = _banded_spd(self.N)
        self.csr = (np.asarray(rp).astype(np.int32),
                    np.asarray(ci).astype(np.int32), np.asarray(va))
        rng = np.random.default_rng(self.N)
        self.b = oracle.csr_spmv(*self.csr, rng.uniform(-1, 1, self.N))
        self.b2 = oracle.csr_spmv(*self.csr, np.ones(self.N))
        self.exec_ = exec_
        self.A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, self.N,
                                           self.N, [], [], False,
                                           host.P2P_NONBLOCKING)
        self.d_b, self.d_b2 = exec_.alloc(self.N), exec_.alloc(self.N)
        self.d_x = exec_.alloc(self.N + 2)
        exec_.copy_from_host(self.d_b, self.b)
        exec_.copy_from_host(self.d_b2, self.b2)
        self.ws = host.CgWorkspace(exec_)

    def close(self):
        self.ws.close()
        self.A.close()
        for d in (self.d_b, self.d_b2, self.d_x):
            self.exec_.free(d)


# 13 824 rows (6 units and a ragged 7th), 1 331 rows (odd, less than one unit
# of 2 048 doubles), 4 097 rows (odd, two units and the tail element alone)
SHAPES = ("poisson24", "poisson11", "banded4097")


@pytest.fixture(scope="module")
def problems(exec_, comm):
    ps = {name: _Problem(exec_, comm, name) for name in SHAPES}
    yield ps
    for p in ps.values():
        p.close()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, exec_):
    """Both instantiations of every BLAS-1 kernel."""
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


def _solve(comm, P, kmax, rtol, defer, ws=None, d_b=None, x_off=0, **kw):
    """-> (k, history, x); x_off in doubles from the 256-byte aligned buffer"""
    e = P.exec_
    e.copy_from_host(P.d_x, np.full(P.N + 2, 777.0))
    d_x = P.d_x + 8 * x_off
    k, hist, _, _ = host.cg_ex(comm, e, P.A, d_b or P.d_b, d_x, kmax, rtol,
                               ws or P.ws, history=True, defer_x=defer, **kw)
    return k, hist.copy(), e.copy_to_host(d_x, P.N)


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what
    assert np.all(np.isfinite(a[2])) and not np.any(a[2] == 777.0), what


def _pair(comm, P, kmax, rtol, what, **kw):
    ref = _solve(comm, P, kmax, rtol, False, **kw)
    new = _solve(comm, P, kmax, rtol, True, **kw)
    _same(ref, new, what)
    return ref


@pytest.mark.parametrize("shape", SHAPES)
def test_loop_ends_on_either_parity(comm, problems, nt, shape):
    """rtol = 0: no iteration, a P step alone + flush, a whole pair, a pair +
    P step + flush, three pairs, three pairs + P step + flush."""
    P = problems[shape]
    for kmax in (0, 1, 2, 3, 6, 7):
        k, hist, x = _pair(comm, P, kmax, 0.0, (shape, kmax))
        assert k == kmax and len(hist) == kmax + 1
        assert np.any(x != 0.0) == (kmax > 0)


def _rtol_stopping_at(hist, parity, lo=5):
    """An rtol that iteration k is the first to meet, for the first k >= lo of
    the given parity at which the history reaches a new minimum."""
    rel = hist / hist[0]
    for k in range(lo, len(hist)):
        before = rel[1:k].min()
        if k % 2 == parity and rel[k] < before:
            rtol = float(np.sqrt(rel[k] * before))
            if rel[k] < rtol <= before:
                return k, rtol
    raise AssertionError("no new minimum of that parity in the history")


@pytest.mark.parametrize("shape", SHAPES)
def test_stops_by_tolerance_on_either_parity(comm, problems, nt, shape):
    """The tolerance is met at an odd k (a P step: its converged branch
    updates x) and at an even k (an X2P step: both updates), with kmax far
    beyond, so every launch after `done` and the flush do nothing; then with
    kmax == k odd, where `done` is never raised and only the flush's own test
    keeps it from applying the update a second time."""
    P = problems[shape]
    _, hist, _ = _solve(comm, P, 40, 0.0, False)
    for parity in (1, 0):
        kstop, rtol = _rtol_stopping_at(hist, parity)
        for kmax in (kstop + 40, kstop + 41):  # queue ends on either parity
            k, h, _ = _pair(comm, P, kmax, rtol, (shape, parity, kmax),
                            poll_every=255)  # host enqueues all of them
            assert k == kstop and np.array_equal(h, hist[:kstop + 1])
        k, _, _ = _pair(comm, P, kstop + 40, rtol, (shape, parity, "poll"),
                        poll_every=1)  # host stops enqueuing early
        assert k == kstop
        if parity == 1:
            k, _, _ = _pair(comm, P, kstop, rtol, (shape, "k == kmax, odd"))
            assert k == kstop


def test_workspace_reused_after_either_parity(comm, problems, nt):
    """A solve that ended on the second p buffer leaves nothing behind: the
    next solve on the same workspace (another b, even kmax) equals one on a
    fresh workspace, and so in the other order."""
    P = problems["poisson11"]
    for first, second in ((7, 6), (6, 7), (1, 2)):
        fresh = host.CgWorkspace(P.exec_)
        want = _solve(comm, P, second, 0.0, True, ws=fresh, d_b=P.d_b2)
        fresh.close()
        _solve(comm, P, first, 0.0, True)
        got = _solve(comm, P, second, 0.0, True, d_b=P.d_b2)
        _same(want, got, (first, second))
        _same(want, _solve(comm, P, second, 0.0, False, d_b=P.d_b2),
              (first, second, "defer_x=False"))


def test_workspace_grows_between_solves(comm, problems):
    """The second p buffer follows the workspace when a larger problem
    arrives on it."""
    ws = host.CgWorkspace(problems["poisson11"].exec_)
    for shape in ("poisson11", "poisson24", "banded4097"):
        P = problems[shape]
        _same(_solve(comm, P, 7, 0.0, False), _solve(comm, P, 7, 0.0, True, ws=ws),
              shape)
    ws.close()


def test_workspace_kept_by_a_smaller_solve_and_p2_brought_back(comm, problems,
                                                               exec_):
    """One workspace through n = 11, n = 8 (smaller: nothing regrows), n = 11
    without defer_x, n = 11 with it (the second p buffer after a solve that
    did not use it).  kmax = 7: the loop ends on a P step and the flush runs.
    Every solve equals the same solve on a fresh workspace, x and history."""
    big, small = problems["poisson11"], _Problem(exec_, comm, "poisson8")
    ws = host.CgWorkspace(exec_)
    try:
        for P, defer in ((big, True), (small, True), (big, False), (big, True)):
            fresh = host.CgWorkspace(exec_)
            want = _solve(comm, P, 7, 0.0, defer, ws=fresh)
            fresh.close()
            got = _solve(comm, P, 7, 0.0, defer, ws=ws)
            _same(want, got, (P.N, defer))
            assert got[0] == 7 and len(got[1]) == 8
    finally:
        ws.close()
        small.close()


@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_fallbacks_keep_the_bits(comm, problems, shape):
    """Where the deferred sequence does not apply the parent's runs, with the
    parent's bits: an x that is not 16-byte aligned, reducer kernels instead
    of consumer-side reductions, a mixed-precision solve."""
    P = problems[shape]
    for kmax in (6, 7):
        ref = _solve(comm, P, kmax, 0.0, False)
        for defer in (False, True):
            _same(ref, _solve(comm, P, kmax, 0.0, defer, x_off=1),
                  (shape, kmax, defer, "x + 8 bytes"))
            _same(ref, _solve(comm, P, kmax, 0.0, defer,
                              consumer_reductions=False),
                  (shape, kmax, defer, "reducer kernels"))
        out = []
        for defer in (False, True):
            P.exec_.copy_from_host(P.d_x, np.full(P.N + 2, 777.0))
            k, h, _ = host.cg_mixed(comm, P.exec_, P.A, P.d_b, P.d_x, kmax, 0.0,
                                    replace_every=4, workspace=P.ws,
                                    defer_x=defer)
            out.append((k, h.copy(), P.exec_.copy_to_host(P.d_x, P.N)))
        _same(out[0], out[1], (shape, kmax, "mixed"))


def test_against_the_oracle(comm, problems, nt):
    """The deferred sequence against the CPU oracle's CG, with the bars of the
    other CG tests (test_gpu_matrix._cg_vs_oracle: |dk| <= 1, residual history
    to 1e-6 over the first 50 iterations, ||dx|| <= 1e-8 ||x||)."""
    P = problems["poisson24"]
    kmax, rtol = 100, 1e-10
    x_ref, k_ref, hist_ref = oracle.cg(*P.csr, P.b2, kmax, rtol)
    k, hist, x = _solve(comm, P, kmax, rtol, True, d_b=P.d_b2)
    assert (k == k_ref == kmax) or abs(k - k_ref) <= 1, (k, k_ref)
    if k < kmax:
        assert hist[-1] / hist[0] < rtol
    m = min(k, k_ref, 50)
    dev = np.abs(hist[:m + 1] / hist_ref[:m + 1] - 1)
    assert np.all(dev <= 1e-6), dev.max()
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    assert err <= 1e-8, err
