"""spmv::pcg (CG with a diagonal preconditioner), Matrix::diagonal and
jacobi_inverse.

Shapes are those of test_gpu_cg_block.py, for the reasons given at its top:
1 331 rows (odd; less than one streaming unit of 2 048 doubles), 13 824 rows,
4 097 rows (odd); both instantiations (cached / non-temporal) of every kernel
run through `blas1_nt_min_elems`.

The matrix under test is S A S with S = diag(s), s = 10 ** uniform(-1, 1): the
class of matrices a diagonal preconditioner is for.  Entry (i, j) is
a_ij * (s_i * s_j) -- the product in the parentheses commutes bit for bit, so
the scaled matrix is exactly symmetric and symmetric storage holds the same
matrix as general storage.

The reference is the numpy Jacobi-PCG below, the algorithm of cg.h restated on
oracle.csr_spmv / oracle.ddot (oracle.dist_spmv and a rank-ordered sum for
several ranks).  Bars are the project's own (test_gpu_cg_block._vs_oracle):
|k - k_ref| <= 1, residual history to 1e-6 relative over min(k, k_ref, 50)
entries (the last one only above the noise floor 8 u ||A||_inf ||x_ref||_2),
||x - x_ref|| <= 1e-8 ||x_ref||.

X sits between guard words and is filled with a sentinel before every solve,
so a kernel that did nothing, or wrote past its range, cannot pass."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from spmv_amd import _lib, host, poisson

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24  # common.h: blas1_nt_min_elems
SENTINEL = 777.0
U = 2.0 ** -53
KMAX, RTOL = 200, 1e-10
GUARD = 2  # doubles in front of an aligned X (16 bytes)
CMS = [host.P2P_BLOCKING, host.P2P_NONBLOCKING, host.COLLECTIVE_BLOCKING,
       host.COLLECTIVE_NONBLOCKING]


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
    irrational values (the generator of test_gpu_cg_block.py)."""
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


def _csr(name):
    if name.startswith("poisson"):
        rp, ci, va = poisson.poisson3d_csr(int(name[7:]))
    else:
        rp, ci, va = _banded_spd(int(name[6:]))
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, dtype=np.float64))


def _row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _scaled(csr):
    """S A S (see the top of the file)"""
    rp, ci, va = csr
    N = len(rp) - 1
    s = 10.0 ** np.random.default_rng(N).uniform(-1, 1, N)
    return rp, ci, va * (s[_row_of(rp)] * s[ci])


def _diag_of(csr):
    """the diagonal of a CSR with at most one entry (i, i) per row; 0 where a
    row has none"""
    rp, ci, va = csr
    rows = _row_of(rp)
    d = np.zeros(len(rp) - 1)
    on = ci == rows
    d[rows[on]] = va[on]
    return d


def _norm_inf(csr):
    return float(np.add.reduceat(np.abs(csr[2]), csr[0][:-1]).max())


# ---- the reference: Jacobi-PCG of cg.h in numpy ------------------------------
def _pcg_ref(spmv, dot, b, dinv, kmax, rtol):
    """-> (x, k, history of ||r_j||); spmv(p) = A p, dot = the global dot"""
    x = np.zeros(len(b))
    r = np.array(b, dtype=np.float64)
    z = dinv * r
    p = z.copy()
    rz, rr0 = dot(r, z), dot(r, r)
    hist = [math.sqrt(rr0)]
    k = 0
    if rr0 == 0.0:
        return x, 0, np.array(hist)
    while k < kmax:
        k += 1
        Ap = spmv(p)
        alpha = rz / dot(p, Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = dinv * r
        rz_new, rr = dot(r, z), dot(r, r)
        hist.append(math.sqrt(rr))
        if math.sqrt(rr) / math.sqrt(rr0) < rtol:
            break
        beta = rz_new / rz
        rz = rz_new
        p = beta * p + z
    return x, k, np.array(hist)


def _noise_floor(norm_a, x_ref):
    return 8 * U * norm_a * np.linalg.norm(x_ref)


def _vs_oracle(k, hist, x, ref, kmax, rtol, norm_a, what):
    x_ref, k_ref, hist_ref = ref
    print(what, "k", k, "k_ref", k_ref)
    assert abs(k - k_ref) <= 1, (what, k, k_ref)
    assert len(hist) == k + 1, what
    if 0 < k < kmax:
        assert hist[k] / hist[0] < rtol, what
    m = min(k, k_ref, 50)
    upto = m + 1 if hist_ref[m] >= _noise_floor(norm_a, x_ref) else m
    dev = np.abs(hist[:upto] / hist_ref[:upto] - 1)
    print(what, "history deviation", dev.max())
    assert np.all(dev <= 1e-6), (what, dev.max())
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print(what, "x error", err)
    assert err <= 1e-8, (what, err)


class _Problem:
    """One shape: the scaled matrix in both storages, its Jacobi dinv on the
    device (through Matrix::diagonal and jacobi_inverse), right-hand sides and
    references (computed once)."""

    def __init__(self, exec_, comm, name):
        self.name, self.exec_ = name, exec_
        self.plain = _csr(name)
        self.csr = _scaled(self.plain)
        self.N = N = len(self.csr[0]) - 1
        self.diag = _diag_of(self.csr)
        self.norm_a = _norm_inf(self.csr)
        rng = np.random.default_rng(N + 1)
        self.rhs = {"ones": oracle.csr_spmv(*self.csr, np.ones(N)),
                    "rand": oracle.csr_spmv(*self.csr, rng.uniform(-1, 1, N)),
                    "zero": np.zeros(N)}
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.d_dinv = {}
        for sym, A in self.A.items():
            self.d_dinv[sym] = exec_.alloc(N + 1)
            A.diagonal(self.d_dinv[sym])
            host.jacobi_inverse(exec_, self.d_dinv[sym], self.d_dinv[sym], N)
        self.d_b = exec_.alloc(N)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.PcgWorkspace(exec_)
        self._ref = {}

    def ref(self, rhs, kmax=KMAX, rtol=RTOL):
        key = (rhs, kmax, rtol)
        if key not in self._ref:
            self._ref[key] = _pcg_ref(lambda p: oracle.csr_spmv(*self.csr, p),
                                      oracle.ddot, self.rhs[rhs],
                                      1.0 / self.diag, kmax, rtol)
        return self._ref[key]

    def solve(self, comm, rhs, kmax=KMAX, rtol=RTOL, symmetric=False, ws=None,
              x_off=GUARD, A=None, d_dinv=None, b=None, **kw):
        """-> (k, history, x); x_off in doubles from the 256-byte aligned
        buffer (GUARD: aligned, GUARD + 1: 8 bytes off)"""
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_b, self.rhs[rhs] if b is None else b)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        d_x = self.d_x + 8 * x_off
        k, hist = host.pcg(comm, e, A or self.A[symmetric], self.d_b, d_x,
                           d_dinv or self.d_dinv[symmetric], kmax, rtol,
                           ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[x_off + N:] == SENTINEL), (self.name, "guard behind")
        assert np.all(np.isfinite(x)) and not np.any(x == SENTINEL), self.name
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in list(self.d_dinv.values()) + [self.d_b, self.d_x]:
            self.exec_.free(p)


SHAPES = ("poisson11", "poisson24", "banded4097")


@pytest.fixture(scope="module")
def problems(exec_, comm):
    ps = {name: _Problem(exec_, comm, name) for name in SHAPES}
    yield ps
    for p in ps.values():
        p.close()


@pytest.fixture(params=[NT_DEFAULT, 1], ids=["cached", "nontemporal"])
def nt(request, exec_):
    """Both instantiations of every kernel."""
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              request.param)
    yield request.param
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
              NT_DEFAULT)


# ---- 1. the diagonal and its inverse, exact ----------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_diagonal_and_inverse_are_exact(exec_, problems, shape):
    P = problems[shape]
    d_d, d_i = exec_.alloc(P.N), exec_.alloc(P.N)
    for sym, A in P.A.items():
        exec_.copy_from_host(d_d, np.full(P.N, SENTINEL))
        A.diagonal(d_d)
        d = exec_.copy_to_host(d_d, P.N)
        assert np.array_equal(d, P.diag), (shape, sym)
        host.jacobi_inverse(exec_, d_d, d_i, P.N)
        assert np.array_equal(exec_.copy_to_host(d_i, P.N), 1.0 / P.diag)
        # ... what every solve below uses
        assert np.array_equal(exec_.copy_to_host(P.d_dinv[sym], P.N),
                              1.0 / P.diag), (shape, sym)
    exec_.free(d_d), exec_.free(d_i)


def test_rows_without_a_diagonal_and_bad_entries(exec_, comm, problems):
    """General storage: a row without an entry (i, i) has diagonal 0.0, and
    jacobi_inverse refuses that diagonal; likewise a negative entry and a NaN."""
    rp, ci, va = problems["poisson11"].csr
    N = len(rp) - 1
    rows = _row_of(rp)
    gone = np.array([0, 5, 700, N - 1])
    keep = ~((ci == rows) & np.isin(rows, gone))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=N))])
    holes = (rp2.astype(np.int32), ci[keep], va[keep])
    neg = va.copy()
    neg[np.flatnonzero(ci == rows)[17]] *= -1.0
    nan = va.copy()
    nan[np.flatnonzero(ci == rows)[N - 2]] = np.nan
    d_d, d_i = exec_.alloc(N), exec_.alloc(N)
    for what, csr in (("holes", holes), ("negative", (rp, ci, neg)),
                      ("nan", (rp, ci, nan))):
        A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], False,
                                      host.P2P_NONBLOCKING)
        exec_.copy_from_host(d_d, np.full(N, SENTINEL))
        A.diagonal(d_d)
        d = exec_.copy_to_host(d_d, N)
        assert np.array_equal(d, _diag_of(csr), equal_nan=True), what
        if what == "holes":
            assert np.all(d[gone] == 0.0) and np.count_nonzero(d == 0.0) == 4
        with pytest.raises(host.SpmvHostError, match="positive"):
            host.jacobi_inverse(exec_, d_d, d_i, N)
        A.close()
    exec_.free(d_d), exec_.free(d_i)


def _slab_inputs(n):
    csr = _scaled(_csr(f"poisson{n}"))
    return csr, _diag_of(csr)


@pytest.mark.parametrize("world", [2, 3])
def test_diagonal_on_slab_ranks(world):
    """Ranks as threads, the scaled Poisson matrix in slabs, both storages,
    every halo model: each rank gets the diagonal of its own rows."""
    from thread_world import ThreadWorld
    (rp, ci, va), diag = _slab_inputs(8)
    N = len(rp) - 1
    ranges = oracle.owner_ranges(world, N)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        d_d = exec_.alloc(M)
        for sym in (False, True):
            for cm in CMS:
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                exec_.copy_from_host(d_d, np.full(M, SENTINEL))
                A.diagonal(d_d)
                assert np.array_equal(exec_.copy_to_host(d_d, M), diag[r0:r1]), \
                    (world, rank, sym, cm)
                A.close()
        exec_.free(d_d)

    tw.run(rank_body, gpu=True)


# ---- 2. against the reference -------------------------------------------------
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_reference(comm, problems, nt, shape, symmetric, rhs):
    P = problems[shape]
    ref = P.ref(rhs)
    k, hist, x = P.solve(comm, rhs, symmetric=symmetric)
    assert k < KMAX
    _vs_oracle(k, hist, x, ref, KMAX, RTOL, P.norm_a, (shape, symmetric, rhs))
    # what the preconditioner is for: plain CG on the same system is not done
    # after twice as many iterations (a relation between two references)
    _, k_ref_cg, _ = oracle.cg(*P.csr, P.rhs[rhs], 400, RTOL)
    print(shape, rhs, "k_ref_pcg", ref[1], "k_ref_cg", k_ref_cg)
    assert ref[1] < k_ref_cg


# ---- 3. the paths agree bit for bit on one rank -------------------------------
def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reducer_and_consumer_paths_and_unaligned_x(comm, problems, nt, shape,
                                                    symmetric):
    P = problems[shape]
    for kmax in (KMAX, 9):
        want = P.solve(comm, "rand", kmax=kmax, symmetric=symmetric)
        assert want[0] > 1
        got = P.solve(comm, "rand", kmax=kmax, symmetric=symmetric,
                      consumer_reductions=False)
        _same(want, got, (shape, symmetric, kmax, "reducer kernels"))
        got = P.solve(comm, "rand", kmax=kmax, symmetric=symmetric,
                      x_off=GUARD + 1)  # X + 8 bytes
        _same(want, got, (shape, symmetric, kmax, "unaligned x"))


def test_unaligned_dinv_keeps_the_bits(exec_, comm, problems, nt):
    P = problems["banded4097"]
    want = P.solve(comm, "rand", kmax=25)
    d = exec_.alloc(P.N + 1)
    exec_.copy(d + 8, P.d_dinv[False], P.N * 8)
    got = P.solve(comm, "rand", kmax=25, d_dinv=d + 8)
    _same(want, got, "unaligned dinv")
    exec_.free(d)


def test_workspace_reused_and_grown(comm, problems, nt):
    """One workspace across shapes (small, large, middle) and across a smaller
    kmax: every result equals the one on a fresh workspace, bit for bit."""
    e = problems["poisson11"].exec_
    shared = host.PcgWorkspace(e)
    plan = [("poisson11", 30, GUARD), ("poisson24", 40, GUARD + 1),
            ("banded4097", 12, GUARD), ("poisson24", 7, GUARD),
            ("poisson11", 40, GUARD + 1), ("poisson11", 0, GUARD)]
    for shape, kmax, x_off in plan:
        P = problems[shape]
        fresh = host.PcgWorkspace(e)
        want = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=fresh, x_off=x_off)
        fresh.close()
        got = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=shared, x_off=x_off)
        _same(want, got, (shape, kmax, x_off))
    shared.close()


# ---- 4. dinv = 1: the preconditioner degenerates to CG ------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_unit_dinv_is_cg(exec_, comm, problems, nt, shape):
    P = problems[shape]
    rp, ci, va = P.plain
    N = P.N
    d_one = exec_.alloc(N)
    exec_.copy_from_host(d_one, np.ones(N))
    b = oracle.csr_spmv(rp, ci, va, np.ones(N))
    ref = oracle.cg(rp, ci, va, b, KMAX, RTOL)
    assert ref[1] < KMAX
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        k, hist, x = P.solve(comm, None, A=A, d_dinv=d_one, b=b)
        _vs_oracle(k, hist, x, ref, KMAX, RTOL, _norm_inf(P.plain),
                   (shape, sym, "dinv = 1"))
        A.close()
    exec_.free(d_one)


# ---- 5. rtol = 0 ----------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape, symmetric):
    P = problems[shape]
    for kmax in (0, 1, 2, 7):
        for kw in ({}, {"consumer_reductions": False}):
            k, hist, x = P.solve(comm, "ones", kmax=kmax, rtol=0.0,
                                 symmetric=symmetric, **kw)
            what = (shape, symmetric, kmax, kw)
            assert k == kmax, what
            assert hist.shape == (kmax + 1,) and np.all(hist > 0.0), what
            assert np.any(x != 0.0) == (kmax > 0), what
            # b = 0: stopped at k = 0 with x = 0, nothing undefined
            k, hist, x = P.solve(comm, "zero", kmax=kmax, rtol=0.0,
                                 symmetric=symmetric, **kw)
            assert k == 0 and np.all(x == 0.0), what
            assert hist.shape == (1,) and hist[0] == 0.0, what


# ---- 6. frozen after convergence -------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_after_convergence(comm, problems, nt, shape):
    """poll_every = 255 and kmax far beyond the stop: every iteration is
    enqueued, so every kernel launched after `done` had the chance to touch x;
    poll_every = 1: the host stops enqueuing early."""
    P = problems[shape]
    for kw in ({}, {"consumer_reductions": False}):
        k, hist, x = P.solve(comm, "rand", **kw)
        assert 1 < k and k + 80 < 255
        for poll in (255, 1):
            got = P.solve(comm, "rand", kmax=k + 80, poll_every=poll, **kw)
            _same((k, hist, x), got, (shape, kw, poll))
        got = P.solve(comm, "rand", kmax=k, **kw)
        _same((k, hist, x), got, (shape, kw, "kmax = k"))


# ---- 7. errors ---------------------------------------------------------------------
def _current_stream(exec_):
    s = C.c_void_p()
    _lib.call("spmv_hip_get_stream", exec_.context, C.byref(s))
    return s.value


def test_errors_leave_the_executor_as_it_was(comm, problems):
    P = problems["poisson11"]
    e, A, N = P.exec_, P.A[False], P.N
    dinv = P.d_dinv[False]
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)
    try:
        e.copy_from_host(P.d_b, P.rhs["ones"])
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg(comm, e, A, P.d_b, P.d_b, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg(comm, e, A, P.d_b, P.d_b + 8 * (N - 1), dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg(comm, e, A, P.d_b, dinv, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg(comm, e, A, P.d_b, dinv + 8, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.pcg(comm, e, A, P.d_b, P.d_x, dinv, -1, 1e-10)
        assert _current_stream(e) == mine.value
        # dinv is as it was
        assert np.array_equal(e.copy_to_host(dinv, N), 1.0 / P.diag)
        # ... and after a solve that went through
        k, _ = host.pcg(comm, e, A, P.d_b, P.d_x, dinv, 3, 0.0, P.ws)
        assert k == 3
        assert _current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


def test_abi_refuses_short_destinations_and_bad_iterations(exec_):
    """spmv_hip_pcg_ws_read_async copies nothing into a buffer that is too
    short; slots and kernels refuse an iteration outside their range."""
    h, ctx = _lib.hip, exec_.context
    ws = C.c_void_p()
    _lib.call("spmv_hip_pcg_ws_create", ctx, 5, C.byref(ws))
    try:
        kmax = C.c_int()
        _lib.call("spmv_hip_pcg_ws_capacity", ws, C.byref(kmax))
        assert kmax.value == 5
        flags = np.full(2, 99, np.int32)
        zr = np.full(12, -7.0)
        fp, zp = flags.ctypes.data_as(C.c_void_p), zr.ctypes.data_as(C.c_void_p)
        assert h.spmv_hip_pcg_ws_read_async(ws, fp, zp, 11, None) == -1
        assert h.spmv_hip_pcg_ws_read_async(ws, None, zp, 6, None) == -1
        assert h.spmv_hip_pcg_ws_read_async(ws, fp, zp, 0, None) == -1
        exec_.synchronize()
        assert np.all(flags == 99) and np.all(zr == -7.0)
        _lib.call("spmv_hip_pcg_ws_reset", ws, 1e-8, None)
        _lib.call("spmv_hip_pcg_ws_read_async", ws, fp, zp, 12, None)
        exec_.synchronize()
        assert flags[0] == 0 and flags[1] == -1 and np.all(zr == 0.0)
        # the pair {rz[k], rr[k]} is adjacent: slot k + 1 is 16 bytes further
        s0, s1, slot = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.call("spmv_hip_pcg_ws_rz_rr", ws, 0, C.byref(s0))
        _lib.call("spmv_hip_pcg_ws_rz_rr", ws, 1, C.byref(s1))
        assert s1.value - s0.value == 16
        assert h.spmv_hip_pcg_ws_rz_rr(ws, 6, C.byref(slot)) == -1
        assert h.spmv_hip_pcg_ws_rz_rr(ws, -1, C.byref(slot)) == -1
        assert h.spmv_hip_pcg_ws_pAp(ws, 6, C.byref(slot)) == -1
        assert h.spmv_hip_pcg_reduce_pAp(ctx, ws, 0, None) == -1
        assert h.spmv_hip_pcg_reduce_pAp(ctx, ws, 6, None) == -1
        assert h.spmv_hip_pcg_reduce_pAp2(ctx, ws, 6, s0, None) == -1
        assert h.spmv_hip_pcg_reduce_rz_rr(ctx, ws, 6, None) == -1
        assert h.spmv_hip_pcg_reduce_rz_rr(ctx, ws, -1, None) == -1
        for k in (0, 6):
            assert h.spmv_hip_pcg_update_r_f64(ctx, ws, k, 4, s0, s0, s0,
                                               None) == -1
            assert h.spmv_hip_pcg_update_xp_f64(ctx, ws, k, 4, s0, s0, s0, s0,
                                                None) == -1
            assert h.spmv_hip_pcg_update_r_cs_f64(ctx, ws, k, 4, s0, s0, s0,
                                                  None, None) == -1
            assert h.spmv_hip_pcg_update_xp_cs_f64(ctx, ws, k, 4, s0, s0, s0,
                                                   s0, None) == -1
        exec_.synchronize()
        _lib.call("spmv_hip_pcg_ws_read_async", ws, fp, zp, 12, None)
        exec_.synchronize()
        assert flags[0] == 0 and np.all(zr == 0.0)  # nothing ran
    finally:
        exec_.synchronize()
        _lib.call("spmv_hip_pcg_ws_destroy", ws)


# ---- 8. several ranks -----------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_pcg(world):
    """Ranks as threads (tests/thread_world.py), the scaled Poisson matrix in
    slabs, both storages, a blocking and an overlapping halo model, ONE
    workspace per rank over all solves; against the numpy reference on
    oracle.dist_spmv with the rank-ordered all-reduce of oracle.dist_cg."""
    from thread_world import ThreadWorld
    (rp, ci, va), diag = _slab_inputs(8)
    N = len(rp) - 1
    norm_a = _norm_inf((rp, ci, va))
    rng = np.random.default_rng(world)
    bs = [oracle.csr_spmv(rp, ci, va, np.ones(N)),
          oracle.csr_spmv(rp, ci, va, rng.uniform(-1, 1, N))]
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)

    def dist_dot(a, b):
        s = 0.0
        for r in range(world):
            s += oracle.ddot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
        return s

    refs = {(sym, cm): [_pcg_ref(lambda p: oracle.dist_spmv(world, rp, ci, va, p,
                                                            sym, cm),
                                 dist_dot, b, 1.0 / diag, KMAX, RTOL)
                        for b in bs]
            for sym in (False, True) for cm in models}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        ws = host.PcgWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for (sym, cm), ref in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, cm)
            A.diagonal(d_dinv)
            host.jacobi_inverse(exec_, d_dinv, d_dinv, M)
            for j, b in enumerate(bs):
                exec_.copy_from_host(d_b, b[r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist = host.pcg(comm, exec_, A, d_b, d_x + 8 * GUARD, d_dinv,
                                   KMAX, RTOL, ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k]))
                assert np.all(ks == k), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX
                _vs_oracle(k, hist, xs, ref[j], KMAX, RTOL, norm_a,
                           (world, sym, cm, j))
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
