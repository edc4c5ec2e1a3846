"""spmv::cg_block: CG for a block of nrhs interleaved right-hand sides, nrhs
independent recurrences in lockstep on Matrix::mult_block.

Shapes are those of test_gpu_cg_defer_x.py, the smallest that reach every
branch of the streaming loop: 1 331 rows (odd; at nrhs = 1 less than one unit
of 2 048 doubles), 13 824 rows, 4 097 rows (odd).  nrhs = 2, 4, 8 run the
streaming kernels, 1 and 3 the run-time-width kernels; both instantiations
(cached / non-temporal) of every kernel run through `blas1_nt_min_elems`.

X is overwritten with a sentinel before every solve, so a kernel that did
nothing cannot pass.  The ghost tail of P belongs to the workspace and cannot
be reached from here: the distributed test keeps ONE workspace per rank over
all its solves, so every solve but the first starts on the tail (and the R,
AP, P) another block left behind.

Bars against the oracle are the project's own (test_gpu_matrix._cg_vs_oracle):
|k_c - k_ref| <= 1, residual history to 1e-6 relative over the compared
entries, ||x_c - x_ref|| <= 1e-8 ||x_ref||.  The history is compared over the
entries 0 .. m - 1, m = min(k, k_ref, 50), and over entry m as well unless the
reference's ||r_m|| is below 8 u ||A||_inf ||x_ref||_2 (u = 2^-53): the
rounding error of evaluating A x itself on rows of at most 7 entries.  A
residual that small (the eigenvector column after its single step: 1.5e-14
||r_0|| at n = 24) is rounding noise that no second implementation reproduces
to a relative 1e-6."""
import ctypes as C

import numpy as np
import pytest

import oracle
from spmv_amd import _lib, host, poisson

pytestmark = pytest.mark.gpu

NT_DEFAULT = 1 << 24  # common.h: blas1_nt_min_elems
SENTINEL = 777.0
U = 2.0 ** -53
KMAX, RTOL = 120, 1e-10


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
    irrational values."""
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


def _sine_mode(n):
    """The lowest eigenvector of the 7-point operator on the n^3 grid: a
    product of sines.  CG on it stops after one step."""
    s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
    return np.einsum("i,j,k->ijk", s, s, s).reshape(-1).copy()


def _columns(csr, N, n_grid):
    """name -> right-hand side; they differ on purpose"""
    rng = np.random.default_rng(N)
    cols = {"ones": oracle.csr_spmv(*csr, np.ones(N)), "zero": np.zeros(N)}
    for j in range(7):
        cols[f"rand{j}"] = oracle.csr_spmv(*csr, rng.uniform(-1, 1, N))
    if n_grid:
        cols["eig"] = _sine_mode(n_grid)
    return cols


class _Problem:
    def __init__(self, exec_, comm, name):
        self.name, self.exec_ = name, exec_
        self.poisson = name.startswith("poisson")
        self.n = int(name[7:]) if self.poisson else 0
        if self.poisson:
            rp, ci, va = poisson.poisson3d_csr(self.n)
            self.N = self.n ** 3
        else:
            self.N = int(name[6:])
            rp, ci, va = _banded_spd(self.N)
        self.csr = (np.asarray(rp).astype(np.int32),
                    np.asarray(ci).astype(np.int32), np.asarray(va))
        self.cols = _columns(self.csr, self.N, self.n)
        self.norm_a = float(np.add.reduceat(np.abs(self.csr[2]),
                                            self.csr[0][:-1]).max())
        self.A = {False: host.Matrix.create_matrix(
            comm, exec_, rp, ci, va, self.N, self.N, [], [], False,
            host.P2P_NONBLOCKING)}
        if self.poisson:
            self.A[True] = host.Matrix.create_poisson3d(
                comm, exec_, self.n, True, host.P2P_NONBLOCKING)
        self.d_b = exec_.alloc(self.N * 8)
        self.d_x = exec_.alloc(self.N * 8 + 2)
        self.ws = host.CgBlockWorkspace(exec_)
        self._ref = {}

    def ref(self, col, symmetric=False, kmax=KMAX, rtol=RTOL):
        """oracle.cg on one column, computed once: (x, k, history)"""
        key = (col, symmetric, kmax, rtol)
        if key not in self._ref:
            if col == "zero":  # the rule of cg.h: stopped at k = 0 with x = 0
                self._ref[key] = (np.zeros(self.N), 0, np.zeros(1))
            elif symmetric:
                rp, ci, va, dg = oracle.poisson3d_lower(self.n)
                self._ref[key] = oracle.cg(rp, ci, va, self.cols[col], kmax,
                                           rtol, diagonal=dg)
            else:
                self._ref[key] = oracle.cg(*self.csr, self.cols[col], kmax, rtol)
        return self._ref[key]

    def solve(self, comm, names, kmax=KMAX, rtol=RTOL, symmetric=False, ws=None,
              x_off=0, **kw):
        """-> (iterations, history[nrhs, kmax + 1], X[N, nrhs]); x_off in
        doubles from the 256-byte aligned buffer"""
        e, nrhs = self.exec_, len(names)
        B = np.stack([self.cols[c] for c in names], axis=1)
        e.copy_from_host(self.d_b, B)
        e.copy_from_host(self.d_x, np.full(self.N * 8 + 2, SENTINEL))
        d_x = self.d_x + 8 * x_off
        its, hist, _ = host.cg_block(comm, e, self.A[symmetric], self.d_b, d_x,
                                     nrhs, kmax, rtol, ws or self.ws, **kw)
        X = e.copy_to_host(d_x, self.N * nrhs).reshape(self.N, nrhs)
        guard = e.copy_to_host(self.d_x, self.N * 8 + 2)
        lo, hi = x_off, x_off + self.N * nrhs
        assert np.all(guard[:lo] == SENTINEL) and np.all(guard[hi:] == SENTINEL)
        assert np.all(np.isfinite(X)) and not np.any(X == SENTINEL), names
        return its.copy(), hist.copy(), X

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        self.exec_.free(self.d_b)
        self.exec_.free(self.d_x)


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


def _check_history_tail(its, hist, what):
    """valid entries up to iterations[c], -1.0 beyond"""
    for c, k in enumerate(its):
        assert np.all(hist[c, :k + 1] >= 0.0), (what, c)
        assert np.all(hist[c, k + 1:] == -1.0), (what, c)


def _noise_floor(norm_a, x_ref):
    """see the top of the file"""
    return 8 * U * norm_a * np.linalg.norm(x_ref)


def _vs_oracle(k, hist_c, x_c, ref, kmax, rtol, norm_a, what):
    x_ref, k_ref, hist_ref = ref
    print(what, "k", k, "k_ref", k_ref)
    assert abs(k - k_ref) <= 1, (what, k, k_ref)
    if 0 < k < kmax:
        assert hist_c[k] / hist_c[0] < rtol, what
    if k_ref == 0:  # the zero column
        assert k == 0 and np.all(x_c == 0.0), what
        return
    m = min(k, k_ref, 50)
    upto = m + 1 if hist_ref[m] >= _noise_floor(norm_a, x_ref) else m
    dev = np.abs(hist_c[:upto] / hist_ref[:upto] - 1)
    print(what, "history deviation", dev.max())
    assert np.all(dev <= 1e-6), (what, dev.max())
    err = np.linalg.norm(x_c - x_ref) / np.linalg.norm(x_ref)
    print(what, "x error", err)
    assert err <= 1e-8, (what, err)


def _block_names(P, nrhs):
    pool = ["ones", "rand0", "eig" if P.poisson else "rand6", "rand1", "rand2",
            "rand3", "rand4", "rand5"]
    return pool[:nrhs]


# ---- 1. against the oracle, per column ---------------------------------------
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_oracle_per_column(comm, problems, nt, shape, nrhs):
    P = problems[shape]
    names = _block_names(P, nrhs)
    for symmetric in sorted(P.A):
        its, hist, X = P.solve(comm, names, symmetric=symmetric)
        _check_history_tail(its, hist, (shape, nrhs, symmetric))
        for c, col in enumerate(names):
            _vs_oracle(int(its[c]), hist[c], X[:, c], P.ref(col, symmetric),
                       KMAX, RTOL, P.norm_a, (shape, nrhs, symmetric, col))
        if "eig" in names:
            assert its[names.index("eig")] == 1
        # the native multi-vector kernel is the one under the solver where it
        # applies: general fp64 storage, nrhs = 2, 4, 8
        native = not symmetric and nrhs in (2, 4, 8)
        assert P.A[symmetric].plan_get("mv_form") == (1 if native else 2)


# ---- 2. columns stop at different k --------------------------------------------
@pytest.mark.parametrize("shape", ["poisson11", "poisson24"])
def test_columns_stop_at_different_k(comm, problems, nt, shape):
    """An eigenvector column (k = 1), a zero column (k = 0) and two slow ones,
    kmax far beyond the last stop.  poll_every = 255: every iteration is
    enqueued, so every kernel launched after a column stopped had the chance
    to touch it; poll_every = 1: the host stops enqueuing early."""
    P = problems[shape]
    names = ["eig", "zero", "ones", "rand0"]
    refs = [P.ref(c, kmax=250) for c in names]
    kmax = max(r[1] for r in refs) + 60
    assert max(r[1] for r in refs) < 250 and kmax < 255
    for poll in (255, 1):
        its, hist, X = P.solve(comm, names, kmax=kmax, poll_every=poll)
        what = (shape, poll)
        for c in range(4):
            assert abs(int(its[c]) - refs[c][1]) <= 1, (what, c, its, refs[c][1])
        assert its[0] == 1 and its[1] == 0 and np.all(X[:, 1] == 0.0), what
        assert hist[1, 0] == 0.0
        _check_history_tail(its, hist, what)
        assert its.max() < kmax
        # every column that stopped before the last one was frozen: its x is
        # the x of a solve that ends at its k
        last = int(its.max())
        for c in range(4):
            if its[c] == last:
                continue
            its2, hist2, X2 = P.solve(comm, names, kmax=int(its[c]))
            assert its2[c] == its[c], (what, c)
            assert np.array_equal(X2[:, c], X[:, c]), (what, c)
            assert np.array_equal(hist2[c, :its[c] + 1], hist[c, :its[c] + 1])


# ---- 3. independence ---------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [4, 3])
@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_a_column_does_not_see_the_others(comm, problems, nt, shape, nrhs):
    """Column `keep` in slot c, beside two sets of other columns: one of them
    becomes zero (stops earlier), one that was zero becomes a slow column
    (stops later), on Poisson a slow one becomes the eigenvector.  The kept
    column's x, history and count keep their bits."""
    P = problems[shape]
    first = ["rand1", "zero", "ones"][:nrhs - 1]
    second = ["zero", "rand2", "eig" if P.poisson else "rand1"][:nrhs - 1]
    for slot in range(nrhs):
        a = first[:slot] + ["rand0"] + first[slot:]
        b = second[:slot] + ["rand0"] + second[slot:]
        its_a, hist_a, X_a = P.solve(comm, a)
        its_b, hist_b, X_b = P.solve(comm, b)
        what = (shape, nrhs, slot)
        assert its_a[slot] == its_b[slot] and 1 < its_a[slot] < KMAX, what
        assert np.array_equal(hist_a[slot], hist_b[slot]), what
        assert np.array_equal(X_a[:, slot], X_b[:, slot]), what
        # the others did change the way they were meant to
        oa, ob = np.delete(its_a, slot), np.delete(its_b, slot)
        assert ob[0] == 0 < oa[0] and oa[1] == 0 < ob[1], (what, oa, ob)
        if nrhs == 4 and P.poisson:
            assert ob[2] == 1 < oa[2], (what, oa, ob)


# ---- 4. rtol = 0 ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape):
    P = problems[shape]
    for nrhs in (1, 2, 3, 4, 8):
        names = ["ones", "rand0", "rand1", "rand2", "rand3", "rand4", "rand5",
                 "rand6"][:nrhs]
        for kmax in (0, 1, 2, 7):
            its, hist, X = P.solve(comm, names, kmax=kmax, rtol=0.0)
            what = (shape, nrhs, kmax)
            assert np.all(its == kmax), (what, its)
            assert hist.shape == (nrhs, kmax + 1) and np.all(hist > 0.0), what
            for c in range(nrhs):
                assert np.any(X[:, c] != 0.0) == (kmax > 0), (what, c)


# ---- 5. workspace reuse and growth ----------------------------------------------------
def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


def test_workspace_reused_and_grown(comm, problems, nt):
    """One workspace across shapes (small, large, middle), across nrhs
    (4 -> 8 -> 2) and across a smaller kmax: every result equals the one on a
    fresh workspace, bit for bit."""
    e = problems["poisson11"].exec_
    shared = host.CgBlockWorkspace(e)
    plan = [("poisson11", 4, 30), ("poisson24", 8, 40), ("banded4097", 2, 12),
            ("poisson24", 4, 7), ("poisson11", 3, 40), ("poisson11", 8, 0)]
    for shape, nrhs, kmax in plan:
        P = problems[shape]
        names = ["rand0", "ones", "rand1", "zero", "rand2", "rand3", "rand4",
                 "rand5"][:nrhs]
        fresh = host.CgBlockWorkspace(e)
        want = P.solve(comm, names, kmax=kmax, rtol=1e-6, ws=fresh)
        fresh.close()
        got = P.solve(comm, names, kmax=kmax, rtol=1e-6, ws=shared)
        _same(want, got, (shape, nrhs, kmax))
    shared.close()


# ---- 6. unaligned X ---------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [4, 3])
def test_unaligned_x_keeps_the_bits(comm, problems, nt, nrhs):
    for shape in ("poisson11", "banded4097"):
        P = problems[shape]
        names = ["rand0", "ones", "zero", "rand1"][:nrhs]
        want = P.solve(comm, names, kmax=25)
        got = P.solve(comm, names, kmax=25, x_off=1)  # X + 8 bytes
        _same(want, got, (shape, nrhs))


# ---- 7. errors ----------------------------------------------------------------------------
def _current_stream(exec_):
    s = C.c_void_p()
    _lib.call("spmv_hip_get_stream", exec_.context, C.byref(s))
    return s.value


def test_errors_leave_the_executor_as_it_was(comm, problems):
    P = problems["poisson11"]
    e, A, N = P.exec_, P.A[False], P.N
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)
    try:
        e.copy_from_host(P.d_b, np.ones(N * 8))
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.cg_block(comm, e, A, P.d_b, P.d_b, 4, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.cg_block(comm, e, A, P.d_b, P.d_b + 8 * (4 * N - 2), 4, 5, 1e-10)
        for nrhs in (0, 9):
            with pytest.raises(host.SpmvHostError, match="nrhs"):
                host.cg_block(comm, e, A, P.d_b, P.d_x, nrhs, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.cg_block(comm, e, A, P.d_b, P.d_x, 4, -1, 1e-10)
        assert _current_stream(e) == mine.value
        # ... and after a solve that went through
        its, _, _ = host.cg_block(comm, e, A, P.d_b, P.d_x, 4, 3, 0.0, P.ws)
        assert np.all(its == 3)
        assert _current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


def test_abi_refuses_short_destinations_and_bad_iterations(exec_):
    """spmv_hip_cgb_ws_read_async copies nothing into a buffer that is too
    short; slots and kernels refuse an iteration outside 0..kmax."""
    h, ctx = _lib.hip, exec_.context
    ws = C.c_void_p()
    _lib.call("spmv_hip_cgb_ws_create", ctx, 5, 3, C.byref(ws))
    try:
        kmax, nrhs = C.c_int(), C.c_int()
        _lib.call("spmv_hip_cgb_ws_capacity", ws, C.byref(kmax), C.byref(nrhs))
        assert (kmax.value, nrhs.value) == (5, 3)
        state = np.full(17, 99, np.int32)
        rr = np.full(18, -7.0)
        sp, rp = state.ctypes.data_as(C.c_void_p), rr.ctypes.data_as(C.c_void_p)
        assert h.spmv_hip_cgb_ws_read_async(ws, sp, 16, None, 0, None) == -1
        assert h.spmv_hip_cgb_ws_read_async(ws, None, 0, rp, 17, None) == -1
        assert h.spmv_hip_cgb_ws_read_async(ws, sp, 17, rp, 17, None) == -1
        exec_.synchronize()
        assert np.all(state == 99) and np.all(rr == -7.0)
        _lib.call("spmv_hip_cgb_ws_reset", ws, 1e-8, None)
        _lib.call("spmv_hip_cgb_ws_read_async", ws, sp, 17, rp, 18, None)
        exec_.synchronize()
        assert state[0] == 0 and np.all(state[1:9] == 0)
        assert np.all(state[9:] == -1) and np.all(rr == 0.0)
        slot = C.c_void_p()
        assert h.spmv_hip_cgb_ws_rr(ws, 6, C.byref(slot)) == -1
        assert h.spmv_hip_cgb_ws_pAp(ws, -1, C.byref(slot)) == -1
        assert h.spmv_hip_cgb_reduce_pAp(ctx, ws, 0, None) == -1
        assert h.spmv_hip_cgb_reduce_rr(ctx, ws, 6, None) == -1
        assert h.spmv_hip_cgb_update_r_f64(ctx, ws, 6, 4, None, None, None) == -1
    finally:
        exec_.synchronize()
        _lib.call("spmv_hip_cgb_ws_destroy", ws)


# ---- 8. several ranks -----------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_cg_block(world):
    """Ranks as threads (tests/thread_world.py), the Poisson matrix in slabs,
    both storages, a blocking and an overlapping halo model; every column
    against oracle.dist_cg with the bars of
    test_gpu_matrix.test_slab_ranks_threaded_spmv_and_cg."""
    from thread_world import ThreadWorld
    n, kmax, rtol = 8, 200, 1e-10
    N = n ** 3
    rp, ci, va = poisson.poisson3d_csr(n)
    csr = (rp, ci.astype(np.int32), va)
    rng = np.random.default_rng(world)
    cols = [oracle.csr_spmv(*csr, np.ones(N)),
            oracle.csr_spmv(*csr, rng.uniform(-1, 1, N)), _sine_mode(n),
            oracle.csr_spmv(*csr, rng.uniform(-1, 1, N))]
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    refs = {(sym, cm): [oracle.dist_cg(world, rp, ci, va, b, kmax, rtol, sym, cm)
                        for b in cols]
            for sym in (False, True) for cm in models}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.CgBlockWorkspace(exec_)
        d_b, d_x = exec_.alloc(M * 4), exec_.alloc(M * 4)
        for (sym, cm), ref in refs.items():
            A = host.Matrix.create_poisson3d(comm, exec_, n, sym, cm)
            for nrhs in (4, 3):
                B = np.stack([b[r0:r1] for b in cols[:nrhs]], axis=1)
                exec_.copy_from_host(d_b, B)
                exec_.copy_from_host(d_x, np.full(M * 4, SENTINEL))
                its, hist, _ = host.cg_block(comm, exec_, A, d_b, d_x, nrhs,
                                             kmax, rtol, ws)
                X = exec_.copy_to_host(d_x, M * nrhs).reshape(M, nrhs)
                all_its = tw.gather(rank, its).reshape(world, nrhs)
                assert np.all(all_its == all_its[0]), all_its
                _check_history_tail(its, hist, (sym, cm, nrhs))
                for c in range(nrhs):
                    xs = tw.gather(rank, np.ascontiguousarray(X[:, c]))
                    x_ref, k_ref, hist_ref = ref[c]
                    k = int(its[c])
                    what = (world, sym, cm, nrhs, c)
                    assert abs(k - k_ref) <= 1 and k < kmax, (what, k, k_ref)
                    m = min(k, k_ref, 50)
                    # (the 7-point operator: ||A||_inf = 12)
                    upto = m + 1 if hist_ref[m] >= _noise_floor(12.0, x_ref) else m
                    assert np.allclose(hist[c, :upto], hist_ref[:upto],
                                       rtol=1e-6, atol=0.0), what
                    assert (np.linalg.norm(xs - x_ref)
                            <= 1e-8 * np.linalg.norm(x_ref)), what
                assert its[2] == 1  # the eigenvector column
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
