"""spmv::pcg_block: preconditioned CG for a block of nrhs interleaved right-hand
sides -- pcg_sgs's recurrence once per column, in lockstep on
Matrix::mult_block, with a diagonal, an SGS or an ILU(0) preconditioner.

Shapes are cg_block's (the smallest that reach every branch of the streaming
loop): 1 331 rows (odd), 13 824 rows, 4 097 rows (odd), and ragged3001 (long
rows, 24+ colours) for the SGS form.  nrhs = 2, 4, 8 run the streaming kernels
and the compiled widths of the block sweeps, 1 and 3 the run-time-width forms;
both instantiations (cached / non-temporal) of every vector kernel run through
`blas1_nt_min_elems`.  X sits between guard words and is overwritten with a
sentinel before every solve.

Every column is compared with the numpy restatement of pcg_block_cases.py
(computed once per column, shared by the tests) through
test_gpu_chebyshev._vs_ref unchanged: |k - k_ref| <= 1, history to 1e-6 over
min(k, k_ref, 50) entries above the noise floor, ||x - x_ref|| <= 1e-8
||x_ref||.  dev_ref, the restatement's own deviation between the two summation
orders _vs_ref uses, was computed on the CPU for every (matrix, preconditioner,
column) held to the history bar here (test_pcg_block_host.py asserts it stays
below 1e-7, a tenth of the bar, so the bar is never widened, and names the two
columns that were replaced for that reason).  Over every compared entry, the
last one included, the largest is 6.0e-8 (two ranks, b = A 1); on one rank
1.5e-8 (poisson24, ILU(0), b = A 1), every other case below 1e-8."""
import ctypes as C

import numpy as np
import pytest

import pcg_block_cases as pc
import test_gpu_cg_block as tb
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from spmv_amd import _lib, host
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = pc.KMAX, pc.RTOL
SHAPES, KINDS, NRHS = pc.SHAPES, pc.KINDS, pc.NRHS


class _Problem:
    """One matrix of pcg_block_cases in both storages with its device
    preconditioners and buffers."""

    def __init__(self, exec_, comm, name):  # noqa: F811
        self.name, self.exec_ = name, exec_
        self.case = P = pc.case(name)
        self.N = N = P.N
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *P.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.M = {}
        for sym, A in self.A.items():
            self.M[("sgs", sym)] = host.SgsPreconditioner(exec_, A)
            if name in SHAPES:
                self.M[("ilu0", sym)] = host.Ilu0Preconditioner(exec_, A)
        for M in self.M.values():  # the restatement sweeps in these colours
            assert np.array_equal(M.colors(), P.colours), name
        self.d_dinv = exec_.alloc(N + 1)
        exec_.copy_from_host(self.d_dinv, P.dinv)
        self.d_b = exec_.alloc(N * 8)
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD + 1)
        self.ws = host.PcgBlockWorkspace(exec_)

    def pre(self, kind, symmetric):
        """the preconditioner arguments of host.pcg_block"""
        if kind == "dinv":
            return dict(dinv=self.d_dinv)
        return dict(sgs=self.M[(kind, symmetric)])

    def solve(self, comm, kind, names, kmax=KMAX, rtol=RTOL,  # noqa: F811
              symmetric=False, ws=None, x_off=GUARD, **kw):
        """-> (iterations, history[nrhs, kmax + 1], X[N, nrhs]); x_off in
        doubles (GUARD: 16-byte aligned, GUARD + 1: 8 bytes off)"""
        e, N, nrhs = self.exec_, self.N, len(names)
        size = N * 8 + 2 * GUARD + 1
        e.copy_from_host(self.d_b, self.case.block(names))
        e.copy_from_host(self.d_x, np.full(size, SENTINEL))
        d_x = self.d_x + 8 * x_off
        its, hist, _ = host.pcg_block(comm, e, self.A[symmetric], self.d_b, d_x,
                                      nrhs, kmax, rtol, workspace=ws or self.ws,
                                      **self.pre(kind, symmetric), **kw)
        buf = e.copy_to_host(self.d_x, size)
        lo, hi = x_off, x_off + N * nrhs
        assert np.all(buf[:lo] == SENTINEL) and np.all(buf[hi:] == SENTINEL)
        X = buf[lo:hi].reshape(N, nrhs).copy()
        assert np.all(np.isfinite(X)) and not np.any(X == SENTINEL), names
        return its.copy(), hist.copy(), X

    def vs_ref(self, kind, names, its, hist, X, what, kmax=KMAX, rtol=RTOL):
        tb._check_history_tail(its, hist, what)
        for c, col in enumerate(names):
            k = int(its[c])
            ref = self.case.ref(kind, col, kmax, rtol)
            if col == "zero":
                assert k == 0 and hist[c, 0] == 0.0 and np.all(X[:, c] == 0.0)
                continue
            tc._vs_ref(k, hist[c, :k + 1], X[:, c], ref, self.case.norm_a,
                       what + (col,), kmax, rtol)

    def close(self):
        self.ws.close()
        for M in self.M.values():
            M.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_dinv, self.d_b, self.d_x):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Problem(exec_, comm, name)
        return made[name]
    yield get
    for p in made.values():
        p.close()


# ---- 1. per column against the restatement ------------------------------------------
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_per_column_against_the_restatement(comm, problems, nt,  # noqa: F811
                                            shape, kind, nrhs):
    P = problems(shape)
    names = P.case.pool(kind)[:nrhs]
    for symmetric in (False, True):
        its, hist, X = P.solve(comm, kind, names, symmetric=symmetric)
        assert its.max() < KMAX
        P.vs_ref(kind, names, its, hist, X, (shape, kind, nrhs, symmetric))


@pytest.mark.parametrize("nrhs", [4, 3])
def test_on_the_ragged_matrix(comm, problems, nt, nrhs):  # noqa: F811
    P = problems("ragged3001")
    names = P.case.pool("sgs")[:nrhs]
    for symmetric in (False, True):
        its, hist, X = P.solve(comm, "sgs", names, symmetric=symmetric)
        assert its.max() < KMAX
        P.vs_ref("sgs", names, its, hist, X, ("ragged", nrhs, symmetric))


# ---- 2. independence -------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [4, 3])
@pytest.mark.parametrize("kind", ["sgs", "dinv"])
@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_a_column_does_not_see_the_others(comm, problems, nt,  # noqa: F811
                                          shape, kind, nrhs):
    """Column `keep` in slot c, beside two sets of other columns: one of them
    becomes zero (stops earlier), one that was zero becomes a slow column
    (stops later), on Poisson a slow one becomes the eigenvector.  The kept
    column's x, history and count keep their bits."""
    P = problems(shape)
    first = ["rand1", "zero", "ones"][:nrhs - 1]
    second = ["zero", "rand2", "eig" if P.case.n_grid else "rand1"][:nrhs - 1]
    for slot in range(nrhs):
        a = first[:slot] + ["rand0"] + first[slot:]
        b = second[:slot] + ["rand0"] + second[slot:]
        its_a, hist_a, X_a = P.solve(comm, kind, a)
        its_b, hist_b, X_b = P.solve(comm, kind, b)
        what = (shape, kind, nrhs, slot)
        assert its_a[slot] == its_b[slot] and 1 < its_a[slot] < KMAX, what
        assert np.array_equal(hist_a[slot], hist_b[slot]), what
        assert np.array_equal(X_a[:, slot], X_b[:, slot]), what
        # the others did change the way they were meant to
        oa, ob = np.delete(its_a, slot), np.delete(its_b, slot)
        assert ob[0] == 0 < oa[0] and oa[1] == 0 < ob[1], (what, oa, ob)
        if nrhs == 4 and P.case.n_grid:
            assert ob[2] < oa[2], (what, oa, ob)


# ---- 3. columns stop at different k ------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["poisson11", "poisson24"])
def test_columns_stop_at_different_k(comm, problems, nt, shape, kind):  # noqa: F811
    """An eigenvector column, a zero column (k = 0) and two slow ones, kmax far
    beyond the last stop.  poll_every = 255: every iteration is enqueued, so
    every kernel launched after a column stopped had the chance to touch it;
    poll_every = 1: the host stops enqueuing early."""
    P = problems(shape)
    names = ["eig", "zero", "ones", "rand0"]
    ks = [P.case.ref(kind, c).k for c in names]
    kmax = max(ks) + 60
    assert max(ks) < KMAX and kmax < 255 and len(set(ks)) == 4
    for poll in (255, 1):
        its, hist, X = P.solve(comm, kind, names, kmax=kmax, poll_every=poll)
        what = (shape, kind, poll)
        for c in range(4):
            assert abs(int(its[c]) - ks[c]) <= 1, (what, c, its, ks)
        assert its[1] == 0 and np.all(X[:, 1] == 0.0) and hist[1, 0] == 0.0, what
        tb._check_history_tail(its, hist, what)
        assert its.max() < kmax
        # every column that stopped before the last one was frozen: its x is
        # the x of a solve cut at its k
        last = int(its.max())
        for c in range(4):
            if its[c] == last:
                continue
            its2, hist2, X2 = P.solve(comm, kind, names, kmax=int(its[c]))
            assert its2[c] == its[c], (what, c)
            assert np.array_equal(X2[:, c], X[:, c]), (what, c)
            assert np.array_equal(hist2[c, :its[c] + 1], hist[c, :its[c] + 1])


# ---- 4. rtol = 0 ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape, kind):  # noqa: F811
    P = problems(shape)
    for nrhs in NRHS:
        names = ["ones", "rand0", "rand1", "rand2", "rand3", "rand4", "rand5",
                 "rand6"][:nrhs]
        for kmax in (0, 1, 2, 7):
            its, hist, X = P.solve(comm, kind, names, kmax=kmax, rtol=0.0)
            what = (shape, kind, nrhs, kmax)
            assert np.all(its == kmax), (what, its)
            assert hist.shape == (nrhs, kmax + 1) and np.all(hist > 0.0), what
            for c in range(nrhs):
                assert np.any(X[:, c] != 0.0) == (kmax > 0), (what, c)
    # the history of a cut solve is the reference's
    ref = P.case.ref(kind, "ones", 7, 0.0)
    assert np.allclose(hist[0], ref.hist, rtol=1e-6, atol=0.0), (shape, kind)


# ---- 5. workspace reuse and growth, alignment ------------------------------------------------
def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


def test_workspace_reused_and_grown(comm, problems, nt):  # noqa: F811
    """One workspace across shapes (small, large, middle), across nrhs, across
    preconditioners and across a smaller kmax: every result equals the one on
    a fresh workspace, bit for bit."""
    e = problems("poisson11").exec_
    shared = host.PcgBlockWorkspace(e)
    plan = [("poisson11", "sgs", 4, 30), ("poisson24", "dinv", 8, 40),
            ("banded4097", "ilu0", 2, 12), ("poisson24", "sgs", 4, 7),
            ("poisson11", "dinv", 3, 40), ("poisson11", "ilu0", 8, 0)]
    for shape, kind, nrhs, kmax in plan:
        P = problems(shape)
        names = ["rand0", "ones", "rand1", "zero", "rand2", "rand3", "rand4",
                 "rand5"][:nrhs]
        fresh = host.PcgBlockWorkspace(e)
        want = P.solve(comm, kind, names, kmax=kmax, rtol=1e-6, ws=fresh)
        fresh.close()
        got = P.solve(comm, kind, names, kmax=kmax, rtol=1e-6, ws=shared)
        _same(want, got, (shape, kind, nrhs, kmax))
    shared.close()


@pytest.mark.parametrize("nrhs", [4, 3])
def test_unaligned_x_keeps_the_bits(comm, problems, nt, nrhs):  # noqa: F811
    for shape in ("poisson11", "banded4097"):
        P = problems(shape)
        names = ["rand0", "ones", "zero", "rand1"][:nrhs]
        for kind in KINDS:
            want = P.solve(comm, kind, names, kmax=25)
            got = P.solve(comm, kind, names, kmax=25, x_off=GUARD + 1)
            _same(want, got, (shape, kind, nrhs))


# ---- 6. errors ------------------------------------------------------------------------------------
def test_errors_leave_the_executor_as_it_was(comm, problems):  # noqa: F811
    P = problems("poisson11")
    e, A, N = P.exec_, P.A[False], P.N
    sgs, ilu = P.M[("sgs", False)], P.M[("ilu0", False)]
    other = problems("banded4097").M[("sgs", False)]
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)

    def solve(b, x, nrhs=4, kmax=5, **pre):
        return host.pcg_block(comm, e, A, b, x, nrhs, kmax, 1e-10, **pre)
    try:
        e.copy_from_host(P.d_b, np.ones(N * 8))
        x = P.d_x + 8 * GUARD
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, P.d_b, sgs=sgs)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, P.d_b + 8 * (4 * N - 1), dinv=P.d_dinv)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, P.d_dinv - 8 * (4 * N - 1), dinv=P.d_dinv)
        for nrhs in (0, 9):
            with pytest.raises(host.SpmvHostError, match="nrhs"):
                solve(P.d_b, x, nrhs=nrhs, sgs=sgs)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            solve(P.d_b, x, kmax=-1, sgs=sgs)
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            solve(P.d_b, x)
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            solve(P.d_b, x, dinv=P.d_dinv, sgs=ilu)
        with pytest.raises(host.SpmvHostError, match="rows"):
            solve(P.d_b, x, sgs=other)
        assert tp._current_stream(e) == mine.value
        # ... and after a solve that went through
        its, _, _ = host.pcg_block(comm, e, A, P.d_b, x, 4, 3, 0.0, sgs=ilu,
                                   workspace=P.ws)
        assert np.all(its == 3)
        assert tp._current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


def test_negative_pivots_are_refused(exec_, comm):  # noqa: F811
    """An ILU(0) factor with a negative pivot is not positive definite: "pivot",
    before any launch (X keeps its sentinel)."""
    rp = np.array([0, 2, 4, 5], np.int32)
    ci = np.array([0, 1, 0, 1, 2], np.int32)
    va = np.array([1.0, 2.0, 2.0, 1.0, 3.0])  # second pivot 1 - 2 * 2 / 1 = -3
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, 3, 3, [], [], False,
                                  host.P2P_NONBLOCKING)
    M = host.Ilu0Preconditioner(exec_, A)
    assert M.negative_pivots() == 1
    d_b, d_x = exec_.alloc(6), exec_.alloc(6)
    exec_.copy_from_host(d_b, np.ones(6))
    exec_.copy_from_host(d_x, np.full(6, SENTINEL))
    with pytest.raises(host.SpmvHostError, match="pivot"):
        host.pcg_block(comm, exec_, A, d_b, d_x, 2, 5, 1e-10, sgs=M)
    exec_.synchronize()
    assert np.all(exec_.copy_to_host(d_x, 6) == SENTINEL)
    exec_.free(d_b), exec_.free(d_x)
    M.close()
    A.close()


def test_time_spmv_counts_one_mult_block_per_iteration(comm, problems):  # noqa: F811
    P = problems("poisson11")
    e = P.exec_
    e.copy_from_host(P.d_b, P.case.block(["ones", "rand0", "rand1", "rand2"]))
    _, _, stats = host.pcg_block(comm, e, P.A[False], P.d_b, P.d_x + 8 * GUARD,
                                 4, 5, 0.0, sgs=P.M[("sgs", False)],
                                 workspace=P.ws, time_spmv=True)
    assert stats["max_iterations"] == 5
    assert stats["spmv_launches"] == 5 and stats["spmv_ms_total"] > 0.0


# ---- 7. against the single-vector solvers ---------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_one_column_reaches_the_k_of_pcg_sgs_and_pcg(comm, problems,  # noqa: F811
                                                     shape):
    P = problems(shape)
    e, N = P.exec_, P.N
    d_x1 = e.alloc(N)
    for col in ("ones", "rand0"):
        e.copy_from_host(P.d_b, P.case.cols[col])
        k_sgs, _ = host.pcg_sgs(comm, e, P.A[False], P.M[("sgs", False)], P.d_b,
                                d_x1, KMAX, RTOL)
        x_sgs = e.copy_to_host(d_x1, N)
        k_jac, _ = host.pcg(comm, e, P.A[False], P.d_b, d_x1, P.d_dinv, KMAX,
                            RTOL)
        for kind, k_single in (("sgs", k_sgs), ("dinv", k_jac)):
            its, hist, X = P.solve(comm, kind, [col])
            print(shape, col, kind, "k", int(its[0]), "single", k_single)
            assert abs(int(its[0]) - k_single) <= 1, (shape, col, kind)
            if kind == "sgs":
                err = np.linalg.norm(X[:, 0] - x_sgs) / np.linalg.norm(x_sgs)
                assert err <= 1e-8, (shape, col, err)
    e.free(d_x1)


# ---- 8. several ranks --------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_pcg_block(world):
    """Ranks as threads (tests/thread_world.py), the Poisson matrix of 8^3 in
    slabs, both storages, a blocking and an overlapping halo model, nrhs = 4
    with the SGS preconditioner (block-Jacobi over the ranks), ONE workspace
    per rank over all solves; every column against the restatement on
    oracle.dist_spmv with the block-diagonal preconditioner and the
    rank-ordered sum."""
    from thread_world import ThreadWorld
    S = pc.slab_case(world)
    kmax, rtol, B, ranges, blocks = S.kmax, S.rtol, S.B, S.ranges, S.blocks
    refs, norm_a = S.refs, S.norm_a
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        ws = host.PcgBlockWorkspace(exec_)
        d_b = exec_.alloc(M * 4)
        d_x = exec_.alloc(M * 4 + 2 * GUARD)
        for (sym, cm), ref in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, cm)
            pre = host.SgsPreconditioner(exec_, A)
            exec_.copy_from_host(d_b, np.ascontiguousarray(B[r0:r1]))
            exec_.copy_from_host(d_x, np.full(M * 4 + 2 * GUARD, SENTINEL))
            its, hist, _ = host.pcg_block(comm, exec_, A, d_b, d_x + 8 * GUARD, 4,
                                          kmax, rtol, sgs=pre, workspace=ws)
            buf = exec_.copy_to_host(d_x, M * 4 + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL)
            assert np.all(buf[GUARD + M * 4:] == SENTINEL)
            X = buf[GUARD:GUARD + M * 4].reshape(M, 4)
            all_its = tw.gather(rank, its).reshape(world, 4)
            assert np.all(all_its == all_its[0]), all_its
            tb._check_history_tail(its, hist, (sym, cm))
            for c in range(4):
                xs = tw.gather(rank, np.ascontiguousarray(X[:, c]))
                k = int(its[c])
                assert k < kmax
                tc._vs_ref(k, hist[c, :k + 1], xs, ref[c], norm_a,
                           (world, sym, cm, c), kmax, rtol)
            pre.close()
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
