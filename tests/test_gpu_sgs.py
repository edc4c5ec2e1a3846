"""The multicolour symmetric Gauss-Seidel preconditioner: spmv::SgsPreconditioner,
sgs_apply and pcg_sgs.

Shapes, matrices and bars are those of test_gpu_pcg.py (its generators are
imported, not copied): 1 331 rows (odd), 13 824 rows, 4 097 rows (odd), each
plain and scaled to S A S, both storages; both instantiations (cached /
non-temporal) of the streaming kernels run through `blas1_nt_min_elems`.  One
numpy-built ragged matrix adds what those do not have: 3 001 rows (odd, not a
multiple of 64), many colours, colours of a single row, and two rows of about
500 entries for the long-row path of the sweeps; a diagonal matrix and n = 1
close the list.

sgs_apply has no reductions and inside a colour the rows are independent, so it
is compared with np.array_equal against the numpy restatement of cg.h, driven
by the colours read back from the object.  The restatement is vectorised per
colour with one numpy operation per entry slot (the k-th entry of every row of
the colour at once): every product and every sum is one rounding, in the
kernel's order.

pcg_sgs is compared against test_gpu_chebyshev._pcg_ref with precond = the
restatement, on oracle.csr_spmv / oracle.ddot, in two summation orders of the
dot product, through test_gpu_chebyshev._vs_ref unchanged: |k - k_ref| <= 1;
history to 1e-6 over min(k, k_ref, 50) entries above the noise floor --
max(1e-6, 10 * dev_ref) where dev_ref exceeds 1e-7, and a case with dev_ref >
1e-5 FAILS instead; ||x - x_ref|| <= 1e-8 ||x_ref||.  On the CPU the largest
dev_ref of the cases below is 1.5e-9 (poisson24, plain, b = A 1).

X, and z of sgs_apply, sit between guard words and are filled with a sentinel
before every call."""
import ctypes as C

import numpy as np
import pytest

import oracle
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from spmv_amd import _lib, host
from test_gpu_bicgstab import _dot_chunked
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = tp.KMAX, tp.RTOL
SHAPES = tp.SHAPES


# ---- cg.h restated in numpy -------------------------------------------------------
class Sweeps:
    """before(i) / after(i) of the local diagonal block (columns < n) of a CSR,
    as the storage holds them, grouped by the colour of the row and by the
    entry's slot in its part."""

    def __init__(self, csr, n, colours, symmetric):
        rp, ci, va = csr
        rows = tp._row_of(rp)[:len(ci)]
        if symmetric:  # the stored lower entries, then their mirror images
            low = ci < rows
            rows, cols, vals = (np.concatenate([rows[low], ci[low]]),
                                np.concatenate([ci[low], rows[low]]),
                                np.concatenate([va[low], va[low]]))
        else:
            keep = (ci < n) & (ci != rows)
            rows, cols, vals = rows[keep], ci[keep], va[keep]
        order = np.lexsort((cols, rows))  # stable: duplicates keep their order
        rows, cols, vals = rows[order], cols[order].astype(np.int64), vals[order]
        self.n, self.colours = n, np.asarray(colours)
        self.nc = int(self.colours.max()) + 1 if n else 0
        assert not np.any(self.colours[rows] == self.colours[cols])
        self.parts = []
        for sel in (self.colours[cols] < self.colours[rows],
                    self.colours[cols] > self.colours[rows]):
            r, c, v = rows[sel], cols[sel], vals[sel]
            first = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
            slot = np.arange(len(r)) - first[r]
            by_colour = []
            for colour in range(self.nc):
                mine = self.colours[r] == colour
                slots = []
                for k in range(int(slot[mine].max()) + 1 if mine.any() else 0):
                    m = mine & (slot == k)
                    slots.append((r[m], c[m], v[m]))
                by_colour.append(slots)
            self.parts.append(by_colour)
        self.rows_of = [np.flatnonzero(self.colours == c) for c in range(self.nc)]

    def _sum(self, part, colour, z):
        s = np.zeros(self.n)
        for r, c, v in self.parts[part][colour]:
            s[r] = s[r] + v * z[c]
        return s

    def apply(self, dinv, r):
        """z = M^-1 r"""
        z = np.full(self.n, np.nan)
        for colour in range(self.nc):
            i = self.rows_of[colour]
            s = self._sum(0, colour, z)
            z[i] = (r[i] - s[i]) * dinv[i]
        for colour in range(self.nc - 2, -1, -1):
            i = self.rows_of[colour]
            t = self._sum(1, colour, z)
            z[i] = z[i] - dinv[i] * t[i]
        return z


class _Ref(tc._Ref):
    """test_gpu_chebyshev._Ref with any preconditioner"""

    def __init__(self, spmv, dot, dot2, b, precond, kmax=KMAX, rtol=RTOL):
        self.x, self.k, self.hist = tc._pcg_ref(spmv, dot, b, precond, kmax, rtol)
        self.second = tc._pcg_ref(spmv, dot2, b, precond, kmax, rtol)


def ragged_spd(n=3001, seed=7):
    """Symmetric, strictly diagonally dominant, irregular: up to 20 partners
    chosen per row (row lengths 1 to about 60), two hub rows of about 500
    entries -- one early in the natural order (most of its entries come after
    it in the colour order), one late --, the last 24 rows all coupled to each
    other (24 colours at the least, the highest worn by single rows), and row 7
    without any off-diagonal entry."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        if i == 7:
            continue
        js = rng.integers(0, n, rng.integers(0, 21))
        a += [i] * len(js)
        b += js.tolist()
    for i in range(n - 24, n):
        a += [i] * (n - 1 - i)
        b += list(range(i + 1, n))
    for hub in (100, n - 501):
        js = rng.choice(n, 500, replace=False)
        a += [hub] * len(js)
        b += js.tolist()
    a, b = np.array(a), np.array(b)
    ok = (a != b) & (a != 7) & (b != 7)
    lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
    pairs = np.unique(lo * n + hi)
    lo, hi = pairs // n, pairs % n
    v = -rng.uniform(0.1, 1.0, len(pairs))
    rows = np.concatenate([lo, hi, np.arange(n)])
    cols = np.concatenate([hi, lo, np.arange(n)])
    off = np.bincount(np.concatenate([lo, hi]),
                      weights=np.abs(np.concatenate([v, v])), minlength=n)
    vals = np.concatenate([v, v, off + 1.0 + rng.uniform(0, 1, n)])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32), vals[order])


def _diagonal_matrix(n):
    i = np.arange(n)
    return (np.arange(n + 1).astype(np.int32), i.astype(np.int32),
            2.0 + np.sin(i) ** 2)


def _make_csr(name):
    if name == "ragged3001":
        return ragged_spd()
    if name.startswith("diag"):
        return _diagonal_matrix(int(name[4:]))
    return tp._csr(name)


class _Problem:
    """One matrix in both storages with its preconditioners, right-hand sides,
    buffers and references (computed once)."""

    def __init__(self, exec_, comm, name, scaled):
        self.name, self.exec_ = (name, "scaled" if scaled else "plain"), exec_
        csr = _make_csr(name)
        self.csr = tp._scaled(csr) if scaled else csr
        self.N = N = len(self.csr[0]) - 1
        self.dinv = 1.0 / tp._diag_of(self.csr)
        self.norm_a = tp._norm_inf(self.csr)
        rng = np.random.default_rng(N + 1)
        self.rhs = {"ones": self.spmv(np.ones(N)),
                    "rand": self.spmv(rng.uniform(-1, 1, N)),
                    "zero": np.zeros(N)}
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.M = {sym: host.SgsPreconditioner(exec_, A)
                  for sym, A in self.A.items()}
        self.sweeps = {}
        for sym, M in self.M.items():
            colours = M.colors()
            assert M.rows() == N and M.num_colors() == colours.max() + 1
            assert M.plan_bytes() >= 12 * N  # perm and dinv at the least
            self.sweeps[sym] = Sweeps(self.csr, N, colours, sym)
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.SgsWorkspace(exec_)
        self._ref = {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, v)

    def precond(self, r, symmetric=False):
        return self.sweeps[symmetric].apply(self.dinv, r)

    def ref(self, rhs, kmax=KMAX, rtol=RTOL):
        key = (rhs, kmax, rtol)
        if key not in self._ref:
            self._ref[key] = _Ref(self.spmv, oracle.ddot, _dot_chunked,
                                  self.rhs[rhs], self.precond, kmax, rtol)
        return self._ref[key]

    def _guarded(self, off):
        self.exec_.copy_from_host(self.d_x, np.full(self.N + 2 * GUARD, SENTINEL))
        return self.d_x + 8 * off

    def _read_guarded(self, off):
        N = self.N
        buf = self.exec_.copy_to_host(self.d_x, N + 2 * GUARD)
        assert np.all(buf[:off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[off + N:] == SENTINEL), (self.name, "guard behind")
        out = buf[off:off + N].copy()
        assert np.all(np.isfinite(out)) and not np.any(out == SENTINEL), self.name
        return out

    def apply(self, r, symmetric=False, r_off=0, z_off=GUARD, M=None):
        """-> z; r_off / z_off in doubles (1 / GUARD + 1: 8 bytes off)"""
        e = self.exec_
        e.copy_from_host(self.d_b + 8 * r_off, r)
        d_z = self._guarded(z_off)
        host.sgs_apply(e, M or self.M[symmetric], self.d_b + 8 * r_off, d_z)
        return self._read_guarded(z_off)

    def solve(self, comm, rhs, kmax=KMAX, rtol=RTOL, symmetric=False, ws=None,
              x_off=GUARD, **kw):
        """-> (k, history, x)"""
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist = host.pcg_sgs(comm, e, self.A[symmetric], self.M[symmetric],
                               self.d_b, d_x, kmax, rtol, ws or self.ws, **kw)
        x = self._read_guarded(x_off)
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x

    def close(self):
        self.ws.close()
        for M in self.M.values():
            M.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_b, self.d_x):
            self.exec_.free(p)


EXTRA = ("ragged3001", "diag200", "diag1")


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    ps = {(shape, scaled): _Problem(exec_, comm, shape, scaled)
          for shape in SHAPES for scaled in (False, True)}
    for name in EXTRA:
        ps[(name, False)] = _Problem(exec_, comm, name, False)
    yield ps
    for p in ps.values():
        p.close()


MATS = [pytest.param(False, id="plain"), pytest.param(True, id="scaled")]
STORAGE = [pytest.param(False, id="general"), pytest.param(True, id="symmetric")]
OFFSETS = ((0, GUARD), (1, GUARD + 1), (0, GUARD + 1), (1, GUARD))


# ---- 1. sgs_apply is exact ------------------------------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_is_exact(problems, shape, scaled, symmetric):
    P = problems[(shape, scaled)]
    if shape.startswith("poisson"):
        assert P.M[symmetric].num_colors() == 2
    # exactly symmetric: both storages hold the same rows
    assert np.array_equal(P.M[True].colors(), P.M[False].colors())
    for rhs in ("rand", "ones"):
        r = P.rhs[rhs]
        want = P.precond(r, symmetric)
        assert np.any(want != P.dinv * r)
        for r_off, z_off in OFFSETS:
            z = P.apply(r, symmetric, r_off, z_off)
            assert np.array_equal(z, want), (shape, scaled, symmetric, rhs,
                                             r_off, z_off)


@pytest.mark.parametrize("symmetric", STORAGE)
def test_apply_on_the_ragged_matrix(problems, symmetric):
    """many colours, colours of a single row, rows on the long-row path in
    both directions, a row without off-diagonal entries"""
    P = problems[("ragged3001", False)]
    M, S = P.M[symmetric], P.sweeps[symmetric]
    lens = np.diff(P.csr[0])
    print("ragged: colours", M.num_colors(), "row lengths", lens.min(),
          lens.max(), "plan bytes", M.plan_bytes())
    assert P.N == 3001 and lens.min() == 1 and np.sum(lens > 400) == 2
    assert M.num_colors() > 8
    assert min(len(i) for i in S.rows_of) == 1
    # a part of more than 64 entries, forward and backward
    for part in (0, 1):
        assert max(len(slots) for slots in S.parts[part]) > 64
    for rhs in ("rand", "ones"):
        r = P.rhs[rhs]
        want = P.precond(r, symmetric)
        for r_off, z_off in OFFSETS:
            z = P.apply(r, symmetric, r_off, z_off)
            assert np.array_equal(z, want), (symmetric, rhs, r_off, z_off)


@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("name", ["diag200", "diag1"])
def test_apply_on_a_diagonal_matrix(problems, name, symmetric):
    P = problems[(name, False)]
    assert P.M[symmetric].num_colors() == 1
    r = np.random.default_rng(5).uniform(-1, 1, P.N)
    for r_off, z_off in OFFSETS:
        z = P.apply(r, symmetric, r_off, z_off)
        assert np.array_equal(z, r * P.dinv), (name, symmetric, r_off, z_off)


def test_apply_errors(problems):
    P = problems[("poisson11", True)]
    e = P.exec_
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.sgs_apply(e, P.M[False], P.d_x, P.d_x)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.sgs_apply(e, P.M[False], P.d_x, P.d_x + 8 * (P.N - 1))


@pytest.mark.parametrize("world", [2, 3])
def test_apply_on_slab_ranks(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking (one block with ghost columns) and an overlapping
    halo model: bit for bit the restatement on the rank's own diagonal block."""
    from thread_world import ThreadWorld
    (rp, ci, va), diag = tp._slab_inputs(8)
    N = len(rp) - 1
    r_glob = oracle.csr_spmv(rp, ci, va,
                             np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        local = (np.asarray(lrp), np.asarray(lci), np.asarray(lva))
        r, dinv = r_glob[r0:r1], 1.0 / diag[r0:r1]
        d_r = exec_.alloc(M + 1)
        d_z = exec_.alloc(M + 2 * GUARD)
        for sym in (False, True):
            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                pre = host.SgsPreconditioner(exec_, A)
                colours = pre.colors()
                assert np.array_equal(
                    colours, host.sgs_color(lrp, lci, M, M, sym)[0])
                want = Sweeps(local, M, colours, sym).apply(dinv, r)
                for r_off, z_off in ((0, GUARD), (1, GUARD + 1)):
                    exec_.copy_from_host(d_r + 8 * r_off, r)
                    exec_.copy_from_host(d_z, np.full(M + 2 * GUARD, SENTINEL))
                    host.sgs_apply(exec_, pre, d_r + 8 * r_off, d_z + 8 * z_off)
                    buf = exec_.copy_to_host(d_z, M + 2 * GUARD)
                    what = (world, rank, sym, cm, r_off)
                    assert np.all(buf[:z_off] == SENTINEL), what
                    assert np.all(buf[z_off + M:] == SENTINEL), what
                    assert np.array_equal(buf[z_off:z_off + M], want), what
                pre.close()
                A.close()
        exec_.free(d_r), exec_.free(d_z)

    tw.run(rank_body, gpu=True)


# ---- 2. pcg_sgs against the reference -----------------------------------------------
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_reference(comm, problems, nt, shape, scaled,  # noqa: F811
                               symmetric, rhs):
    P = problems[(shape, scaled)]
    ref = P.ref(rhs)
    k, hist, x = P.solve(comm, rhs, symmetric=symmetric)
    assert k < KMAX
    tc._vs_ref(k, hist, x, ref, P.norm_a, (shape, scaled, symmetric, rhs))


def test_against_the_reference_on_the_ragged_matrix(comm, problems):  # noqa: F811
    P = problems[("ragged3001", False)]
    for symmetric in (False, True):
        k, hist, x = P.solve(comm, "rand", symmetric=symmetric)
        assert k < KMAX
        tc._vs_ref(k, hist, x, P.ref("rand"), P.norm_a, ("ragged", symmetric))


# ---- 3. what it is for ----------------------------------------------------------------
@pytest.mark.parametrize("scaled", MATS)
def test_fewer_iterations_than_jacobi(comm, problems, scaled):  # noqa: F811
    """The two references on the CPU: poisson24 plain 50 iterations against
    100 of Jacobi-PCG, scaled 50 against 99."""
    P = problems[("poisson24", scaled)]
    _, k_jacobi, _ = tp._pcg_ref(P.spmv, oracle.ddot, P.rhs["rand"], P.dinv,
                                 KMAX, RTOL)
    k, _, _ = P.solve(comm, "rand")
    print("poisson24", scaled, "k pcg_sgs", k, "k_ref pcg_sgs",
          P.ref("rand").k, "k_ref jacobi", k_jacobi)
    assert P.ref("rand").k < k_jacobi
    assert k < k_jacobi


# ---- 4. pcg_chebyshev's remaining cases ------------------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape,  # noqa: F811
                                    symmetric):
    P = problems[(shape, True)]
    for kmax in (0, 1, 2, 7):
        k, hist, x = P.solve(comm, "ones", kmax=kmax, rtol=0.0,
                             symmetric=symmetric)
        what = (shape, symmetric, kmax)
        assert k == kmax, what
        assert hist.shape == (kmax + 1,) and np.all(hist > 0.0), what
        assert np.any(x != 0.0) == (kmax > 0), what
        ref = P.ref("ones", kmax, 0.0)
        assert np.allclose(hist, ref.hist, rtol=1e-6, atol=0.0), what
        # b = 0: stopped at k = 0 with x = 0, nothing undefined
        k, hist, x = P.solve(comm, "zero", kmax=kmax, rtol=0.0,
                             symmetric=symmetric)
        assert k == 0 and np.all(x == 0.0), what
        assert hist.shape == (1,) and hist[0] == 0.0, what


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_after_convergence(comm, problems, nt, shape):  # noqa: F811
    """poll_every = 255 and kmax far beyond the stop: every iteration is
    enqueued, so every kernel launched after `done` had the chance to touch x;
    poll_every = 1: the host stops enqueuing early."""
    P = problems[(shape, True)]
    k, hist, x = P.solve(comm, "rand")
    assert 1 < k and k + 80 < 255
    for poll in (255, 1):
        got = P.solve(comm, "rand", kmax=k + 80, poll_every=poll)
        _same((k, hist, x), got, (shape, poll))
    got = P.solve(comm, "rand", kmax=k)
    _same((k, hist, x), got, (shape, "kmax = k"))


def test_workspace_reused_and_grown(comm, problems, nt):  # noqa: F811
    """One workspace across shapes (small, large, middle) and a smaller kmax:
    every result equals the one on a fresh workspace, bit for bit."""
    e = problems[("poisson11", True)].exec_
    shared = host.SgsWorkspace(e)
    plan = [("poisson11", 30, GUARD), ("poisson24", 40, GUARD + 1),
            ("banded4097", 12, GUARD), ("poisson24", 7, GUARD),
            ("poisson11", 40, GUARD + 1), ("poisson11", 0, GUARD)]
    for shape, kmax, x_off in plan:
        P = problems[(shape, True)]
        fresh = host.SgsWorkspace(e)
        want = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=fresh, x_off=x_off)
        fresh.close()
        got = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=shared, x_off=x_off)
        _same(want, got, (shape, kmax, x_off))
    shared.close()


def test_unaligned_x_keeps_the_bits(comm, problems, nt):  # noqa: F811
    for shape in SHAPES:
        P = problems[(shape, True)]
        want = P.solve(comm, "rand", kmax=25)
        assert want[0] > 1
        got = P.solve(comm, "rand", kmax=25, x_off=GUARD + 1)
        _same(want, got, (shape, "unaligned x"))
        # without a workspace of the caller's
        e = P.exec_
        e.copy_from_host(P.d_b, P.rhs["rand"])
        k, hist = host.pcg_sgs(comm, e, P.A[False], P.M[False], P.d_b,
                               P._guarded(GUARD), 25, RTOL)
        _same(want, (k, hist, P._read_guarded(GUARD)), (shape, "no workspace"))


def test_time_spmv_counts_one_spmv_per_iteration(comm, problems):  # noqa: F811
    P = problems[("poisson11", True)]
    stats = {}
    k, _, _ = P.solve(comm, "rand", kmax=5, rtol=0.0, time_spmv=True,
                      stats=stats)
    assert k == 5
    assert stats["spmv_launches"] == 5 and stats["spmv_ms_total"] > 0.0


def test_errors_leave_the_executor_as_it_was(comm, problems):  # noqa: F811
    P = problems[("poisson11", True)]
    e, A, M, N = P.exec_, P.A[False], P.M[False], P.N
    other = problems[("banded4097", True)].M[False]
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)
    try:
        e.copy_from_host(P.d_b, P.rhs["ones"])
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg_sgs(comm, e, A, M, P.d_b, P.d_b, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg_sgs(comm, e, A, M, P.d_b, P.d_b + 8 * (N - 1), 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.pcg_sgs(comm, e, A, M, P.d_b, P.d_x, -1, 1e-10)
        with pytest.raises(host.SpmvHostError, match="rows"):
            host.pcg_sgs(comm, e, A, other, P.d_b, P.d_x, 5, 1e-10)
        assert tp._current_stream(e) == mine.value
        # ... and after a solve that went through
        k, _ = host.pcg_sgs(comm, e, A, M, P.d_b, P.d_x, 3, 0.0, P.ws)
        assert k == 3
        assert tp._current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


# ---- 5. the constructor -------------------------------------------------------------------
def test_a_diagonal_that_is_not_positive_is_refused(exec_, comm):  # noqa: F811
    rp, ci, va = tp._csr("poisson11")
    N = len(rp) - 1
    on = np.flatnonzero(ci == tp._row_of(rp))
    for what, e, value in (("zero", 17, 0.0), ("negative", N - 2, -6.0),
                           ("nan", 5, np.nan)):
        bad = va.copy()
        bad[on[e]] = value
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, rp, ci, bad, N, N, [], [],
                                          sym, host.P2P_NONBLOCKING)
            with pytest.raises(host.SpmvHostError,
                               match="diagonal is not positive"):
                host.SgsPreconditioner(exec_, A)
            A.close()


def test_release_csr_after_the_setup_not_before(comm):  # noqa: F811
    """A preconditioner built before release_csr() owns its copy and applies
    with the same bits afterwards; on a released matrix the constructor throws,
    for both storages."""
    e = host.HipExecutor(0)
    # the sliced jagged forms keep the matrix in the plan: the CSR arrays can go
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    N = len(csr[0]) - 1
    dinv = 1.0 / tp._diag_of(csr)
    r = oracle.gaussian_x_fast(N)
    d_r, d_z = e.alloc(N), e.alloc(N)
    e.copy_from_host(d_r, r)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        print("symmetric", sym, "sjds", A.plan_get("sjds"), "sym_sj",
              A.plan_get("sym_sj"), "long rows", A.plan_get("sj_long_rows"))
        M = host.SgsPreconditioner(e, A)
        want = Sweeps(csr, N, M.colors(), sym).apply(dinv, r)
        host.sgs_apply(e, M, d_r, d_z)
        assert np.array_equal(e.copy_to_host(d_z, N), want), sym
        assert A.release_csr() > 0
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.sgs_apply(e, M, d_r, d_z)
        assert np.array_equal(e.copy_to_host(d_z, N), want), (sym, "released")
        with pytest.raises(host.SpmvHostError, match="released"):
            host.SgsPreconditioner(e, A)
        M.close()
        A.close()
    e.free(d_r), e.free(d_z)
    e.synchronize()
    e.close()


# ---- 6. several ranks -------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_pcg_sgs(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking and an overlapping halo model, ONE workspace per rank
    over all solves; against the reference on oracle.dist_spmv with the
    block-diagonal preconditioner and the rank-ordered sum."""
    from thread_world import ThreadWorld
    (rp, ci, va), diag = tp._slab_inputs(8)
    N = len(rp) - 1
    norm_a = tp._norm_inf((rp, ci, va))
    rng = np.random.default_rng(world)
    bs = [oracle.csr_spmv(rp, ci, va, np.ones(N)),
          oracle.csr_spmv(rp, ci, va, rng.uniform(-1, 1, N))]
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]

    def dist_dot(dot):
        def f(a, b):
            s = 0.0
            for r in range(world):
                s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
            return s
        return f

    refs = {}
    for sym in (False, True):
        sweeps = []
        for r in range(world):
            lrp, lci, lva, _ = blocks[r]
            M = int(ranges[r + 1] - ranges[r])
            colours, _ = host.sgs_color(lrp, lci, M, M, sym)
            sweeps.append(Sweeps((np.asarray(lrp), np.asarray(lci),
                                  np.asarray(lva)), M, colours, sym))

        def precond(v, sweeps=sweeps):
            return np.concatenate([
                sweeps[r].apply(1.0 / diag[ranges[r]:ranges[r + 1]],
                                v[ranges[r]:ranges[r + 1]])
                for r in range(world)])

        for cm in models:
            def spmv(p, sym=sym, cm=cm):
                return oracle.dist_spmv(world, rp, ci, va, p, sym, cm)
            refs[(sym, cm)] = [_Ref(spmv, dist_dot(oracle.ddot),
                                    dist_dot(_dot_chunked), b, precond)
                               for b in bs]
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        ws = host.SgsWorkspace(exec_)
        d_b = exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for (sym, cm), ref in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, cm)
            pre = host.SgsPreconditioner(exec_, A)
            for j, rf in enumerate(ref):
                exec_.copy_from_host(d_b, bs[j][r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist = host.pcg_sgs(comm, exec_, A, pre, d_b, d_x + 8 * GUARD,
                                       KMAX, RTOL, ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k]))
                assert np.all(ks == k), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX
                tc._vs_ref(k, hist, xs, rf, norm_a, (world, sym, cm, j))
            pre.close()
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
