"""The multicolour ILU(0) preconditioner factored on the device:
spmv::Ilu0Preconditioner, refactor, ilu0_apply, and pcg_sgs / gmres with it.

The factorisation has no reductions: every entry receives its subtractions in
ascending pos(k) whichever lane performs them, so factor() is compared with
np.array_equal against the numpy restatement of ilu0_cases.py, driven by the
colours read back from the object; ilu0_apply likewise against the
restatement's sweeps (position order).

Matrices: Poisson 11^3 (1 331 rows, odd, two colours), test_gpu_pcg's banded
matrix of 4 097 rows, gmres_cases.convdiff(8) (nonsymmetric), test_gpu_sgs's
ragged matrix (imported, not copied: 3 001 rows, 24 colours and more, hub rows
of about 500 entries -- the global-memory path of the factor kernel and the
long-row path of the sweeps --, a row without off-diagonal entries), the arrow
matrix of 130 rows (a hub row of 129 entries before it: the LDS path at more
than 64 entries), a diagonal matrix and n = 1; each plain and scaled S A S, the
symmetric ones in both storages.

Solves: pcg_sgs against test_gpu_chebyshev._pcg_ref with the restatement as
preconditioner through test_gpu_chebyshev._vs_ref unchanged (bars: see
test_gpu_sgs.py); gmres(30) against gmres_cases.gmres_ref through
test_gpu_gmres._vs_ref unchanged.  On the CPU the largest dev_ref of the cases
below is printed by every test; on the arrow matrix M = A up to rounding and the
restatement's k is 1, which the GPU must return exactly.

X and z sit between guard words and are filled with a sentinel before every
call."""
import ctypes as C

import numpy as np
import pytest

import gmres_cases as gc
import ilu0_cases as ic
import oracle
import sgs_layout
import test_gpu_chebyshev as tc
import test_gpu_gmres as tg
import test_gpu_pcg as tp
import test_gpu_sgs as ts
from spmv_amd import _lib, host
from test_gpu_bicgstab import _dot_chunked
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

_McgsPart, _McgsHost = sgs_layout._McgsPart, sgs_layout._McgsHost
_Ilu0Part, _Ilu0Host = sgs_layout._Ilu0Part, sgs_layout._Ilu0Host
_sliced = sgs_layout._sliced

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = tp.KMAX, tp.RTOL
OFFSETS = ((0, GUARD), (1, GUARD + 1))


def _make_csr(name):
    if name == "arrow130":
        return ic.arrow(130)
    if name == "convdiff8":
        return gc.convdiff(8)
    return ts._make_csr(name)


SYMMETRIC = ("poisson11", "banded4097", "ragged3001", "diag200", "diag1")
NAMES = SYMMETRIC + ("convdiff8", "arrow130")


class _Problem:
    """One matrix in its storages with its preconditioners, the restatement's
    factor, right-hand sides, buffers and references (computed once)."""

    def __init__(self, exec_, comm, name, scaled):  # noqa: F811
        self.name, self.exec_ = (name, "scaled" if scaled else "plain"), exec_
        csr = _make_csr(name)
        self.csr = tp._scaled(csr) if scaled else csr
        self.N = N = len(self.csr[0]) - 1
        self.norm_a = tp._norm_inf(self.csr)
        rng = np.random.default_rng(N + 1)
        self.rhs = {"ones": self.spmv(np.ones(N)),
                    "rand": self.spmv(rng.uniform(-1, 1, N)),
                    "zero": np.zeros(N)}
        self.storages = (False, True) if name in SYMMETRIC else (False,)
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in self.storages}
        self.M = {sym: host.Ilu0Preconditioner(exec_, A)
                  for sym, A in self.A.items()}
        colours = self.M[False].colors()
        for M in self.M.values():
            assert M.rows() == N and np.array_equal(M.colors(), colours)
            assert M.negative_pivots() == 0
        self.ref = ic.Ilu0Ref(self.csr, N, colours, False)
        self.fac = self.ref.factor()
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.SgsWorkspace(exec_)
        self.gws = host.GmresWorkspace(exec_)
        self._refs = {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, v)

    def precond(self, r):
        return self.ref.apply(self.fac, r)

    def pcg_ref(self, rhs, kmax=KMAX, rtol=RTOL):
        key = ("pcg", rhs, kmax, rtol)
        if key not in self._refs:
            self._refs[key] = ts._Ref(self.spmv, oracle.ddot, _dot_chunked,
                                      self.rhs[rhs], self.precond, kmax, rtol)
        return self._refs[key]

    def gmres_ref(self, rhs, m, kmax=tg.KMAX, rtol=tg.RTOL):
        key = ("gmres", rhs, m, kmax, rtol)
        if key not in self._refs:
            self._refs[key] = tg._Ref(self.spmv, self.precond, self.rhs[rhs], m,
                                      kmax=kmax, rtol=rtol)
        return self._refs[key]

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
        e = self.exec_
        e.copy_from_host(self.d_b + 8 * r_off, r)
        d_z = self._guarded(z_off)
        host.ilu0_apply(e, M or self.M[symmetric], self.d_b + 8 * r_off, d_z)
        return self._read_guarded(z_off)

    def pcg(self, comm, rhs, kmax=KMAX, rtol=RTOL, symmetric=False,  # noqa: F811
            x_off=GUARD):
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist = host.pcg_sgs(comm, e, self.A[symmetric], self.M[symmetric],
                               self.d_b, d_x, kmax, rtol, self.ws)
        x = self._read_guarded(x_off)
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x

    def gmres(self, comm, rhs, m, kmax=tg.KMAX, rtol=tg.RTOL,  # noqa: F811
              x_off=GUARD):
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist, status = host.gmres(comm, e, self.A[False], self.d_b, d_x, m,
                                     kmax, rtol, sgs=self.M[False], ws=self.gws)
        x = self._read_guarded(x_off)
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x, status

    def close(self):
        self.ws.close()
        self.gws.close()
        for M in self.M.values():
            M.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_b, self.d_x):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    ps = {}

    def get(name, scaled):
        if (name, scaled) not in ps:
            ps[(name, scaled)] = _Problem(exec_, comm, name, scaled)
        return ps[(name, scaled)]
    yield get
    for p in ps.values():
        p.close()


MATS = [pytest.param(False, id="plain"), pytest.param(True, id="scaled")]


def _same_factor(got, want, what):
    for g, w, part in zip(got, want, ("l", "u", "d")):
        assert g.shape == w.shape, (what, part)
        assert np.array_equal(g, w), (what, part, int(np.sum(g != w)), len(g))


# ---- 1. the factor, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", NAMES)
def test_factor_is_exact(problems, name, scaled):
    P = problems(name, scaled)
    ref = P.ref
    lens = [np.diff(part["ptr"]) for part in ref.parts]
    print(name, scaled, "colours", P.M[False].num_colors(), "longest before",
          lens[0].max(initial=0), "longest after", lens[1].max(initial=0),
          "plan bytes", P.M[False].plan_bytes())
    if name == "poisson11":
        assert P.M[False].num_colors() == 2
    if name == "ragged3001":
        assert P.M[False].num_colors() >= 24
        # longer than the LDS slab of 256 entries, and more than 64 in a part
        assert (lens[0] + lens[1] + 1).max() > 256
        assert lens[0].max() > 64 and lens[1].max() > 64
        assert (lens[0] + lens[1]).min() == 0
    if name == "arrow130":
        assert P.M[False].num_colors() == 2 and lens[0].max() == 129
    if name in ("poisson11", "banded4097", "convdiff8", "ragged3001"):
        # the factor is not the matrix: some pivot has changed
        assert np.any(P.fac[2] != ref.diag[ref.perm])
    for sym, M in P.M.items():
        assert M.plan_bytes() >= 28 * P.N
        (bptr, bcol), (aptr, acol) = M.pattern()
        for got, want in (((bptr, bcol), ref.parts[0]), ((aptr, acol), ref.parts[1])):
            assert np.array_equal(got[0], want["ptr"]), (name, sym)
            assert np.array_equal(got[1], want["col"]), (name, sym)
        _same_factor(M.factor(), P.fac, (name, scaled, sym))
    if len(P.M) == 2:  # both storages: identical factors
        _same_factor(P.M[True].factor(), P.M[False].factor(), (name, "storages"))


# ---- 2. the application, bit for bit ----------------------------------------------------
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", NAMES)
def test_apply_is_exact(problems, name, scaled):
    P = problems(name, scaled)
    for rhs in ("rand", "ones"):
        r = P.rhs[rhs]
        want = P.precond(r)
        for sym in P.storages:
            for r_off, z_off in OFFSETS:
                z = P.apply(r, sym, r_off, z_off)
                assert np.array_equal(z, want), (name, scaled, sym, rhs, r_off)
    e = P.exec_
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.ilu0_apply(e, P.M[False], P.d_x, P.d_x)


@pytest.mark.parametrize("world", [2, 3])
def test_apply_on_slab_ranks(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking (one block with ghost columns) and an overlapping halo
    model: the factor and the application of the rank's own diagonal block."""
    from thread_world import ThreadWorld
    (rp, ci, va), _ = tp._slab_inputs(8)
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
        r = r_glob[r0:r1]
        d_r = exec_.alloc(M + 1)
        d_z = exec_.alloc(M + 2 * GUARD)
        for sym in (False, True):
            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                pre = host.Ilu0Preconditioner(exec_, A)
                ref = ic.Ilu0Ref(local, M, pre.colors(), False)
                fac = ref.factor()
                what = (world, rank, sym, cm)
                _same_factor(pre.factor(), fac, what)
                want = ref.apply(fac, r)
                for r_off, z_off in OFFSETS:
                    exec_.copy_from_host(d_r + 8 * r_off, r)
                    exec_.copy_from_host(d_z, np.full(M + 2 * GUARD, SENTINEL))
                    host.ilu0_apply(exec_, pre, d_r + 8 * r_off, d_z + 8 * z_off)
                    buf = exec_.copy_to_host(d_z, M + 2 * GUARD)
                    assert np.all(buf[:z_off] == SENTINEL), what
                    assert np.all(buf[z_off + M:] == SENTINEL), what
                    assert np.array_equal(buf[z_off:z_off + M], want), what
                pre.close()
                A.close()
        exec_.free(d_r), exec_.free(d_z)

    tw.run(rank_body, gpu=True)


# ---- 3. refactor -------------------------------------------------------------------------
def _changed(csr):
    """2 A, perturbed entry by entry, symmetric where A is"""
    rp, ci, va = csr
    rows = tp._row_of(rp)[:len(ci)]
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)
    return rp, ci, 2.0 * va * (1.0 + 0.05 * np.sin(3.0 * lo + 7.0 * hi))


def _write_values(exec_, A, csr, symmetric):  # noqa: F811
    """the matrix's coefficients rewritten in place on the device"""
    rp, ci, va = csr
    rows = tp._row_of(rp)[:len(ci)]
    values, diagonal = A.local_values()
    nnz = A.blocks()["local"][2]
    if symmetric:
        assert nnz == np.sum(ci < rows) and diagonal
        exec_.copy_from_host(values, va[ci < rows])
        exec_.copy_from_host(diagonal, va[ci == rows])
    else:
        assert nnz == len(va) and not diagonal
        exec_.copy_from_host(values, va)


@pytest.mark.parametrize("name", ["poisson11", "ragged3001", "convdiff8"])
def test_refactor_equals_a_fresh_object(exec_, comm, name):  # noqa: F811
    csr = tp._scaled(_make_csr(name))
    new = _changed(csr)
    N = len(csr[0]) - 1
    for sym in ((False, True) if name in SYMMETRIC else (False,)):
        A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        M = host.Ilu0Preconditioner(exec_, A)
        old = M.factor()
        # the arrays are where and how this test believes them to be
        values, _ = A.local_values()
        rows = tp._row_of(csr[0])[:len(csr[1])]
        keep = (csr[1] < rows) if sym else np.ones(len(rows), bool)
        assert np.array_equal(exec_.copy_to_host(values, int(keep.sum())),
                              csr[2][keep])
        _write_values(exec_, A, new, sym)
        M.refactor(A)
        A2 = host.Matrix.create_matrix(comm, exec_, *new, N, N, [], [], sym,
                                       host.P2P_NONBLOCKING)
        fresh = host.Ilu0Preconditioner(exec_, A2)
        got = M.factor()
        _same_factor(got, fresh.factor(), (name, sym, "refactor"))
        ref = ic.Ilu0Ref(new, N, M.colors(), False)
        _same_factor(got, ref.factor(), (name, sym, "restatement"))
        assert np.any(got[2] != old[2]) and np.any(got[2] != 2.0 * old[2])
        # ... and the sweeps run on the new factor
        r = np.random.default_rng(3).uniform(-1, 1, N)
        d_r, d_z = exec_.alloc(N), exec_.alloc(N)
        exec_.copy_from_host(d_r, r)
        host.ilu0_apply(exec_, M, d_r, d_z)
        assert np.array_equal(exec_.copy_to_host(d_z, N), ref.apply(got, r))
        exec_.free(d_r), exec_.free(d_z)
        other = host.Matrix.create_matrix(comm, exec_, *_make_csr("diag200"), 200,
                                          200, [], [], sym, host.P2P_NONBLOCKING)
        with pytest.raises(host.SpmvHostError, match="pattern"):
            M.refactor(other)
        for obj in (other, fresh, A2, M, A):
            obj.close()


def test_refactor_after_plan_values_changed_on_a_baked_plan(comm):  # noqa: F811
    """The SpMV plan keeps its own copy of the values (sliced jagged form,
    forced by sj_min_nnz = 0).  Coefficients rewritten in place: before
    plan_values_changed mult does not return the new product; after it and a
    refactor, matrix and preconditioner are those of a fresh pair -- factor,
    product and one whole pcg_sgs solve, bit for bit."""
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    new = _changed(csr)
    N = len(csr[0]) - 1
    v = oracle.gaussian_x_fast(N)
    d_v, d_y, d_x = e.alloc(N), e.alloc(N), e.alloc(N)
    e.copy_from_host(d_v, v)
    ws = host.SgsWorkspace(e)

    def product(A):
        e.copy_from_host(d_y, np.full(N, SENTINEL))
        A.mult(d_v, d_y)
        return e.copy_to_host(d_y, N)

    def solve(A, M):
        e.copy_from_host(d_x, np.full(N, SENTINEL))
        k, hist = host.pcg_sgs(comm, e, A, M, d_y, d_x, KMAX, RTOL, ws)
        return k, hist.copy(), e.copy_to_host(d_x, N)

    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        print("symmetric", sym, "sjds", A.plan_get("sjds"), "sym_sj",
              A.plan_get("sym_sj"))
        M = host.Ilu0Preconditioner(e, A)
        old_product = product(A)
        _write_values(e, A, new, sym)
        A2 = host.Matrix.create_matrix(comm, e, *new, N, N, [], [], sym,
                                       host.P2P_BLOCKING)
        M2 = host.Ilu0Preconditioner(e, A2)
        want = product(A2)
        assert np.any(want != old_product)
        # a baked plan IS involved: with the arrays rewritten and nothing else
        # done, mult does not return the new matrix's product (the general
        # sliced jagged form returns the old one; the symmetric one reads part
        # of the matrix from the caller's arrays and returns a mixture)
        stale = product(A)
        assert not np.array_equal(stale, want), (sym, "no stale copy")
        if not sym:
            assert np.array_equal(stale, old_product), (sym, "stale copy")
        A.plan_values_changed()
        M.refactor(A)
        assert np.array_equal(product(A), want), (sym, "product")
        _same_factor(M.factor(), M2.factor(), (sym, "values_changed"))
        # d_y holds A v: the right-hand side of one solve with each pair
        got, fresh = solve(A, M), solve(A2, M2)
        assert got[0] == fresh[0] and 1 < got[0] < KMAX, (sym, got[0], fresh[0])
        assert np.array_equal(got[1], fresh[1]), (sym, "history")
        assert np.array_equal(got[2], fresh[2]), (sym, "x")
        # after release_csr there is nothing to rewrite
        assert A.release_csr() > 0
        with pytest.raises(host.SpmvHostError, match="released"):
            A.plan_values_changed()
        with pytest.raises(host.SpmvHostError, match="released"):
            A.local_values()
        for obj in (M2, A2, M, A):
            obj.close()
    ws.close()
    for q in (d_v, d_y, d_x):
        e.free(q)
    e.synchronize()
    e.close()


def test_release_csr_after_the_setup_not_before(comm):  # noqa: F811
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    N = len(csr[0]) - 1
    r = oracle.gaussian_x_fast(N)
    d_r, d_z = e.alloc(N), e.alloc(N)
    e.copy_from_host(d_r, r)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        M = host.Ilu0Preconditioner(e, A)
        ref = ic.Ilu0Ref(csr, N, M.colors(), False)
        want = ref.apply(ref.factor(), r)
        host.ilu0_apply(e, M, d_r, d_z)
        assert np.array_equal(e.copy_to_host(d_z, N), want), sym
        assert A.release_csr() > 0
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.ilu0_apply(e, M, d_r, d_z)
        assert np.array_equal(e.copy_to_host(d_z, N), want), (sym, "released")
        with pytest.raises(host.SpmvHostError, match="released"):
            M.refactor(A)
        with pytest.raises(host.SpmvHostError, match="released"):
            host.Ilu0Preconditioner(e, A)
        # the failed calls left the factor alone
        host.ilu0_apply(e, M, d_r, d_z)
        assert np.array_equal(e.copy_to_host(d_z, N), want), (sym, "after")
        M.close()
        A.close()
    e.free(d_r), e.free(d_z)
    e.synchronize()
    e.close()


# ---- 4. pivots ------------------------------------------------------------------------------
def test_pivots(exec_, comm):  # noqa: F811
    """2 x 2 blocks [[a, 1], [1, b]]: the second pivot is b - 1 / a."""
    n = 64
    i = np.arange(n // 2)
    rows = np.concatenate([2 * i, 2 * i + 1, 2 * i, 2 * i + 1])
    cols = np.concatenate([2 * i, 2 * i + 1, 2 * i + 1, 2 * i])
    order = np.lexsort((cols, rows))
    rp = np.arange(0, 2 * n + 1, 2).astype(np.int32)
    ci = cols[order].astype(np.int32)

    def values(a, b):
        half = np.ones(n // 2)  # entries: (2i, 2i), (2i+1, 2i+1), then the ones
        return np.concatenate([a * half, b * half, np.ones(n)])[order]

    good = values(2.0, 3.0)
    a = np.full(n // 2, 2.0)
    b_zero = np.full(n // 2, 3.0)
    b_zero[5] = 0.5  # 0.5 - 1 / 2 == 0
    b_neg = np.full(n // 2, 3.0)
    b_neg[[3, 9]] = 0.25  # 0.25 - 0.5 < 0: symmetric indefinite
    d_b, d_x = exec_.alloc(n), exec_.alloc(n)
    exec_.copy_from_host(d_b, np.ones(n))
    for sym in (False, True):
        def matrix(va):
            return host.Matrix.create_matrix(comm, exec_, rp, ci, va, n, n, [],
                                             [], sym, host.P2P_NONBLOCKING)
        A_zero, A_neg, A_good = (matrix(values(a, b_zero)),
                                 matrix(values(a, b_neg)), matrix(good))
        with pytest.raises(host.SpmvHostError, match="pivot"):
            host.Ilu0Preconditioner(exec_, A_zero)
        M = host.Ilu0Preconditioner(exec_, A_neg)
        assert M.negative_pivots() == 2
        with pytest.raises(host.SpmvHostError, match="pivot"):
            host.pcg_sgs(comm, exec_, A_neg, M, d_b, d_x, 10, 1e-10)
        k, hist, status = host.gmres(comm, exec_, A_neg, d_b, d_x, 30, 50, 1e-10,
                                     sgs=M)
        # M = A: one step solves it, the lucky breakdown (status 1) included
        assert status in (0, 1) and k <= 2 and hist[k] / hist[0] < 1e-10
        # a refactor that meets a zero pivot: not usable until one succeeds
        with pytest.raises(host.SpmvHostError, match="pivot"):
            M.refactor(A_zero)
        with pytest.raises(host.SpmvHostError, match="pivot"):
            host.ilu0_apply(exec_, M, d_b, d_x)
        with pytest.raises(host.SpmvHostError, match="pivot"):
            host.gmres(comm, exec_, A_neg, d_b, d_x, 30, 50, 1e-10, sgs=M)
        M.refactor(A_good)
        assert M.negative_pivots() == 0
        k, hist = host.pcg_sgs(comm, exec_, A_good, M, d_b, d_x, 10, 1e-10)
        assert k <= 2 and hist[k] / hist[0] < 1e-10
        for obj in (M, A_zero, A_neg, A_good):
            obj.close()
    exec_.free(d_b), exec_.free(d_x)


# ---- 5. solves --------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", ["poisson11", "banded4097", "ragged3001"])
def test_pcg_against_the_reference(comm, problems, name, scaled):  # noqa: F811
    P = problems(name, scaled)
    ref = P.pcg_ref("rand")
    for sym in P.storages:
        k, hist, x = P.pcg(comm, "rand", symmetric=sym)
        assert k < KMAX
        tc._vs_ref(k, hist, x, ref, P.norm_a, (name, scaled, sym))


@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", ["convdiff8", "arrow130"])
def test_gmres_against_the_reference(comm, problems, name, scaled):  # noqa: F811
    P = problems(name, scaled)
    ref = P.gmres_ref("rand", 30)
    k, hist, x, status = P.gmres(comm, "rand", 30)
    tg._vs_ref(k, hist, x, status, ref, P.spmv, (name, scaled))
    if name == "arrow130":  # no fill is dropped: M = A
        print("arrow130: k of the restatement", ref.k)
        assert ref.k == 1 and k == ref.k


def test_fixed_number_of_iterations_and_a_zero_right_hand_side(
        comm, problems):  # noqa: F811
    P = problems("poisson11", True)
    for kmax in (0, 1, 5):
        ref = P.pcg_ref("ones", kmax, 0.0)
        for sym in P.storages:
            k, hist, x = P.pcg(comm, "ones", kmax=kmax, rtol=0.0, symmetric=sym)
            assert k == kmax and hist.shape == (kmax + 1,)
            assert np.allclose(hist, ref.hist, rtol=1e-6, atol=0.0), (sym, kmax)
            k, hist, x = P.pcg(comm, "zero", kmax=kmax, rtol=0.0, symmetric=sym)
            assert k == 0 and np.all(x == 0.0) and hist[0] == 0.0
    Q = problems("convdiff8", True)
    for kmax in (0, 3):
        ref = Q.gmres_ref("ones", 30, kmax, 0.0)
        k, hist, x, status = Q.gmres(comm, "ones", 30, kmax=kmax, rtol=0.0)
        assert k == kmax and status == 0
        assert np.allclose(hist, ref.hist, rtol=1e-6, atol=0.0), kmax
        k, hist, x, status = Q.gmres(comm, "zero", 30, kmax=kmax, rtol=0.0)
        assert k == 0 and np.all(x == 0.0) and hist[0] == 0.0


@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_solves(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs: pcg_sgs
    (both storages) and gmres(30) with the block-Jacobi ILU(0); the same k and
    status on every rank, against the references on oracle.dist_spmv with the
    rank-ordered sum."""
    from thread_world import ThreadWorld
    (rp, ci, va), _ = tp._slab_inputs(8)
    N = len(rp) - 1
    norm_a = tp._norm_inf((rp, ci, va))
    b = oracle.csr_spmv(rp, ci, va,
                        np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]

    def dist_dot(dot):
        def f(u, v):
            s = 0.0
            for r in range(world):
                s += dot(u[ranges[r]:ranges[r + 1]], v[ranges[r]:ranges[r + 1]])
            return s
        return f

    refs, facs = [], []
    for r in range(world):
        lrp, lci, lva, _ = blocks[r]
        M = int(ranges[r + 1] - ranges[r])
        local = (np.asarray(lrp), np.asarray(lci), np.asarray(lva))
        refs.append(ic.Ilu0Ref(local, M, ic.greedy_colours(local, M), False))
        facs.append(refs[r].factor())

    def precond(v):
        return np.concatenate([refs[r].apply(facs[r], v[ranges[r]:ranges[r + 1]])
                               for r in range(world)])

    cm = host.P2P_NONBLOCKING

    def spmv(p):
        return oracle.dist_spmv(world, rp, ci, va, p, False, cm)
    pcg_ref = ts._Ref(spmv, dist_dot(oracle.ddot), dist_dot(_dot_chunked), b,
                      precond)
    x_g, k_g, hist_g, st_g = gc.gmres_ref(spmv, dist_dot(oracle.ddot), precond, b,
                                          30, tg.KMAX, tg.RTOL)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        ws, gws = host.SgsWorkspace(exec_), host.GmresWorkspace(exec_)
        d_b = exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        exec_.copy_from_host(d_b, b[r0:r1])
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, cm)
            pre = host.Ilu0Preconditioner(exec_, A)
            assert np.array_equal(pre.colors(), refs[rank].colours)
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
            tc._vs_ref(k, hist, xs, pcg_ref, norm_a, (world, sym))
            if not sym:
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.gmres(comm, exec_, A, d_b,
                                             d_x + 8 * GUARD, 30, tg.KMAX,
                                             tg.RTOL, sgs=pre, ws=gws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks == np.array([k, status] * world)), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                print(world, "gmres k", k, "k_ref", k_g)
                assert status == st_g == 0 and abs(k - k_g) <= 1
                assert np.linalg.norm(xs - x_g) <= 1e-8 * np.linalg.norm(x_g)
            pre.close()
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close(), gws.close()

    tw.run(rank_body, gpu=True)


# ---- 6. plan_create checks what a kernel will index with ------------------------------
def test_plan_create_refuses_every_bad_index(exec_):  # noqa: F811
    """spmv_hip_ilu0_plan_create through the C ABI on hand-built input: the
    sound input is taken, and each corrupted index a kernel would dereference
    -- colour relation and order of cpos, src, slot, row pointers, an empty
    colour -- is SPMV_HIP_EINVAL."""
    EINVAL = -1
    csr = gc.poisson(5)
    n, nnz = len(csr[0]) - 1, len(csr[2])
    sym = host.ilu0_symbolic(csr[0], csr[1], n)
    c1 = int(sym["color_start"][1])
    keep = []  # every array a struct points to stays alive

    def ptr_of(a):
        if a is None:
            return None
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def build(change=None):
        y = {k: (dict(v) if isinstance(v, dict) else v) for k, v in sym.items()}
        sl = {h: _sliced(sym, sym[h]) for h in ("before", "after")}
        num_values = nnz
        for h in ("before", "after"):
            for k in ("ptr", "cpos", "src", "slot"):
                y[h][k] = y[h][k].copy()
        if change:
            num_values = change(y, sl) or nnz
        s = _Ilu0Host()
        s.mcgs.num_rows, s.mcgs.num_colors = n, len(y["color_start"]) - 1
        s.mcgs.perm = ptr_of(np.ascontiguousarray(y["perm"], np.int32))
        s.mcgs.color_start = ptr_of(np.ascontiguousarray(y["color_start"],
                                                         np.int32))
        s.mcgs.dinv = ptr_of(np.zeros(n))
        for h in ("before", "after"):
            for k, a in sl[h].items():
                setattr(getattr(s.mcgs, h), k, ptr_of(a))
            for k in ("ptr", "cpos", "src", "slot"):
                setattr(getattr(s, h), k, ptr_of(y[h][k]))
        s.num_values = num_values
        keep.append(s)
        plan = C.c_void_p()
        rc = _lib.hip.spmv_hip_ilu0_plan_create(
            exec_.context, C.cast(C.pointer(s), C.c_void_p), C.byref(plan))
        if rc == 0:
            assert _lib.hip.spmv_hip_ilu0_plan_destroy(plan) == 0
        else:
            assert not plan.value
        return rc

    assert build() == 0
    row = int(np.flatnonzero(np.diff(sym["before"]["ptr"]) >= 2)[0])
    e0 = int(sym["before"]["ptr"][row])

    def set_(h, k, e, value):
        def change(y, sl):
            y[h][k][e] = value
        return change

    def swap(y, sl):
        c = y["before"]["cpos"]
        c[e0], c[e0 + 1] = c[e0 + 1], c[e0]

    def empty_colour(y, sl):
        y["color_start"] = np.array([0, c1, c1, n], np.int32)
        for h in sl:
            sl[h]["color_slice"] = np.array([0, 1, 1, 2], np.int32)
            sl[h]["color_long"] = np.zeros(4, np.int32)

    bad = {
        "before: column of the row's own colour": set_("before", "cpos", e0, c1),
        "before: negative position": set_("before", "cpos", e0, -1),
        "after: column of the row's own colour": set_("after", "cpos", 0, c1 - 1),
        "after: position beyond the rows": set_("after", "cpos", 0, n),
        "cpos not ascending": swap,
        "cpos twice": set_("before", "cpos", e0 + 1, sym["before"]["cpos"][e0]),
        "src at num_values": set_("before", "src", e0, nnz),
        "src negative": set_("after", "src", 0, -1),
        "slot beyond the slices": set_(
            "before", "slot", e0, len(sym["before"]["sliced_col"])),
        "slot in an empty long list": set_("after", "slot", 0, ~0),
        "row pointer not monotone": set_(
            "before", "ptr", row, int(sym["before"]["ptr"][row + 1]) + 1),
        "row pointer does not start at 0": set_("after", "ptr", 0, 1),
        "fewer values than the sources need": lambda y, sl: 5,
        "a colour nobody wears": empty_colour,
    }
    for what, change in bad.items():
        assert build(change) == EINVAL, what
    assert build() == 0
