"""The aggregation multigrid preconditioner on the device:
spmv::AmgPreconditioner, refresh, amg_apply, pcg_amg and gmres with it.

Nothing in the hierarchy or the cycle has a free summation order (the Galerkin
sums and the restriction add left to right, a maximum has no order), so levels,
aggregates, coarse operators, bounds and amg_apply are compared with
np.array_equal against the numpy restatement of amg_cases.py; its products are
oracle.csr_spmv / oracle.csr_spmv_sym, whose order the SpMV kernels keep.

Matrices: Poisson 11^3 and 24^3, test_gpu_pcg's banded matrix of 4 097 rows,
gmres_cases.convdiff(8) (nonsymmetric), test_gpu_sgs's ragged matrix (hub rows:
source lists of a few thousand entries), the arrow matrix of 130 rows (one
aggregate), a diagonal matrix (one level) and n = 1; plain and scaled S A S, the
symmetric ones in both storages; the defaults and min_coarse_rows = 20.

Solves: pcg_amg against test_gpu_chebyshev._pcg_ref with the restatement as
preconditioner through test_gpu_chebyshev._vs_ref unchanged, gmres(30) against
gmres_cases.gmres_ref through test_gpu_gmres._vs_ref unchanged.  dev_ref, the
restatement's own deviation between two summation orders of the dot products,
is printed and must stay below a tenth of the bars (1e-6 of the history) on
every case kept here.

X and z sit between guard words and are filled with a sentinel before every
call."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as ac
import gmres_cases as gc
import ilu0_cases as ic
import oracle
import test_gpu_chebyshev as tc
import test_gpu_gmres as tg
import test_gpu_pcg as tp
import test_gpu_sgs as ts
from spmv_amd import _lib, host
from test_gpu_bicgstab import _dot_chunked
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = tp.KMAX, tp.RTOL
OFFSETS = ((0, GUARD), (1, GUARD + 1))
EINVAL = -1


def _make_csr(name):
    if name == "arrow130":
        return ic.arrow(130)
    if name.startswith("convdiff"):
        return gc.convdiff(int(name[8:]))
    return ts._make_csr(name)


SYMMETRIC = ("poisson11", "poisson24", "banded4097", "ragged3001", "diag200",
             "diag1")
NAMES = SYMMETRIC + ("convdiff8", "arrow130")


def _oracle_of(csr):
    """The product of a general block as the plan it gets takes it: the
    sequential loop of oracle.csr_spmv, or -- a small block with more than 64
    entries per row on average, such as the coarse levels of the ragged matrix
    -- the fixed order of the sub-wavefront kernel."""
    rp, ci, va = (np.ascontiguousarray(csr[0], np.int32),
                  np.ascontiguousarray(csr[1], np.int32),
                  np.ascontiguousarray(csr[2], np.float64))
    lpr = ac.vector_lanes((rp, ci, va)) if FORMS["auto"] else 0
    if lpr:
        return lambda x: ac.spmv_vector((rp, ci, va), np.asarray(x), lpr)
    return lambda x: oracle.csr_spmv(rp, ci, va, np.ascontiguousarray(x))


# auto: the context's default rule picks the blocks' plans (sj_min_nnz = 0
# sends every block to the sliced jagged form, which keeps the sequential order)
FORMS = {"auto": True}


def restate(csr, n, symmetric, ncols=None, frozen=None, **options):
    """the restatement of one storage of the rows `csr` (general form)"""
    if not symmetric:
        return ac.AmgRef(csr, n, spmv0=_oracle_of(csr), spmv_of=_oracle_of,
                         ncols=ncols, frozen=frozen, **options)
    rows = gc.row_of(csr[0])
    low = csr[1] < rows
    lrp = np.concatenate([[0], np.cumsum(np.bincount(rows[low], minlength=n))])
    lower = (lrp.astype(np.int32), np.ascontiguousarray(csr[1][low]),
             np.ascontiguousarray(csr[2][low]))
    diag = np.zeros(n)
    on = csr[1] == rows
    diag[rows[on]] = csr[2][on]

    def spmv0(x):
        return oracle.csr_spmv_sym(*lower, diag, np.ascontiguousarray(x[:n]))
    return ac.AmgRef(lower, n, True, diag, spmv0=spmv0, spmv_of=_oracle_of,
                     ncols=ncols, frozen=frozen, **options)


def _same_hierarchy(M, ref, what):
    assert M.levels() == len(ref.levels), (what, M.levels(), len(ref.levels))
    for l, L in enumerate(ref.levels):
        assert M.rows(l) == L["n"], (what, l)
        assert M.lmax(l) == L["lmax"], (what, l, M.lmax(l), L["lmax"])
        if "step" in L:
            assert np.array_equal(M.aggregates(l), L["step"]["agg"]), (what, l)
        if l >= 1:
            rp, ci, va = M.level_matrix(l)
            assert M.non_zeros(l) == len(L["csr"][1]), (what, l)
            assert np.array_equal(rp, L["csr"][0]), (what, l)
            assert np.array_equal(ci, L["csr"][1]), (what, l)
            assert np.array_equal(va, L["csr"][2]), \
                (what, l, int(np.sum(va != L["csr"][2])), len(va))


class _Problem:
    """One matrix in its storages with its preconditioners, the restatements,
    right-hand sides, buffers and references (computed once)."""

    def __init__(self, exec_, comm, name, scaled, **options):  # noqa: F811
        self.name, self.exec_ = (name, "scaled" if scaled else "plain"), exec_
        csr = _make_csr(name)
        self.csr = tp._scaled(csr) if scaled else csr
        self.N = N = len(self.csr[0]) - 1
        self.norm_a = tp._norm_inf(self.csr)
        self.options = options
        rng = np.random.default_rng(N + 1)
        self.rhs = {"ones": self.spmv(np.ones(N)),
                    "rand": self.spmv(rng.uniform(-1, 1, N)),
                    "zero": np.zeros(N)}
        self.storages = (False, True) if name in SYMMETRIC else (False,)
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in self.storages}
        self.M = {sym: host.AmgPreconditioner(exec_, A, **options)
                  for sym, A in self.A.items()}
        self.ref = {sym: restate(self.csr, N, sym, **options)
                    for sym in self.storages}
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.AmgPcgWorkspace(exec_)
        self.gws = host.GmresWorkspace(exec_)
        self._refs = {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, v)

    def precond(self, r):
        return self.ref[False].apply(r)

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
        host.amg_apply(e, M or self.M[symmetric], self.d_b + 8 * r_off, d_z)
        z = self._read_guarded(z_off)
        assert np.array_equal(e.copy_to_host(self.d_b + 8 * r_off, self.N), r), \
            (self.name, "r changed")
        return z

    def solve(self, comm, rhs, kmax=KMAX, rtol=RTOL, symmetric=False,  # noqa: F811
              ws=None, x_off=GUARD, **kw):
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist = host.pcg_amg(comm, e, self.A[symmetric], self.M[symmetric],
                               self.d_b, d_x, kmax, rtol, ws or self.ws, **kw)
        x = self._read_guarded(x_off)
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x

    def gmres(self, comm, rhs, m, kmax=tg.KMAX, rtol=tg.RTOL,  # noqa: F811
              x_off=GUARD):
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist, status = host.gmres(comm, e, self.A[False], self.d_b, d_x, m,
                                     kmax, rtol, amg=self.M[False], ws=self.gws)
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

    def get(name, scaled, **options):
        key = (name, scaled, tuple(sorted(options.items())))
        if key not in ps:
            ps[key] = _Problem(exec_, comm, name, scaled, **options)
        return ps[key]
    yield get
    for p in ps.values():
        p.close()


MATS = [pytest.param(False, id="plain"), pytest.param(True, id="scaled")]
OPTS = [pytest.param({}, id="defaults"),
        pytest.param({"min_coarse_rows": 20}, id="coarse20")]


# ---- 1. the hierarchy, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("options", OPTS)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", NAMES)
def test_hierarchy_is_exact(problems, name, scaled, options):
    P = problems(name, scaled, **options)
    ref = P.ref[False]
    print(name, scaled, options, "levels", [L["n"] for L in ref.levels],
          "entries", [L["nnz"] for L in ref.levels],
          "lmax", [L["lmax"] for L in ref.levels],
          "plan bytes", P.M[False].plan_bytes())
    for sym in P.storages:
        _same_hierarchy(P.M[sym], P.ref[sym], (name, scaled, sym))
        assert P.M[sym].plan_bytes() >= 48 * P.N
    if len(P.storages) == 2:  # both storages: identical coarse levels
        for l in range(1, len(ref.levels)):
            for a, b in zip(P.M[True].level_matrix(l), P.M[False].level_matrix(l)):
                assert np.array_equal(a, b), (name, l)
            assert P.M[True].lmax(l) == P.M[False].lmax(l)
    if name.startswith("diag"):
        assert len(ref.levels) == 1
    if name == "poisson11" and options:
        assert len(ref.levels) >= 3
    if name == "poisson24" and not options and not scaled:
        assert [L["n"] for L in ref.levels] == [13824, 1685, 150]
    if name == "ragged3001" and not scaled:
        assert np.diff(ref.levels[0]["step"]["src_ptr"]).max() > 1000


# ---- 2. the application, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("options", OPTS)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", NAMES)
def test_apply_is_exact(problems, name, scaled, options):
    P = problems(name, scaled, **options)
    for rhs in ("rand", "ones"):
        r = P.rhs[rhs]
        for sym in P.storages:
            want = P.ref[sym].apply(r)
            for r_off, z_off in OFFSETS:
                z = P.apply(r, sym, r_off, z_off)
                assert np.array_equal(z, want), \
                    (name, scaled, sym, rhs, r_off, int(np.sum(z != want)))


@pytest.mark.parametrize("options", [
    {"smooth_degree": 1}, {"smooth_degree": 3}, {"coarse_scale": 1.6},
    {"smooth_degree": 1, "coarse_scale": 1.6, "coarse_degree": 1},
    {"max_levels": 1}, {"max_levels": 2, "theta": 0.0},
    {"eig_ratio": 10.0, "coarse_degree": 3, "min_coarse_rows": 20}],
    ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["poisson11", "convdiff8", "ragged3001"])
def test_apply_with_other_options(exec_, comm, name, options):  # noqa: F811
    P = _Problem(exec_, comm, name, True, **options)
    try:
        if "max_levels" in options:
            assert P.M[False].levels() == options["max_levels"]
        for sym in P.storages:
            _same_hierarchy(P.M[sym], P.ref[sym], (name, options, sym))
            want = P.ref[sym].apply(P.rhs["rand"])
            for r_off, z_off in OFFSETS:
                z = P.apply(P.rhs["rand"], sym, r_off, z_off)
                assert np.array_equal(z, want), (name, options, sym, r_off)
    finally:
        P.close()


def test_apply_errors(problems):
    P = problems("poisson11", False)
    e = P.exec_
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.amg_apply(e, P.M[False], P.d_x, P.d_x)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.amg_apply(e, P.M[False], P.d_x, P.d_x + 8 * (P.N - 1))
    with pytest.raises(host.SpmvHostError, match="NULL"):
        host.amg_apply(e, P.M[False], None, P.d_x)
    with pytest.raises(host.SpmvHostError, match="NULL"):
        host.amg_apply(e, P.M[False], P.d_b, None)
    with pytest.raises(host.SpmvHostError, match="min_coarse_rows"):
        host.AmgPreconditioner(e, P.A[False], min_coarse_rows=0)


@pytest.mark.parametrize("world", [2, 3])
def test_apply_on_slab_ranks(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking (one block with ghost columns) and an overlapping halo
    model: hierarchy and application of the rank's own diagonal block."""
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
        lrp, lci, lva = np.asarray(lrp), np.asarray(lci), np.asarray(lva)
        keep = lci < M  # the diagonal block
        brp = np.concatenate([[0], np.cumsum(np.bincount(
            gc.row_of(lrp)[keep], minlength=M))]).astype(np.int32)
        block = (brp, np.ascontiguousarray(lci[keep]),
                 np.ascontiguousarray(lva[keep]))
        r = r_glob[r0:r1]
        d_r = exec_.alloc(M + 1)
        d_z = exec_.alloc(M + 2 * GUARD)
        for sym in (False, True):
            ref = restate(block, M, sym, min_coarse_rows=20)
            assert len(ref.levels) >= 2
            want = ref.apply(r)
            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                pre = host.AmgPreconditioner(exec_, A, min_coarse_rows=20)
                what = (world, rank, sym, cm)
                _same_hierarchy(pre, ref, what)
                for r_off, z_off in OFFSETS:
                    exec_.copy_from_host(d_r + 8 * r_off, r)
                    exec_.copy_from_host(d_z, np.full(M + 2 * GUARD, SENTINEL))
                    host.amg_apply(exec_, pre, d_r + 8 * r_off, d_z + 8 * z_off)
                    buf = exec_.copy_to_host(d_z, M + 2 * GUARD)
                    assert np.all(buf[:z_off] == SENTINEL), what
                    assert np.all(buf[z_off + M:] == SENTINEL), what
                    assert np.array_equal(buf[z_off:z_off + M], want), what
                pre.close()
                A.close()
        exec_.free(d_r), exec_.free(d_z)

    tw.run(rank_body, gpu=True)


# ---- 3. refresh ----------------------------------------------------------------------------
def _changed(csr, eps):
    """2 A, perturbed entry by entry, symmetric where A is"""
    rp, ci, va = csr
    rows = tp._row_of(rp)[:len(ci)]
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)
    return rp, ci, 2.0 * va * (1.0 + eps * np.sin(3.0 * lo + 7.0 * hi))


def _write_values(exec_, A, csr, symmetric):  # noqa: F811
    """the matrix's coefficients rewritten in place on the device"""
    rp, ci, va = csr
    rows = tp._row_of(rp)[:len(ci)]
    values, diagonal = A.local_values()
    if symmetric:
        exec_.copy_from_host(values, va[ci < rows])
        exec_.copy_from_host(diagonal, va[ci == rows])
    else:
        exec_.copy_from_host(values, va)
    A.plan_values_changed()


@pytest.mark.parametrize("name", ["poisson11", "ragged3001", "convdiff8"])
def test_refresh_equals_a_fresh_object(exec_, comm, name):  # noqa: F811
    _refresh_case_plain(exec_, comm, name, "default plans")


def _refresh_case_plain(e, comm, name, what):  # noqa: F811
    """Two changes of the values.  eps = 0.05 moves the strength of connection:
    the refreshed object keeps its aggregates, as the restatement with frozen
    aggregates does.  eps = 1e-4 keeps them (checked on the restatement), so a
    fresh object on the new values is the same hierarchy, bit for bit."""
    csr = tp._scaled(_make_csr(name))
    N = len(csr[0]) - 1
    d_r, d_z = e.alloc(N), e.alloc(N)
    opts = {"min_coarse_rows": 20}

    def applied(pre, r):
        e.copy_from_host(d_r, r)
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.amg_apply(e, pre, d_r, d_z)
        return e.copy_to_host(d_z, N)
    for sym in ((False, True) if name in SYMMETRIC else (False,)):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        print(what, name, sym, "sjds", A.plan_get("sjds"))
        M = host.AmgPreconditioner(e, A, **opts)
        old = restate(csr, N, sym, **opts)
        _same_hierarchy(M, old, (name, sym, "old"))
        for eps in (0.05, 1e-4):
            new = _changed(csr, eps)
            r = oracle.csr_spmv(*new, np.random.default_rng(3).uniform(-1, 1, N))
            _write_values(e, A, new, sym)
            M.refresh(A)
            ref = restate(new, N, sym, frozen=old, **opts)
            _same_hierarchy(M, ref, (name, sym, eps, "refreshed"))
            want = ref.apply(r)
            assert np.array_equal(applied(M, r), want), (name, sym, eps)
            assert np.any(want != old.apply(r))
        fresh = restate(new, N, sym, **opts)
        for a, b in zip(fresh.levels, old.levels):  # the choice of eps
            assert ("step" in a) == ("step" in b)
            if "step" in a:
                assert np.array_equal(a["step"]["agg"], b["step"]["agg"])
        A2 = host.Matrix.create_matrix(comm, e, *new, N, N, [], [], sym,
                                       host.P2P_NONBLOCKING)
        M2 = host.AmgPreconditioner(e, A2, **opts)
        _same_hierarchy(M2, ref, (name, sym, "fresh"))
        assert np.array_equal(applied(M2, r), want), (name, sym, "fresh")
        # a non-positive diagonal: refused, unusable, then good again
        on = np.flatnonzero(new[1] == tp._row_of(new[0])[:len(new[1])])
        bad = (new[0], new[1], new[2].copy())
        bad[2][on[5 % len(on)]] = -1.0
        _write_values(e, A, bad, sym)
        with pytest.raises(host.SpmvHostError, match="diagonal is not positive"):
            M.refresh(A)
        with pytest.raises(host.SpmvHostError, match="refresh"):
            host.amg_apply(e, M, d_r, d_z)
        _write_values(e, A, new, sym)
        M.refresh(A)
        _same_hierarchy(M, ref, (name, sym, "refreshed again"))
        assert np.array_equal(applied(M, r), want), (name, sym, "again")
        for h in (M, M2, A, A2):
            h.close()
    e.free(d_r), e.free(d_z)


def test_refresh_on_a_baked_sliced_jagged_plan(comm):  # noqa: F811
    """sj_min_nnz = 0: the plans of level 0 AND of the coarse levels bake a
    sliced jagged copy of the values, which refresh must renew"""
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    FORMS["auto"] = False
    try:
        _refresh_case_plain(e, comm, "banded4097", "sj_min_nnz = 0")
    finally:
        FORMS["auto"] = True
        e.synchronize()
        e.close()


def test_refresh_refuses_another_pattern(problems):
    P, Q = problems("poisson11", False), problems("convdiff8", False)
    with pytest.raises(host.SpmvHostError, match="not the pattern"):
        P.M[False].refresh(Q.A[False])
    with pytest.raises(host.SpmvHostError, match="not the pattern"):
        P.M[False].refresh(P.A[True])


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
                host.AmgPreconditioner(exec_, A)
            A.close()


def test_a_released_matrix_is_refused(comm):  # noqa: F811
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    N = len(csr[0]) - 1
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        assert A.release_csr() > 0
        with pytest.raises(host.SpmvHostError, match="released"):
            host.AmgPreconditioner(e, A)
        A.close()
    e.synchronize()
    e.close()


# ---- 4. the C ABI checks every index ------------------------------------------------------
class _AmgHost(C.Structure):
    _fields_ = [("fine_rows", C.c_int32), ("coarse_rows", C.c_int32),
                ("num_values", C.c_int64), ("num_diagonal", C.c_int32),
                ("coarse_nnz", C.c_int64), ("agg", C.c_void_p),
                ("member_ptr", C.c_void_p), ("member", C.c_void_p),
                ("src_ptr", C.c_void_p), ("src", C.c_void_p),
                ("xrow_ptr", C.c_void_p), ("xrow_src", C.c_void_p)]


def test_plan_create_refuses_every_corrupted_index(exec_):  # noqa: F811
    """A hand-built step: 5 rows, aggregates {0, 1}, {2, 4}, {3}; 4 coarse
    entries over 9 values and a diagonal array."""
    hip = _lib.hip
    good = dict(agg=np.array([0, 0, 1, 2, 1], np.int32),
                member_ptr=np.array([0, 2, 4, 5], np.int32),
                member=np.array([0, 1, 2, 4, 3], np.int32),
                src_ptr=np.array([0, 3, 5, 8, 10], np.int64),
                src=np.array([0, 1, ~0, 2, 3, 4, ~2, 5, 8, ~4], np.int32),
                xrow_ptr=np.array([0, 2, 4, 6, 8, 10], np.int64),
                xrow_src=np.array([0, ~0, 1, ~1, 2, ~2, 3, ~3, 4, ~4], np.int32))

    def create(arrays, **scalars):
        s = dict(fine_rows=5, coarse_rows=3, num_values=9, num_diagonal=5,
                 coarse_nnz=4)
        s.update(scalars)
        a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        h = _AmgHost(**s, **{k: v.ctypes.data for k, v in a.items()})
        plan = C.c_void_p()
        rc = hip.spmv_hip_amg_plan_create(exec_.context, C.byref(h),
                                          C.byref(plan))
        if rc == 0:
            assert plan.value
            nbytes = C.c_int64()
            assert hip.spmv_hip_amg_plan_bytes(plan, C.byref(nbytes)) == 0
            assert nbytes.value > 0
            assert hip.spmv_hip_amg_plan_destroy(plan) == 0
        else:
            assert not plan.value
        return rc

    assert create(good) == 0

    def corrupt(key, index, value):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][index] = value
        return bad

    cases = [("agg out of range", corrupt("agg", 2, 3)),
             ("agg negative", corrupt("agg", 0, -1)),
             ("agg and members disagree", corrupt("agg", 4, 2)),
             ("member list out of order",
              dict(good, member=np.array([1, 0, 2, 4, 3], np.int32))),
             ("member out of range", corrupt("member", 4, 5)),
             ("member twice", corrupt("member", 1, 0)),
             ("member_ptr not monotone", corrupt("member_ptr", 1, 5)),
             ("member_ptr does not start at 0", corrupt("member_ptr", 0, 1)),
             ("member_ptr does not end at n", corrupt("member_ptr", 3, 4)),
             ("src out of range", corrupt("src", 3, 9)),
             ("src diagonal out of range", corrupt("src", 2, ~5)),
             ("src_ptr not monotone", corrupt("src_ptr", 2, 2)),
             ("src_ptr does not start at 0", corrupt("src_ptr", 0, 1)),
             ("xrow_src out of range", corrupt("xrow_src", 0, 9)),
             ("xrow_ptr not monotone", corrupt("xrow_ptr", 2, 1))]
    for what, bad in cases:
        assert create(bad) == EINVAL, what
    assert create(good, coarse_rows=6) == EINVAL
    assert create(good, num_diagonal=4) == EINVAL
    assert create(good, num_values=8) == EINVAL
    assert create(good, fine_rows=-1) == EINVAL


# ---- 5. the solves against their references -------------------------------------------------
SOLVE_NAMES = ("poisson11", "poisson24", "banded4097", "ragged3001")


@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("name", SOLVE_NAMES)
def test_pcg_amg_against_the_reference(comm, problems, name, scaled,  # noqa: F811
                                       rhs):
    P = problems(name, scaled)
    ref = P.pcg_ref(rhs)
    dev_ref = ref.dev(min(ref.k, 50) + 1)
    print(name, scaled, rhs, "k_ref", ref.k, "dev_ref", dev_ref)
    assert dev_ref <= 1e-7, "the bar of 1e-6 needs a reference ten times as sharp"
    for sym in P.storages:
        k, hist, x = P.solve(comm, rhs, symmetric=sym)
        assert k < KMAX
        if not sym:
            assert k == ref.k, (name, scaled, rhs, k, ref.k)
        tc._vs_ref(k, hist, x, ref, P.norm_a, (name, scaled, sym, rhs))


@pytest.mark.parametrize("name", ["convdiff8", "poisson11", "banded4097"])
def test_gmres_with_amg_against_the_reference(comm, problems, name):  # noqa: F811
    P = problems(name, True)
    ref = P.gmres_ref("rand", 30)
    k, hist, x, status = P.gmres(comm, "rand", 30)
    print(name, "k", k, "k_ref", ref.k, "status", status)
    assert k == ref.k and status == ref.status
    tg._vs_ref(k, hist, x, status, ref, P.spmv, (name, "gmres(30)", "amg"))


def test_gmres_takes_one_preconditioner(comm, problems):  # noqa: F811
    P = problems("poisson11", True)
    e = P.exec_
    S = host.SgsPreconditioner(e, P.A[False])
    try:
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            host.gmres(comm, e, P.A[False], P.d_b, P.d_x, 30, 5, 1e-8, sgs=S,
                       amg=P.M[False])
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            host.gmres(comm, e, P.A[False], P.d_b, P.d_x, 30, 5, 1e-8,
                       dinv_ptr=P.d_b, amg=P.M[False])
        with pytest.raises(host.SpmvHostError, match="preconditioner"):
            host.gmres(comm, e, P.A[False], P.d_b, P.d_x, 30, 5, 1e-8,
                       cheb=(2, 0.1, 2.0), amg=P.M[False])
        other = problems("convdiff8", True).M[False]
        with pytest.raises(host.SpmvHostError, match="rows"):
            host.gmres(comm, e, P.A[False], P.d_b, P.d_x, 30, 5, 1e-8, amg=other)
    finally:
        S.close()


# ---- 6. what it buys ---------------------------------------------------------------------------
def test_fewer_iterations_than_sgs_than_jacobi(comm, problems):  # noqa: F811
    """Poisson 24^3 to 1e-10.  On the CPU restatement with the defaults: AMG 21,
    SGS 51 (test_amg_host.py); only the inequalities are asserted."""
    P = problems("poisson24", False)
    e = P.exec_
    k_amg, _, _ = P.solve(comm, "rand", rtol=1e-10)
    S = host.SgsPreconditioner(e, P.A[False])
    d_dinv = e.alloc(P.N)
    try:
        e.copy_from_host(P.d_b, P.rhs["rand"])
        k_sgs, _ = host.pcg_sgs(comm, e, P.A[False], S, P.d_b, P._guarded(GUARD),
                                KMAX, 1e-10)
        P.A[False].diagonal(d_dinv)
        host.jacobi_inverse(e, d_dinv, d_dinv, P.N)
        k_pcg, _ = host.pcg(comm, e, P.A[False], P.d_b, P._guarded(GUARD), d_dinv,
                            KMAX, 1e-10)
    finally:
        S.close()
        e.free(d_dinv)
    print("poisson24 k pcg_amg", k_amg, "pcg_sgs", k_sgs, "pcg", k_pcg)
    assert k_amg < k_sgs < k_pcg


# ---- 7. pcg_sgs's remaining cases ----------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson11", "banded4097"])
def test_fixed_number_of_iterations(comm, problems, name):  # noqa: F811
    P = problems(name, True)
    for sym in P.storages:
        for kmax in (0, 1, 2, 7):
            k, hist, x = P.solve(comm, "ones", kmax=kmax, rtol=0.0, symmetric=sym)
            what = (name, sym, kmax)
            assert k == kmax, what
            assert hist.shape == (kmax + 1,) and np.all(hist > 0.0), what
            assert np.any(x != 0.0) == (kmax > 0), what
            ref = P.pcg_ref("ones", kmax, 0.0)
            assert np.allclose(hist, ref.hist, rtol=1e-6, atol=0.0), what
            # b = 0: stopped at k = 0 with x = 0, nothing undefined
            k, hist, x = P.solve(comm, "zero", kmax=kmax, rtol=0.0, symmetric=sym)
            assert k == 0 and np.all(x == 0.0), what
            assert hist.shape == (1,) and hist[0] == 0.0, what


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


@pytest.mark.parametrize("name", ["poisson11", "poisson24"])
def test_frozen_after_convergence(comm, problems, name):  # noqa: F811
    """poll_every = 255 and kmax far beyond the stop: every iteration is
    enqueued, the cycle goes on running on its own scratch, and x, the history
    and k do not change; poll_every = 1: the host stops enqueuing early."""
    P = problems(name, True)
    k, hist, x = P.solve(comm, "rand")
    assert 1 < k and k + 40 < 255
    for poll in (255, 1):
        got = P.solve(comm, "rand", kmax=k + 40, poll_every=poll)
        _same((k, hist, x), got, (name, poll))
    got = P.solve(comm, "rand", kmax=k)
    _same((k, hist, x), got, (name, "kmax = k"))


def test_workspace_reused_and_grown(comm, problems):  # noqa: F811
    e = problems("poisson11", True).exec_
    shared = host.AmgPcgWorkspace(e)
    plan = [("poisson11", 10, GUARD), ("poisson24", 12, GUARD + 1),
            ("banded4097", 6, GUARD), ("poisson24", 4, GUARD),
            ("poisson11", 12, GUARD + 1), ("poisson11", 0, GUARD)]
    for name, kmax, x_off in plan:
        P = problems(name, True)
        fresh = host.AmgPcgWorkspace(e)
        want = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=fresh, x_off=x_off)
        fresh.close()
        got = P.solve(comm, "rand", kmax=kmax, rtol=1e-6, ws=shared, x_off=x_off)
        _same(want, got, (name, kmax, x_off))
    shared.close()


def test_unaligned_x_keeps_the_bits(comm, problems):  # noqa: F811
    for name in ("poisson11", "banded4097"):
        P = problems(name, True)
        want = P.solve(comm, "rand", kmax=6)
        assert want[0] > 1
        got = P.solve(comm, "rand", kmax=6, x_off=GUARD + 1)
        _same(want, got, (name, "unaligned x"))
        e = P.exec_  # without a workspace of the caller's
        e.copy_from_host(P.d_b, P.rhs["rand"])
        k, hist = host.pcg_amg(comm, e, P.A[False], P.M[False], P.d_b,
                               P._guarded(GUARD), 6, RTOL)
        _same(want, (k, hist, P._read_guarded(GUARD)), (name, "no workspace"))


def test_time_spmv_counts_one_spmv_per_iteration(comm, problems):  # noqa: F811
    P = problems("poisson11", True)
    stats = {}
    k, _, _ = P.solve(comm, "rand", kmax=5, rtol=0.0, time_spmv=True, stats=stats)
    assert k == 5
    assert stats["spmv_launches"] == 5 and stats["spmv_ms_total"] > 0.0


def test_errors_leave_the_executor_as_it_was(comm, problems):  # noqa: F811
    P = problems("poisson11", True)
    e, A, M, N = P.exec_, P.A[False], P.M[False], P.N
    other = problems("banded4097", True).M[False]
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)
    try:
        e.copy_from_host(P.d_b, P.rhs["ones"])
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg_amg(comm, e, A, M, P.d_b, P.d_b, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.pcg_amg(comm, e, A, M, P.d_b, P.d_b + 8 * (N - 1), 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.pcg_amg(comm, e, A, M, P.d_b, P.d_x, -1, 1e-10)
        with pytest.raises(host.SpmvHostError, match="rows"):
            host.pcg_amg(comm, e, A, other, P.d_b, P.d_x, 5, 1e-10)
        assert tp._current_stream(e) == mine.value
        k, _ = host.pcg_amg(comm, e, A, M, P.d_b, P.d_x, 3, 0.0, P.ws)
        assert k == 3
        assert tp._current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


# ---- 8. several ranks ---------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_pcg_amg(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, general
    storage, a blocking and an overlapping halo model: the same k on every
    rank, k == k_ref, against the reference on oracle.dist_spmv with the
    block-diagonal preconditioner and the rank-ordered sum.

    The history is held to the existing bars where the reference's own
    deviation between two summation orders, dev_ref, is below a tenth of them
    (1e-7).  Measured on the CPU: 3 ranks 5.9e-9 and 1.3e-10 -- kept; 2 ranks
    4.8e-7 (49 iterations on two blocks of 256 rows, scaled by up to 1e4) --
    DROPPED from the history bar rather than widening it: there k, the
    convergence and the error of x are still asserted."""
    from thread_world import ThreadWorld
    (rp, ci, va), _ = tp._slab_inputs(8)
    N = len(rp) - 1
    norm_a = tp._norm_inf((rp, ci, va))
    b = oracle.csr_spmv(rp, ci, va, np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]
    opts = {"min_coarse_rows": 20}

    def dist_dot(dot):
        def f(u, v):
            s = 0.0
            for r in range(world):
                s += dot(u[ranges[r]:ranges[r + 1]], v[ranges[r]:ranges[r + 1]])
            return s
        return f

    pres = []
    for r in range(world):
        lrp, lci, lva = (np.asarray(a) for a in blocks[r][:3])
        M = int(ranges[r + 1] - ranges[r])
        keep = lci < M
        brp = np.concatenate([[0], np.cumsum(np.bincount(
            gc.row_of(lrp)[keep], minlength=M))]).astype(np.int32)
        pres.append(restate((brp, np.ascontiguousarray(lci[keep]),
                             np.ascontiguousarray(lva[keep])), M, False, **opts))

    def precond(v):
        return np.concatenate([pres[r].apply(v[ranges[r]:ranges[r + 1]])
                               for r in range(world)])
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    refs = {}
    for cm in models:
        def spmv(p, cm=cm):
            return oracle.dist_spmv(world, rp, ci, va, p, False, cm)
        refs[cm] = ts._Ref(spmv, dist_dot(oracle.ddot), dist_dot(_dot_chunked),
                           b, precond)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        ws = host.AmgPcgWorkspace(exec_)
        d_b = exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for cm, rf in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            pre = host.AmgPreconditioner(exec_, A, **opts)
            exec_.copy_from_host(d_b, b[r0:r1])
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
            k, hist = host.pcg_amg(comm, exec_, A, pre, d_b, d_x + 8 * GUARD,
                                   KMAX, RTOL, ws)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL)
            assert np.all(buf[GUARD + M:] == SENTINEL)
            ks = tw.gather(rank, np.array([k]))
            assert np.all(ks == k), ks
            xs = tw.gather(rank, buf[GUARD:GUARD + M])
            assert k < KMAX and k == rf.k, (world, cm, k, rf.k)
            dev_ref = rf.dev(min(rf.k, 50) + 1)
            print(world, cm, "k", k, "dev_ref", dev_ref)
            if world == 2:  # dropped from the history bar: see the docstring
                assert hist[k] / hist[0] < RTOL
                err = np.linalg.norm(xs - rf.x) / np.linalg.norm(rf.x)
                assert err <= 1e-8, (world, cm, err)
            else:
                assert dev_ref <= 1e-7, (world, cm, dev_ref)
                tc._vs_ref(k, hist, xs, rf, norm_a, (world, cm))
            pre.close()
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
