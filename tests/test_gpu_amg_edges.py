"""spmv::AmgPreconditioner on the cases of amg_edges.py: systems scaled by
powers of two (hierarchy, amg_apply, refresh and pcg_amg, bit for bit between two
GPU objects and against the restatement), poisoned right-hand sides followed by
clean ones on the same object and workspace, matrices whose row-sum bound is not
finite, and the cycle with every streaming kernel non-temporal.  Every comparison
is of bits (special_values.same_bits where a NaN may stand)."""
import numpy as np
import pytest

import amg_edges as ae
import solver_edges as se
import test_gpu_amg as ta
import test_gpu_pcg as tp
from special_values import same_bits
from spmv_amd import _lib, host
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD


class Dev:
    """One matrix in one storage with its preconditioner and buffers"""

    def __init__(self, e, comm, csr, symmetric, build=True):  # noqa: F811
        self.e, self.comm, self.csr, self.sym = e, comm, csr, symmetric
        self.N = N = len(csr[0]) - 1
        self.A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], symmetric,
                                           host.P2P_NONBLOCKING)
        self.M = host.AmgPreconditioner(e, self.A, **ae.OPTIONS) if build else None
        self.d_b, self.d_x = e.alloc(N), e.alloc(N + 2 * GUARD)
        self.ws, self.gws = host.AmgPcgWorkspace(e), host.GmresWorkspace(e)

    def _guarded(self):
        self.e.copy_from_host(self.d_x, np.full(self.N + 2 * GUARD, SENTINEL))
        return self.d_x + 8 * GUARD

    def _read(self, what):
        buf = self.e.copy_to_host(self.d_x, self.N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL), (what, "guard in front")
        assert np.all(buf[GUARD + self.N:] == SENTINEL), (what, "guard behind")
        out = buf[GUARD:GUARD + self.N].copy()
        assert not np.any(out == SENTINEL), (what, "not written")
        return out

    def apply(self, r, M=None):
        self.e.copy_from_host(self.d_b, np.ascontiguousarray(r, np.float64))
        host.amg_apply(self.e, M or self.M, self.d_b, self._guarded())
        z = self._read("amg_apply")
        assert same_bits(self.e.copy_to_host(self.d_b, self.N),
                         np.asarray(r, np.float64)), "r changed"
        return z

    def solve(self, b, kmax=ae.KMAX, rtol=ae.RTOL, ws=None):
        self.e.copy_from_host(self.d_b, np.ascontiguousarray(b, np.float64))
        k, hist = host.pcg_amg(self.comm, self.e, self.A, self.M, self.d_b,
                               self._guarded(), kmax, rtol, ws or self.ws)
        return k, hist.copy(), self._read("pcg_amg")

    def gmres(self, b, kmax=ae.KMAX, rtol=ae.RTOL, ws=None):
        self.e.copy_from_host(self.d_b, np.ascontiguousarray(b, np.float64))
        k, hist, status = host.gmres(self.comm, self.e, self.A, self.d_b,
                                     self._guarded(), 30, kmax, rtol, amg=self.M,
                                     ws=ws or self.gws)
        return k, hist.copy(), self._read("gmres"), status

    def write(self, csr):
        ta._write_values(self.e, self.A, csr, self.sym)

    def close(self):
        self.e.synchronize()
        self.ws.close(), self.gws.close()
        if self.M:
            self.M.close()
        self.A.close()
        self.e.free(self.d_b), self.e.free(self.d_x)


def _same_solve(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert same_bits(a[1], b[1]), (what, "history")
    assert same_bits(a[2], b[2]), (what, "x")
    assert len(a) == 3 or a[3] == b[3], (what, "status")


def _scaled_hierarchy(M, base, s, what):
    assert M.levels() == base.levels(), what
    for l in range(base.levels()):
        assert M.rows(l) == base.rows(l), (what, l)
        assert same_bits(np.array([M.lmax(l)]), np.array([base.lmax(l)])), \
            (what, l, M.lmax(l), base.lmax(l))
        if l + 1 < base.levels():
            assert np.array_equal(M.aggregates(l), base.aggregates(l)), (what, l)
        if l >= 1:
            got, want = M.level_matrix(l), base.level_matrix(l)
            assert np.array_equal(got[0], want[0]), (what, l)
            assert np.array_equal(got[1], want[1]), (what, l)
            assert same_bits(got[2], np.ldexp(want[2], s)), (what, l)


# ---- 1. scaling by powers of two -------------------------------------------------------
@pytest.mark.parametrize("name", ae.MATRICES)
def test_scaled_systems(exec_, comm, name):  # noqa: F811
    csr = ae.csr_of(name)
    N = len(csr[0]) - 1
    r = ae.clean_rhs(csr)
    for sym in ae.storages(name):
        ref = ta.restate(csr, N, sym, **ae.OPTIONS)
        D = Dev(exec_, comm, csr, sym)
        R = Dev(exec_, comm, csr, sym)  # refreshed onto every scaled matrix
        try:
            ta._same_hierarchy(D.M, ref, (name, sym))
            z = D.apply(r)
            assert same_bits(z, ref.apply(r)), (name, sym)
            base = D.solve(r)
            # (CG on the nonsymmetric matrix need not converge: the relation
            # holds for whatever it does in KMAX iterations)
            assert 1 < base[0] and np.all(np.isfinite(base[2]))
            assert base[0] < ae.KMAX or name not in ta.SYMMETRIC
            for s, t in ae.PAIRS:
                what = (name, sym, s, t)
                scaled = se.scale_csr(csr, s)
                S = Dev(exec_, comm, scaled, sym)
                try:
                    _scaled_hierarchy(S.M, D.M, s, what)
                    zs = S.apply(np.ldexp(r, t))
                    assert same_bits(zs, np.ldexp(z, t - s)), what
                    assert same_bits(zs, np.ldexp(ref.apply(r), t - s)), what
                    R.write(scaled)
                    R.M.refresh(R.A)
                    _scaled_hierarchy(R.M, D.M, s, (what, "refresh"))
                    assert same_bits(R.apply(np.ldexp(r, t)), zs), (what, "refresh")
                    k, hist, x = S.solve(np.ldexp(r, t))
                    assert k == base[0], (what, k, base[0])
                    assert same_bits(x, np.ldexp(base[2], t - s)), (what, "x")
                    assert same_bits(hist, np.ldexp(base[1], t)), (what, "history")
                finally:
                    S.close()
        finally:
            D.close(), R.close()


# ---- 2. poison, then clean ---------------------------------------------------------------
def _poison_then_clean(e, comm, name, oracle_of_auto=True):  # noqa: F811
    csr = ae.csr_of(name)
    N = len(csr[0]) - 1
    r = ae.clean_rhs(csr)
    ta.FORMS["auto"] = oracle_of_auto
    try:
        for sym in ae.storages(name):
            ref = ta.restate(csr, N, sym, **ae.OPTIONS)
            D = Dev(e, comm, csr, sym)
            try:
                z = D.apply(r)
                assert same_bits(z, ref.apply(r)) and np.all(np.isfinite(z))
                for value, row in ae.poisons(N, few=name == "ragged3001"):
                    what = (name, sym, value, row)
                    bad = ae.poisoned(r, value, row)
                    with np.errstate(all="ignore"):
                        want = ref.apply(bad)
                    # (1e300 stays finite in the cycle, which is linear in r;
                    # it overflows in the dot products of the solves below)
                    assert np.isfinite(value) != np.any(~np.isfinite(want)), what
                    assert same_bits(D.apply(bad), want), what
                    assert same_bits(D.apply(r), z), (what, "clean afterwards")
                # the same through the solvers, on one workspace
                fresh = host.AmgPcgWorkspace(e)
                clean = D.solve(r, ws=fresh)
                fresh.close()
                assert 1 < clean[0] and np.all(np.isfinite(clean[2]))
                assert clean[0] < ae.KMAX or name not in ta.SYMMETRIC
                for value, row in ae.poisons(N, few=True):
                    what = (name, sym, value, row, "pcg_amg")
                    k, hist, x = D.solve(ae.poisoned(r, value, row),
                                         kmax=ae.POISON_KMAX)
                    assert k == ae.POISON_KMAX, (what, k)  # never "converged"
                    assert not np.all(np.isfinite(hist)), what
                    _same_solve(D.solve(r), clean, what)
                if not sym:
                    fresh = host.GmresWorkspace(e)
                    clean = D.gmres(r, ws=fresh)
                    fresh.close()
                    D.gmres(ae.poisoned(r, np.nan, N // 2), kmax=ae.POISON_KMAX)
                    _same_solve(D.gmres(r), clean, (name, "gmres"))
            finally:
                D.close()
    finally:
        ta.FORMS["auto"] = True


@pytest.mark.parametrize("name", ae.MATRICES)
def test_poison_then_clean(exec_, comm, nt, name):  # noqa: F811
    _poison_then_clean(exec_, comm, name)


def test_poison_then_clean_on_sliced_jagged_coarse_levels(comm):  # noqa: F811
    """sj_min_nnz = 0: every block, the coarse ones included, takes the sliced
    jagged plan (sequential order)"""
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    try:
        for name in ("poisson11", "ragged3001"):
            _poison_then_clean(e, comm, name, oracle_of_auto=False)
    finally:
        e.synchronize()
        e.close()


# ---- 3. a bound that is not finite ---------------------------------------------------------
@pytest.mark.parametrize("make", [ae.tiny_diagonal, ae.huge_pairs],
                         ids=["tiny_diagonal", "huge_pairs"])
def test_a_bound_that_is_not_finite_is_refused(exec_, comm, make):  # noqa: F811
    csr = ae.csr_of("poisson11")
    N = len(csr[0]) - 1
    bad = make(csr)
    r = ae.clean_rhs(csr)
    for sym in (False, True):
        B = Dev(exec_, comm, bad, sym, build=False)
        D = Dev(exec_, comm, csr, sym)
        try:
            with pytest.raises(host.SpmvHostError, match="row-sum bound"):
                host.AmgPreconditioner(exec_, B.A, **ae.OPTIONS)
            z = D.apply(r)
            D.write(bad)
            with pytest.raises(host.SpmvHostError, match="row-sum bound"):
                D.M.refresh(D.A)
            with pytest.raises(host.SpmvHostError, match="refresh before"):
                host.amg_apply(exec_, D.M, D.d_b, D.d_x)
            D.write(csr)
            D.M.refresh(D.A)
            assert same_bits(D.apply(r), z), (make.__name__, sym)
        finally:
            B.close(), D.close()


def test_a_nan_far_from_the_diagonal_is_accepted(exec_, comm):  # noqa: F811
    """Documents the maximum rule (a NaN never replaces a number): the bound
    stays finite, refresh succeeds and the application is the restatement's,
    NaNs included.  It does not call the result useful."""
    csr = ae.csr_of("poisson11")
    N = len(csr[0]) - 1
    r = ae.clean_rhs(csr)
    bad, _ = ae.nan_far(csr, ta.restate(csr, N, False, **ae.OPTIONS))
    for sym in (False, True):
        old = ta.restate(csr, N, sym, **ae.OPTIONS)
        with np.errstate(all="ignore"):
            ref = ta.restate(bad, N, sym, frozen=old, **ae.OPTIONS)
            want = ref.apply(r)
        D = Dev(exec_, comm, csr, sym)
        try:
            D.write(bad)
            D.M.refresh(D.A)
            for l, L in enumerate(ref.levels):
                assert D.M.lmax(l) == L["lmax"] and np.isfinite(L["lmax"]), (sym, l)
                if l >= 1:
                    assert same_bits(D.M.level_matrix(l)[2], L["csr"][2]), (sym, l)
            assert np.any(np.isnan(want)) and same_bits(D.apply(r), want), sym
        finally:
            D.close()


# ---- 4. the cycle with every streaming kernel non-temporal -----------------------------------
@pytest.mark.parametrize("name", ["poisson11", "ragged3001"])
def test_apply_is_exact_non_temporal(exec_, comm, name):  # noqa: F811
    """test_gpu_amg.test_apply_is_exact's comparison at blas1_nt_min_elems = 1"""
    _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems", 1)
    P = None
    try:
        P = ta._Problem(exec_, comm, name, True, **ae.OPTIONS)
        for rhs in ("rand", "ones"):
            r = P.rhs[rhs]
            for sym in P.storages:
                want = P.ref[sym].apply(r)
                for r_off, z_off in ta.OFFSETS:
                    z = P.apply(r, sym, r_off, z_off)
                    assert np.array_equal(z, want), \
                        (name, sym, rhs, r_off, int(np.sum(z != want)))
    finally:
        _lib.call("spmv_hip_ctx_set_option", exec_.context, b"blas1_nt_min_elems",
                  tp.NT_DEFAULT)
        if P is not None:
            P.close()
