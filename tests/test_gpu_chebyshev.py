"""The Chebyshev polynomial preconditioner: spmv::chebyshev_apply,
pcg_chebyshev and lambda_max_estimate.

Shapes, matrices and bars are those of test_gpu_pcg.py (its generators and its
reference are imported, not copied): 1 331 rows (odd; less than one streaming
unit of 2 048 doubles), 13 824 rows, 4 097 rows (odd), each plain and scaled to
S A S, both storages; both instantiations (cached / non-temporal) of every
kernel run through `blas1_nt_min_elems`.

chebyshev_apply has no reductions, so it is compared with np.array_equal
against the numpy restatement of cg.h.  The SpMV of the restatement is
oracle.csr_spmv for general storage; for symmetric storage and for several
ranks it is the project's own Matrix.mult round trip, code this preconditioner
does not touch.

pcg_chebyshev is compared against test_gpu_pcg._pcg_ref's recurrence with
z = M(r), on oracle.csr_spmv / oracle.ddot.  The bounds are fixed constants so
that the GPU and the reference use the same numbers: lmax = 2.2 bounds the
spectrum of D^-1 A of every matrix here (< 2 for the Poisson matrices, < 1.95
by Gershgorin for the band), lmin = lmax / 30.  The reference is run in two
summation orders of the dot product (oracle.ddot; chunks of 1 024 summed
pairwise, as test_gpu_bicgstab.py); `dev_ref` is the deviation of their
histories.  Bars: |k - k_ref| <= 1; history to 1e-6 over min(k, k_ref, 50)
entries above the noise floor -- max(1e-6, 10 * dev_ref) where dev_ref exceeds
1e-7, and a case with dev_ref > 1e-5 FAILS instead; ||x - x_ref|| <= 1e-8
||x_ref||.

X, and z of chebyshev_apply, sit between guard words and are filled with a
sentinel before every call."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_pcg as tp
from spmv_amd import _lib, host
from test_gpu_bicgstab import _dot_chunked
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = tp.KMAX, tp.RTOL
LMAX = 2.2
LMIN = LMAX / 30
SHAPES = tp.SHAPES


# ---- cg.h restated in numpy -------------------------------------------------------
def _coefficients(degree, lmin, lmax):
    theta = 0.5 * (lmax + lmin)
    delta = 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    a, b = [0.0], [1.0 / theta]
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        a.append(rho_new * rho)
        b.append(2.0 * rho_new / delta)
        rho = rho_new
    return a, b


def _apply_ref(spmv, r, dinv, degree, lmin=LMIN, lmax=LMAX):
    """z = q(dinv*A) dinv r; every numpy operation is one rounding per element"""
    a, b = _coefficients(degree, lmin, lmax)
    scaled = (lambda v: dinv * v) if dinv is not None else (lambda v: v)
    d = b[0] * scaled(r)
    z = d.copy()
    for j in range(1, degree):
        w = spmv(z)
        d = a[j] * d + b[j] * scaled(r - w)
        z = z + d
    return z


def _pcg_ref(spmv, dot, b, precond, kmax, rtol):
    """test_gpu_pcg._pcg_ref with z = precond(r) -> (x, k, history)"""
    x = np.zeros(len(b))
    r = np.array(b, dtype=np.float64)
    z = precond(r)
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
        r = r - alpha * Ap
        z = precond(r)
        rz_new, rr = dot(r, z), dot(r, r)
        x = x + alpha * p
        hist.append(math.sqrt(rr))
        if math.sqrt(rr) / math.sqrt(rr0) < rtol:
            break
        beta = rz_new / rz
        rz = rz_new
        p = beta * p + z
    return x, k, np.array(hist)


def _lambda_ref(spmv, dot, dinv, v0, steps):
    q = v0 / math.sqrt(dot(v0, v0))
    lam = 0.0
    for _ in range(steps):
        v = dinv * (q / 1.0)
        u = spmv(v)
        lam = dot(v, u) / dot(v, q)
        q = u / math.sqrt(dot(u, u))
    return lam


class _Ref:
    """The reference of one case in both summation orders"""

    def __init__(self, spmv, dot, dot2, b, dinv, degree, kmax=KMAX, rtol=RTOL):
        def M(r):
            return _apply_ref(spmv, r, dinv, degree)
        self.x, self.k, self.hist = _pcg_ref(spmv, dot, b, M, kmax, rtol)
        self.second = _pcg_ref(spmv, dot2, b, M, kmax, rtol)

    def dev(self, m):
        m = min(m, self.second[1])
        if m == 0:
            return 0.0
        return float(np.abs(self.second[2][:m] / self.hist[:m] - 1).max())


def _vs_ref(k, hist, x, ref, norm_a, what, kmax=KMAX, rtol=RTOL):
    """Every figure is printed before anything is asserted."""
    m = min(k, ref.k, 50)
    upto = m + 1 if ref.hist[m] >= tp._noise_floor(norm_a, ref.x) else m
    dev_ref = ref.dev(upto)
    dev = float(np.abs(hist[:upto] / ref.hist[:upto] - 1).max()) if upto else 0.0
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    err_ref = np.linalg.norm(ref.second[0] - ref.x) / np.linalg.norm(ref.x)
    print(what, "k", k, "k_ref", ref.k, "k_ref (second order)", ref.second[1],
          "history deviation", dev, "dev_ref", dev_ref, "x error", err,
          "x error between the references", err_ref)
    assert abs(k - ref.k) <= 1, (what, k, ref.k)
    assert len(hist) == k + 1, what
    if 0 < k < kmax:
        assert hist[k] / hist[0] < rtol, what
    assert dev_ref <= 1e-5, (what, "the reference disagrees with itself", dev_ref)
    bar = 1e-6 if dev_ref <= 1e-7 else max(1e-6, 10 * dev_ref)
    assert dev <= bar, (what, dev, dev_ref)
    assert err <= 1e-8, (what, err)


class _Problem:
    """One matrix (a shape, plain or scaled) in both storages with its Jacobi
    dinv on the device, right-hand sides, buffers and references (computed
    once)."""

    def __init__(self, exec_, comm, shape, scaled):
        self.name, self.exec_ = (shape, "scaled" if scaled else "plain"), exec_
        csr = tp._csr(shape)
        self.csr = tp._scaled(csr) if scaled else csr
        self.N = N = len(self.csr[0]) - 1
        self.diag = tp._diag_of(self.csr)
        self.dinv = 1.0 / self.diag
        self.norm_a = tp._norm_inf(self.csr)
        rng = np.random.default_rng(N + 1)
        self.rhs = {"ones": self.spmv(np.ones(N)),
                    "rand": self.spmv(rng.uniform(-1, 1, N)),
                    "zero": np.zeros(N)}
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.d_dinv = exec_.alloc(N + 1)
        self.A[False].diagonal(self.d_dinv)
        host.jacobi_inverse(exec_, self.d_dinv, self.d_dinv, N)
        assert np.array_equal(exec_.copy_to_host(self.d_dinv, N), self.dinv)
        self.d_ones = exec_.alloc(N)
        exec_.copy_from_host(self.d_ones, np.ones(N))
        self.d_b = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.d_in, self.d_out = exec_.alloc(N), exec_.alloc(N)
        self.ws = host.ChebyshevWorkspace(exec_)
        self._ref = {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, v)

    def device_spmv(self, sym):
        """the project's Matrix.mult round trip"""
        e, A, N = self.exec_, self.A[sym], self.N

        def spmv(v):
            e.copy_from_host(self.d_in, v)
            A.col_map().update(self.d_in)
            A.mult(self.d_in, self.d_out)
            return e.copy_to_host(self.d_out, N)
        return spmv

    def ref(self, rhs, degree, kmax=KMAX, rtol=RTOL):
        key = (rhs, degree, kmax, rtol)
        if key not in self._ref:
            self._ref[key] = _Ref(self.spmv, oracle.ddot, _dot_chunked,
                                  self.rhs[rhs], self.dinv, degree, kmax, rtol)
        return self._ref[key]

    def _guarded(self, off):
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        return self.d_x + 8 * off

    def _read_guarded(self, off):
        N = self.N
        buf = self.exec_.copy_to_host(self.d_x, N + 2 * GUARD)
        assert np.all(buf[:off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[off + N:] == SENTINEL), (self.name, "guard behind")
        out = buf[off:off + N].copy()
        assert np.all(np.isfinite(out)) and not np.any(out == SENTINEL), self.name
        return out

    def apply(self, r, degree, symmetric=False, dinv="jacobi", r_off=0,
              z_off=GUARD, ws=None, lmin=LMIN, lmax=LMAX):
        """-> z; r_off / z_off in doubles (1 / GUARD + 1: 8 bytes off)"""
        e = self.exec_
        e.copy_from_host(self.d_b + 8 * r_off, r)
        d_z = self._guarded(z_off)
        d_dinv = {"jacobi": self.d_dinv, "ones": self.d_ones, None: None}[dinv]
        host.chebyshev_apply(e, self.A[symmetric], self.d_b + 8 * r_off, d_z,
                             d_dinv, degree, lmin, lmax, ws or self.ws)
        return self._read_guarded(z_off)

    def solve(self, comm, rhs, degree, kmax=KMAX, rtol=RTOL, symmetric=False,
              ws=None, x_off=GUARD, d_dinv=None, **kw):
        """-> (k, history, x)"""
        e = self.exec_
        e.copy_from_host(self.d_b, self.rhs[rhs])
        d_x = self._guarded(x_off)
        k, hist = host.pcg_chebyshev(comm, e, self.A[symmetric], self.d_b, d_x,
                                     d_dinv or self.d_dinv, degree, LMIN, LMAX,
                                     kmax, rtol, ws or self.ws, **kw)
        x = self._read_guarded(x_off)
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_dinv, self.d_ones, self.d_b, self.d_x, self.d_in,
                  self.d_out):
            self.exec_.free(p)


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    ps = {(shape, scaled): _Problem(exec_, comm, shape, scaled)
          for shape in SHAPES for scaled in (False, True)}
    yield ps
    for p in ps.values():
        p.close()


MATS = [pytest.param(False, id="plain"), pytest.param(True, id="scaled")]
STORAGE = [pytest.param(False, id="general"), pytest.param(True, id="symmetric")]


# ---- 1. chebyshev_apply is exact ------------------------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_is_exact(problems, nt, shape, scaled, symmetric):  # noqa: F811
    P = problems[(shape, scaled)]
    spmv = P.device_spmv(True) if symmetric else P.spmv
    r = P.rhs["rand"]
    for degree in (1, 2, 3, 8):
        want = _apply_ref(spmv, r, P.dinv, degree)
        plain = _apply_ref(spmv, r, None, degree)
        assert np.any(want != plain)
        for r_off, z_off in ((0, GUARD), (1, GUARD + 1), (0, GUARD + 1)):
            what = (shape, scaled, symmetric, degree, r_off, z_off)
            z = P.apply(r, degree, symmetric, "jacobi", r_off, z_off)
            assert np.array_equal(z, want), (what, "dinv")
            z = P.apply(r, degree, symmetric, None, r_off, z_off)
            assert np.array_equal(z, plain), (what, "no dinv")
        z = P.apply(r, degree, symmetric, "ones")
        assert np.array_equal(z, plain), (shape, scaled, symmetric, degree,
                                          "dinv = 1")
        # without a workspace of the caller's
        e = P.exec_
        e.copy_from_host(P.d_b, r)
        d_z = P._guarded(GUARD)
        host.chebyshev_apply(e, P.A[symmetric], P.d_b, d_z, P.d_dinv, degree,
                             LMIN, LMAX)
        assert np.array_equal(P._read_guarded(GUARD), want)


def test_apply_unaligned_dinv_and_errors(problems, nt):  # noqa: F811
    P = problems[("banded4097", True)]
    e, N = P.exec_, P.N
    r = P.rhs["rand"]
    want = P.apply(r, 3)
    d = e.alloc(N + 1)
    e.copy(d + 8, P.d_dinv, N * 8)
    e.copy_from_host(P.d_b, r)
    host.chebyshev_apply(e, P.A[False], P.d_b, P._guarded(GUARD), d + 8, 3, LMIN,
                         LMAX, P.ws)
    assert np.array_equal(P._read_guarded(GUARD), want)
    e.free(d)
    with pytest.raises(host.SpmvHostError, match="degree"):
        host.chebyshev_apply(e, P.A[False], P.d_b, P.d_x, P.d_dinv, 0, LMIN, LMAX)
    with pytest.raises(host.SpmvHostError, match="degree"):
        host.chebyshev_apply(e, P.A[False], P.d_b, P.d_x, P.d_dinv, 17, LMIN, LMAX)
    with pytest.raises(host.SpmvHostError, match="bounds"):
        host.chebyshev_apply(e, P.A[False], P.d_b, P.d_x, P.d_dinv, 3, LMAX, LMIN)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.chebyshev_apply(e, P.A[False], P.d_b, P.d_b + 8, P.d_dinv, 3, LMIN,
                             LMAX)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.chebyshev_apply(e, P.A[False], P.d_b, P.d_dinv, P.d_dinv, 3, LMIN,
                             LMAX)


@pytest.mark.parametrize("world", [2, 3])
def test_apply_on_slab_ranks(world):
    """Ranks as threads, the Poisson matrix of 8^3 (scaled) in slabs, both
    storages, a blocking and an overlapping halo model: bit for bit the
    restatement on the rank's own Matrix.mult round trip."""
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
        npad = M + len(gh)
        r, dinv = r_glob[r0:r1], 1.0 / diag[r0:r1]
        ws = host.ChebyshevWorkspace(exec_)
        d_r, d_dinv = exec_.alloc(M + 1), exec_.alloc(M)
        d_z = exec_.alloc(M + 2 * GUARD)
        d_in, d_out = exec_.alloc(npad), exec_.alloc(M)
        exec_.copy_from_host(d_dinv, dinv)
        for sym in (False, True):
            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)

                def spmv(v):
                    exec_.copy_from_host(d_in, np.concatenate(
                        [v, np.zeros(npad - M)]))
                    A.col_map().update(d_in)
                    A.mult(d_in, d_out)
                    return exec_.copy_to_host(d_out, M)

                for degree in (1, 2, 3, 8):
                    for dv, d_dv in ((dinv, d_dinv), (None, None)):
                        want = _apply_ref(spmv, r, dv, degree)
                        for r_off, z_off in ((0, GUARD), (1, GUARD + 1)):
                            exec_.copy_from_host(d_r + 8 * r_off, r)
                            exec_.copy_from_host(
                                d_z, np.full(M + 2 * GUARD, SENTINEL))
                            host.chebyshev_apply(exec_, A, d_r + 8 * r_off,
                                                 d_z + 8 * z_off, d_dv, degree,
                                                 LMIN, LMAX, ws)
                            buf = exec_.copy_to_host(d_z, M + 2 * GUARD)
                            what = (world, rank, sym, cm, degree, dv is None,
                                    r_off)
                            assert np.all(buf[:z_off] == SENTINEL), what
                            assert np.all(buf[z_off + M:] == SENTINEL), what
                            assert np.array_equal(buf[z_off:z_off + M], want), \
                                what
                A.close()
        for p in (d_r, d_dinv, d_z, d_in, d_out):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)


# ---- 2. pcg_chebyshev against the reference ----------------------------------------
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("degree", [1, 4, 8])
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_reference(comm, problems, nt, shape, scaled,  # noqa: F811
                               symmetric, degree, rhs):
    P = problems[(shape, scaled)]
    ref = P.ref(rhs, degree)
    k, hist, x = P.solve(comm, rhs, degree, symmetric=symmetric)
    assert k < KMAX
    _vs_ref(k, hist, x, ref, P.norm_a, (shape, scaled, symmetric, degree, rhs))


# ---- 3. what it is for: a relation between two references ------------------------
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", ["poisson11", "poisson24"])
def test_degree_4_halves_the_iterations_of_jacobi(problems, shape, scaled):
    P = problems[(shape, scaled)]
    k_cheb = P.ref("rand", 4).k
    _, k_jacobi, _ = tp._pcg_ref(P.spmv, oracle.ddot, P.rhs["rand"], P.dinv,
                                 KMAX, RTOL)
    print(shape, scaled, "k_ref_chebyshev", k_cheb, "k_ref_jacobi", k_jacobi)
    assert 2 * k_cheb < k_jacobi


# ---- 4. degree 1 degenerates to Jacobi-PCG -----------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_degree_1_is_jacobi_pcg(comm, problems, nt, shape, scaled,  # noqa: F811
                                symmetric):
    P = problems[(shape, scaled)]
    for rhs in ("ones", "rand"):
        x_ref, k_ref, _ = tp._pcg_ref(P.spmv, oracle.ddot, P.rhs[rhs], P.dinv,
                                      KMAX, RTOL)
        k, hist, x = P.solve(comm, rhs, 1, symmetric=symmetric)
        err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
        print(shape, scaled, symmetric, rhs, "k", k, "k_ref", k_ref, "x error",
              err)
        assert abs(k - k_ref) <= 1
        assert err <= 1e-8


# ---- 5. pcg's remaining cases --------------------------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape,  # noqa: F811
                                    symmetric):
    P = problems[(shape, True)]
    for degree in (1, 2, 4):
        for kmax in (0, 1, 2, 7):
            k, hist, x = P.solve(comm, "ones", degree, kmax=kmax, rtol=0.0,
                                 symmetric=symmetric)
            what = (shape, symmetric, degree, kmax)
            assert k == kmax, what
            assert hist.shape == (kmax + 1,) and np.all(hist > 0.0), what
            assert np.any(x != 0.0) == (kmax > 0), what
            ref = P.ref("ones", degree, kmax, 0.0)
            assert np.allclose(hist, ref.hist, rtol=1e-6, atol=0.0), what
            # b = 0: stopped at k = 0 with x = 0, nothing undefined
            k, hist, x = P.solve(comm, "zero", degree, kmax=kmax, rtol=0.0,
                                 symmetric=symmetric)
            assert k == 0 and np.all(x == 0.0), what
            assert hist.shape == (1,) and hist[0] == 0.0, what


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what


@pytest.mark.parametrize("degree", [1, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_after_convergence(comm, problems, nt, shape, degree):  # noqa: F811
    """poll_every = 255 and kmax far beyond the stop: every iteration is
    enqueued, so every kernel launched after `done` had the chance to touch x;
    poll_every = 1: the host stops enqueuing early."""
    P = problems[(shape, True)]
    k, hist, x = P.solve(comm, "rand", degree)
    assert 1 < k and k + 80 < 255
    for poll in (255, 1):
        got = P.solve(comm, "rand", degree, kmax=k + 80, poll_every=poll)
        _same((k, hist, x), got, (shape, degree, poll))
    got = P.solve(comm, "rand", degree, kmax=k)
    _same((k, hist, x), got, (shape, degree, "kmax = k"))


def test_workspace_reused_and_grown(comm, problems, nt):  # noqa: F811
    """One workspace across shapes (small, large, middle), degrees, a smaller
    kmax and chebyshev_apply in between: every result equals the one on a fresh
    workspace, bit for bit."""
    e = problems[("poisson11", True)].exec_
    shared = host.ChebyshevWorkspace(e)
    plan = [("poisson11", 4, 30, GUARD), ("poisson24", 2, 40, GUARD + 1),
            ("banded4097", 8, 12, GUARD), ("poisson24", 1, 7, GUARD),
            ("poisson11", 3, 40, GUARD + 1), ("poisson11", 4, 0, GUARD)]
    for shape, degree, kmax, x_off in plan:
        P = problems[(shape, True)]
        fresh = host.ChebyshevWorkspace(e)
        want = P.solve(comm, "rand", degree, kmax=kmax, rtol=1e-6, ws=fresh,
                       x_off=x_off)
        z_want = P.apply(P.rhs["ones"], degree, ws=fresh)
        fresh.close()
        got = P.solve(comm, "rand", degree, kmax=kmax, rtol=1e-6, ws=shared,
                      x_off=x_off)
        _same(want, got, (shape, degree, kmax, x_off))
        assert np.array_equal(P.apply(P.rhs["ones"], degree, ws=shared), z_want)
    shared.close()


def test_unaligned_x_and_dinv_keep_the_bits(exec_, comm, problems, nt):  # noqa: F811
    for shape in SHAPES:
        P = problems[(shape, True)]
        d = exec_.alloc(P.N + 1)
        exec_.copy(d + 8, P.d_dinv, P.N * 8)
        for degree in (1, 4):
            want = P.solve(comm, "rand", degree, kmax=25)
            assert want[0] > 1
            got = P.solve(comm, "rand", degree, kmax=25, x_off=GUARD + 1)
            _same(want, got, (shape, degree, "unaligned x"))
            got = P.solve(comm, "rand", degree, kmax=25, d_dinv=d + 8)
            _same(want, got, (shape, degree, "unaligned dinv"))
        exec_.free(d)


def test_time_spmv_counts_every_spmv(comm, problems):  # noqa: F811
    P = problems[("poisson11", True)]
    stats = {}
    k, _, _ = P.solve(comm, "rand", 4, kmax=5, rtol=0.0, time_spmv=True,
                      stats=stats)
    assert k == 5
    assert stats["spmv_launches"] == 5 * 4 and stats["spmv_ms_total"] > 0.0


def test_errors_leave_the_executor_as_it_was(comm, problems):  # noqa: F811
    P = problems[("poisson11", True)]
    e, A, N = P.exec_, P.A[False], P.N
    dinv = P.d_dinv
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)

    def solve(b, x, dv, degree=4, lmin=LMIN, lmax=LMAX, kmax=5):
        return host.pcg_chebyshev(comm, e, A, b, x, dv, degree, lmin, lmax, kmax,
                                  1e-10)
    try:
        e.copy_from_host(P.d_b, P.rhs["ones"])
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, P.d_b, dinv)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, P.d_b + 8 * (N - 1), dinv)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, dinv, dinv)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            solve(P.d_b, dinv + 8, dinv)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            solve(P.d_b, P.d_x, dinv, kmax=-1)
        for degree in (0, 17):
            with pytest.raises(host.SpmvHostError, match="degree"):
                solve(P.d_b, P.d_x, dinv, degree=degree)
        for lmin, lmax in ((0.0, LMAX), (LMAX, LMIN), (LMIN, float("inf")),
                           (float("nan"), LMAX)):
            with pytest.raises(host.SpmvHostError, match="bounds"):
                solve(P.d_b, P.d_x, dinv, lmin=lmin, lmax=lmax)
        assert tp._current_stream(e) == mine.value
        # dinv is as it was
        assert np.array_equal(e.copy_to_host(dinv, N), P.dinv)
        # ... and after a solve that went through
        k, _ = host.pcg_chebyshev(comm, e, A, P.d_b, P.d_x, dinv, 4, LMIN, LMAX,
                                  3, 0.0, P.ws)
        assert k == 3
        assert tp._current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


# ---- 6. several ranks -------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_pcg_chebyshev(world):
    """Ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking and an overlapping halo model, ONE workspace per rank
    over all solves; against the reference on oracle.dist_spmv with the
    rank-ordered sum."""
    from thread_world import ThreadWorld
    (rp, ci, va), diag = tp._slab_inputs(8)
    N = len(rp) - 1
    norm_a = tp._norm_inf((rp, ci, va))
    rng = np.random.default_rng(world)
    bs = [oracle.csr_spmv(rp, ci, va, np.ones(N)),
          oracle.csr_spmv(rp, ci, va, rng.uniform(-1, 1, N))]
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)
    # (degree, right-hand side): every degree, both right-hand sides where the
    # reference is cheap
    cases = ((1, 0), (1, 1), (4, 0), (4, 1), (8, 1))

    def dist_dot(dot):
        def f(a, b):
            s = 0.0
            for r in range(world):
                s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
            return s
        return f

    refs = {}
    for sym in (False, True):
        for cm in models:
            def spmv(p, sym=sym, cm=cm):
                return oracle.dist_spmv(world, rp, ci, va, p, sym, cm)
            refs[(sym, cm)] = {
                (degree, j): _Ref(spmv, dist_dot(oracle.ddot),
                                  dist_dot(_dot_chunked), bs[j], 1.0 / diag,
                                  degree)
                for degree, j in cases}
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        ws = host.ChebyshevWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for (sym, cm), ref in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, cm)
            A.diagonal(d_dinv)
            host.jacobi_inverse(exec_, d_dinv, d_dinv, M)
            for (degree, j), rf in ref.items():
                exec_.copy_from_host(d_b, bs[j][r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist = host.pcg_chebyshev(comm, exec_, A, d_b,
                                             d_x + 8 * GUARD, d_dinv, degree,
                                             LMIN, LMAX, KMAX, RTOL, ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k]))
                assert np.all(ks == k), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX
                _vs_ref(k, hist, xs, rf, norm_a, (world, sym, cm, degree, j))
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)


# ---- 7. lambda_max_estimate ----------------------------------------------------------------
@pytest.mark.parametrize("scaled", MATS)
@pytest.mark.parametrize("n", [8, 11])
def test_lambda_max_estimate(exec_, comm, n, scaled):  # noqa: F811
    csr = tp._csr(f"poisson{n}")
    if scaled:
        csr = tp._scaled(csr)
    rp, ci, va = csr
    N = len(rp) - 1
    diag = tp._diag_of(csr)
    dense = np.zeros((N, N))
    dense[tp._row_of(rp), ci] = va
    s = 1.0 / np.sqrt(diag)
    lam = float(np.linalg.eigvalsh(dense * np.outer(s, s))[-1])
    v0 = oracle.csr_spmv(rp, ci, va,
                         np.random.default_rng(N + 1).uniform(-1, 1, N))
    want = _lambda_ref(lambda v: oracle.csr_spmv(rp, ci, va, v), oracle.ddot,
                       1.0 / diag, v0, 20)
    d_v0, d_dinv = exec_.alloc(N + 2 * GUARD), exec_.alloc(N)
    exec_.copy_from_host(d_dinv, 1.0 / diag)
    buf = np.full(N + 2 * GUARD, SENTINEL)
    buf[GUARD:GUARD + N] = v0
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        exec_.copy_from_host(d_v0, buf)
        got = host.lambda_max_estimate(comm, exec_, A, d_dinv, d_v0 + 8 * GUARD,
                                       20)
        print(n, scaled, sym, "estimate", got, "restatement", want, "lambda",
              lam, "ratio", got / lam)
        assert 0.9 * lam <= got <= lam * (1 + 1e-10)
        assert abs(got - want) <= 1e-10 * abs(want)
        assert np.array_equal(exec_.copy_to_host(d_v0, N + 2 * GUARD), buf)
        with pytest.raises(host.SpmvHostError, match="steps"):
            host.lambda_max_estimate(comm, exec_, A, d_dinv, d_v0 + 8 * GUARD, 0)
        exec_.copy_from_host(d_v0, np.zeros(N + 2 * GUARD))
        with pytest.raises(host.SpmvHostError, match="v0"):
            host.lambda_max_estimate(comm, exec_, A, d_dinv, d_v0 + 8 * GUARD, 20)
        A.close()
    exec_.free(d_v0), exec_.free(d_dinv)
