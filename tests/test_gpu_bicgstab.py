"""spmv::bicgstab (BiCGStab with an optional diagonal right preconditioner).

Shapes as in test_gpu_cg_block.py, for the reasons given at its top: 1 331 rows
(odd; less than one streaming unit of 2 048 doubles), 13 824 rows, 4 097 rows
(odd); both instantiations (cached / non-temporal) of every kernel run through
`blas1_nt_min_elems`.

Matrices (none symmetric):
  convdiff n   the n^3 7-point grid, x fastest, diagonal 7.6; for each axis d
               with c = (0.9, 0.5, 0.2) and neighbours a, b = a + stride_d:
               entry (b, a) = -(1 + c_d)(1 + 0.3 sin b),
               entry (a, b) = -(1 + 0.3 cos a)
  banded n     diagonal 6 + 0.3 sin i, offsets 1, 37, 600:
               entry (a, b = a + d) = -(0.3 + 0.25 sin(a + 2b)),
               entry (b, a) = -(0.5 + 0.4 cos(a + b))
each plain and scaled to S A S with the S of test_gpu_pcg.py.  Right-hand sides
A.1 and A.uniform(-1, 1).  KMAX = 400, RTOL = 1e-10.

The reference is the numpy BiCGStab below, the algorithm of cg.h restated on
oracle.csr_spmv / oracle.ddot (oracle.dist_spmv and a rank-ordered sum for
several ranks).  It is run twice per case, with two summation orders of the dot
product: left to right (oracle.ddot) and chunks of 1 024 summed pairwise, the
chunk sums then in order.  BiCGStab's residual history is more sensitive to
that order than CG's, so the bar on the history is not the project's fixed
1e-6 but comes from the reference's own deviation `dev_ref` between those two
orders, computed here for the very case:
  |k - k_ref| <= 1
  ||x - x_ref|| <= 1e-8 ||x_ref||
  history over min(k, k_ref, 50) entries within max(1e-9, 10 * dev_ref) -- the
      factor 10 because the GPU's order is a third one; a case whose dev_ref
      exceeds 1e-5 FAILS instead of widening the bar
  ||b - A x|| / ||b|| <= 10 * max(rtol, the same of x_ref), by oracle.csr_spmv

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
KMAX, RTOL = 400, 1e-10
GUARD = 2  # doubles in front of an aligned X (16 bytes)


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


# ---- matrices -------------------------------------------------------------------
def _to_csr(n, rows, cols, vals):
    rows, cols, vals = map(np.concatenate, (rows, cols, vals))
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), cols[order].astype(np.int32),
            vals[order].astype(np.float64))


def _convdiff(n):
    N = n ** 3
    idx = np.arange(N)
    coord = (idx % n, (idx // n) % n, idx // (n * n))
    rows, cols, vals = [idx], [idx], [np.full(N, 7.6)]
    for d, c in enumerate((0.9, 0.5, 0.2)):
        a = idx[coord[d] < n - 1]
        b = a + n ** d
        rows += [b, a]
        cols += [a, b]
        vals += [-(1 + c) * (1 + 0.3 * np.sin(b.astype(np.float64))),
                 -(1 + 0.3 * np.cos(a.astype(np.float64)))]
    return _to_csr(N, rows, cols, vals)


def _banded(n):
    i = np.arange(n)
    rows, cols, vals = [i], [i], [6.0 + 0.3 * np.sin(i)]
    for d in (1, 37, 600):
        a, b = i[:-d], i[:-d] + d
        rows += [a, b]
        cols += [b, a]
        vals += [-(0.3 + 0.25 * np.sin((a + 2 * b).astype(np.float64))),
                 -(0.5 + 0.4 * np.cos((a + b).astype(np.float64)))]
    return _to_csr(n, rows, cols, vals)


def _csr(name):
    if name.startswith("convdiff"):
        return _convdiff(int(name[8:]))
    if name.startswith("banded"):
        return _banded(int(name[6:].rstrip("n")))
    rp, ci, va = poisson.poisson3d_csr(int(name[7:]))
    return (np.asarray(rp).astype(np.int32), np.asarray(ci).astype(np.int32),
            np.asarray(va, dtype=np.float64))


def _row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _scaled(csr):
    """S A S, the S of test_gpu_pcg.py"""
    rp, ci, va = csr
    N = len(rp) - 1
    s = 10.0 ** np.random.default_rng(N).uniform(-1, 1, N)
    return rp, ci, va * (s[_row_of(rp)] * s[ci])


def _diag_of(csr):
    rp, ci, va = csr
    rows = _row_of(rp)
    d = np.zeros(len(rp) - 1)
    on = ci == rows
    d[rows[on]] = va[on]
    return d


# ---- the reference: BiCGStab of cg.h in numpy ---------------------------------
def _bicgstab_ref(spmv, dot, b, dinv, kmax, rtol):
    """-> (x, k, history of ||r_j||, status); spmv(q) = A q, dot = the global
    dot product, dinv = None or the inverse diagonal"""
    x = np.zeros(len(b))
    r = np.array(b, dtype=np.float64)
    rhat, p = r.copy(), r.copy()
    rho = rr0 = dot(r, r)
    hist = [math.sqrt(rr0)]
    k = status = 0
    if rr0 == 0.0:
        return x, 0, np.array(hist), 0
    while k < kmax:
        ph = p if dinv is None else dinv * p
        v = spmv(ph)
        rv = dot(rhat, v)
        if rv == 0.0:
            status = 1
            break
        alpha = rho / rv
        s = r - alpha * v
        sh = s if dinv is None else dinv * s
        t = spmv(sh)
        ts, tt = dot(t, s), dot(t, t)
        omega = 0.0 if tt == 0.0 else ts / tt
        x = x + alpha * ph
        x = x + omega * sh
        r = s - omega * t
        rr, rho_new = dot(r, r), dot(rhat, r)
        k += 1
        hist.append(math.sqrt(rr))
        if math.sqrt(rr) / math.sqrt(rr0) < rtol:
            break
        if omega == 0.0 or rho_new == 0.0:
            status = 2
            break
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
    return x, k, np.array(hist), status


def _dot_chunked(a, b):
    """the second summation order: chunks of 1 024 products summed pairwise,
    the chunk sums then left to right"""
    prod = np.asarray(a) * np.asarray(b)
    pad = (-len(prod)) % 1024
    v = np.concatenate([prod, np.zeros(pad)]).reshape(-1, 1024)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    s = 0.0
    for c in v[:, 0]:
        s += float(c)
    return s


class _Ref:
    """The reference of one case, in both summation orders, and its own
    deviation between them."""

    def __init__(self, spmv, dot, b, dinv, kmax=KMAX, rtol=RTOL):
        self.x, self.k, self.hist, self.status = _bicgstab_ref(
            spmv, dot, b, dinv, kmax, rtol)
        self.second = _bicgstab_ref(spmv, _dot_chunked, b, dinv, kmax, rtol)
        self.b = b
        self.true_res = (np.linalg.norm(b - spmv(self.x)) / np.linalg.norm(b))

    def dev(self, m):
        """relative deviation of the two histories over their first m entries"""
        m = min(m, self.second[1])
        if m == 0:
            return 0.0
        return float(np.abs(self.second[2][:m] / self.hist[:m] - 1).max())


def _vs_ref(k, hist, x, status, ref, spmv, what, kmax=KMAX, rtol=RTOL):
    """Every figure is printed before anything is asserted; the bars that do
    not rest on dev_ref come first."""
    m = min(k, ref.k, 50)
    dev_ref = ref.dev(m)
    dev = float(np.abs(hist[:m] / ref.hist[:m] - 1).max()) if m else 0.0
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res = np.linalg.norm(ref.b - spmv(x)) / np.linalg.norm(ref.b)
    print(what, "k", k, "k_ref", ref.k, "k_ref (second order)", ref.second[1],
          "status", status, "history deviation", dev, "dev_ref", dev_ref,
          "x error", err, "true residual", res, "of the reference",
          ref.true_res)
    assert status == ref.status == 0, (what, status, ref.status)
    assert abs(k - ref.k) <= 1, (what, k, ref.k)
    assert len(hist) == k + 1, what
    if 0 < k < kmax:
        assert hist[k] / hist[0] < rtol, what
    assert err <= 1e-8, (what, err)
    assert res <= 10 * max(rtol, ref.true_res), (what, res, ref.true_res)
    assert dev_ref <= 1e-5, (what, "the reference disagrees with itself", dev_ref)
    assert dev <= max(1e-9, 10 * dev_ref), (what, dev, dev_ref)


class _Problem:
    """One shape: the matrix plain and scaled (general storage), the Jacobi
    dinv of both on the device (Matrix::diagonal + jacobi_inverse), right-hand
    sides and references (computed once, never changed)."""

    def __init__(self, exec_, comm, name):
        self.name, self.exec_ = name, exec_
        plain = _csr(name)
        self.csr = {"plain": plain, "sas": _scaled(plain)}
        self.N = N = len(plain[0]) - 1
        rng = np.random.default_rng(N + 1)
        u = rng.uniform(-1, 1, N)
        self.rhs, self.A, self.d_dinv, self.diag = {}, {}, {}, {}
        for var, csr in self.csr.items():
            self.rhs[var] = {"ones": oracle.csr_spmv(*csr, np.ones(N)),
                             "rand": oracle.csr_spmv(*csr, u),
                             "zero": np.zeros(N)}
            self.diag[var] = _diag_of(csr)
            self.A[var] = host.Matrix.create_matrix(
                comm, exec_, *csr, N, N, [], [], False, host.P2P_NONBLOCKING)
            self.d_dinv[var] = exec_.alloc(N + 1)
            self.A[var].diagonal(self.d_dinv[var])
            host.jacobi_inverse(exec_, self.d_dinv[var], self.d_dinv[var], N)
        self.d_b = exec_.alloc(N)
        self.d_x = exec_.alloc(N + 2 * GUARD)
        self.ws = host.BicgstabWorkspace(exec_)
        self._ref = {}

    def spmv(self, var):
        return lambda q: oracle.csr_spmv(*self.csr[var], q)

    def ref(self, var, rhs, jacobi=True):
        key = (var, rhs, jacobi)
        if key not in self._ref:
            self._ref[key] = _Ref(self.spmv(var), oracle.ddot,
                                  self.rhs[var][rhs],
                                  1.0 / self.diag[var] if jacobi else None)
        return self._ref[key]

    def solve(self, comm, var, rhs, jacobi=True, kmax=KMAX, rtol=RTOL, ws=None,
              x_off=GUARD, A=None, d_dinv=None, b=None, **kw):
        """-> (k, history, x, status); x_off in doubles from the 256-byte
        aligned buffer (GUARD: aligned, GUARD + 1: 8 bytes off)"""
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_b, self.rhs[var][rhs] if b is None else b)
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        d_x = self.d_x + 8 * x_off
        if d_dinv is None and jacobi:
            d_dinv = self.d_dinv[var]
        k, hist, status = host.bicgstab(comm, e, A or self.A[var], self.d_b, d_x,
                                        d_dinv, kmax, rtol, ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD)
        x = buf[x_off:x_off + N].copy()
        assert np.all(buf[:x_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[x_off + N:] == SENTINEL), (self.name, "guard behind")
        assert np.all(np.isfinite(x)) and not np.any(x == SENTINEL), self.name
        assert np.all(np.isfinite(hist)), self.name
        return k, hist.copy(), x, status

    def close(self):
        self.ws.close()
        for A in self.A.values():
            A.close()
        for p in list(self.d_dinv.values()) + [self.d_b, self.d_x]:
            self.exec_.free(p)


SHAPES = ("convdiff11", "convdiff24", "banded4097n")


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


# ---- 1. against the reference -------------------------------------------------
@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("var", ["plain", "sas"])
@pytest.mark.parametrize("shape", SHAPES)
def test_jacobi_against_the_reference(comm, problems, nt, shape, var, rhs):
    P = problems[shape]
    ref = P.ref(var, rhs)
    k, hist, x, status = P.solve(comm, var, rhs)
    assert k < KMAX
    _vs_ref(k, hist, x, status, ref, P.spmv(var), (shape, var, rhs, "jacobi"))


@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("shape", SHAPES)
def test_unpreconditioned_against_the_reference(comm, problems, nt, shape, rhs):
    P = problems[shape]
    ref = P.ref("plain", rhs, jacobi=False)
    k, hist, x, status = P.solve(comm, "plain", rhs, jacobi=False)
    assert k < KMAX
    _vs_ref(k, hist, x, status, ref, P.spmv("plain"), (shape, rhs, "no dinv"))


@pytest.mark.parametrize("rhs", ["ones", "rand"])
@pytest.mark.parametrize("shape", SHAPES)
def test_what_the_preconditioner_is_for(problems, shape, rhs):
    """A relation between two references on S A S: with the Jacobi dinv the
    solve stops below 400 iterations, without it it has not at 400."""
    P = problems[shape]
    ref = P.ref("sas", rhs)
    _, k_plain, hist_plain, _ = _bicgstab_ref(P.spmv("sas"), oracle.ddot,
                                              P.rhs["sas"][rhs], None, KMAX,
                                              RTOL)
    print(shape, rhs, "k_ref jacobi", ref.k, "k_ref without", k_plain)
    assert ref.k < KMAX and ref.status == 0
    assert k_plain == KMAX and not hist_plain[-1] / hist_plain[0] < RTOL


# ---- 2. dinv = 1 has the bits of dinv = None ----------------------------------
def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2], b[2]), what
    assert a[3] == b[3], (what, a[3], b[3])


@pytest.mark.parametrize("shape", SHAPES)
def test_unit_dinv_has_the_bits_of_no_dinv(exec_, comm, problems, nt, shape):
    P = problems[shape]
    d_one = exec_.alloc(P.N)
    exec_.copy_from_host(d_one, np.ones(P.N))
    for kw in ({}, {"consumer_reductions": False}):
        want = P.solve(comm, "plain", "rand", jacobi=False, **kw)
        assert 1 < want[0] < KMAX
        got = P.solve(comm, "plain", "rand", d_dinv=d_one, **kw)
        _same(want, got, (shape, kw, "dinv = 1"))
    exec_.free(d_one)


# ---- 3. the paths agree bit for bit on one rank -------------------------------
@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "nodinv"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reducer_and_consumer_paths_and_unaligned_x(comm, problems, nt, shape,
                                                    jacobi):
    P = problems[shape]
    var = "sas" if jacobi else "plain"
    for kmax in (KMAX, 9):
        want = P.solve(comm, var, "rand", jacobi=jacobi, kmax=kmax)
        assert want[0] > 1
        got = P.solve(comm, var, "rand", jacobi=jacobi, kmax=kmax,
                      consumer_reductions=False)
        _same(want, got, (shape, jacobi, kmax, "reducer kernels"))
        got = P.solve(comm, var, "rand", jacobi=jacobi, kmax=kmax,
                      x_off=GUARD + 1)  # X + 8 bytes
        _same(want, got, (shape, jacobi, kmax, "unaligned x"))


@pytest.mark.parametrize("shape", SHAPES)
def test_unaligned_dinv_keeps_the_bits(exec_, comm, problems, nt, shape):
    P = problems[shape]
    d = exec_.alloc(P.N + 1)
    exec_.copy(d + 8, P.d_dinv["sas"], P.N * 8)
    for kmax in (KMAX, 9):
        want = P.solve(comm, "sas", "rand", kmax=kmax)
        got = P.solve(comm, "sas", "rand", kmax=kmax, d_dinv=d + 8)
        _same(want, got, (shape, kmax, "unaligned dinv"))
    exec_.free(d)


# ---- 4. workspace reuse ----------------------------------------------------------
def test_workspace_reused_and_grown(comm, problems, nt):
    """One workspace across shapes (small, large, middle), with and without a
    dinv, and across a smaller kmax: every result equals the one on a fresh
    workspace, bit for bit."""
    e = problems["convdiff11"].exec_
    shared = host.BicgstabWorkspace(e)
    plan = [("convdiff11", 30, GUARD, False), ("convdiff24", 40, GUARD + 1, True),
            ("banded4097n", 12, GUARD, True), ("convdiff24", 7, GUARD, False),
            ("convdiff11", 40, GUARD + 1, True), ("convdiff11", 0, GUARD, True)]
    for shape, kmax, x_off, jacobi in plan:
        P = problems[shape]
        fresh = host.BicgstabWorkspace(e)
        want = P.solve(comm, "plain", "rand", jacobi=jacobi, kmax=kmax,
                       rtol=1e-6, ws=fresh, x_off=x_off)
        fresh.close()
        got = P.solve(comm, "plain", "rand", jacobi=jacobi, kmax=kmax, rtol=1e-6,
                      ws=shared, x_off=x_off)
        _same(want, got, (shape, kmax, x_off, jacobi))
    shared.close()


# ---- 5. rtol = 0 ----------------------------------------------------------------
@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "nodinv"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_number_of_iterations(comm, problems, nt, shape, jacobi):
    P = problems[shape]
    for kmax in (0, 1, 2, 7):
        for kw in ({}, {"consumer_reductions": False}):
            k, hist, x, status = P.solve(comm, "plain", "ones", jacobi=jacobi,
                                         kmax=kmax, rtol=0.0, **kw)
            what = (shape, jacobi, kmax, kw)
            assert k == kmax and status == 0, what
            assert hist.shape == (kmax + 1,) and np.all(hist > 0.0), what
            assert np.any(x != 0.0) == (kmax > 0), what
            # b = 0: stopped at k = 0 with x = 0, nothing undefined
            k, hist, x, status = P.solve(comm, "plain", "zero", jacobi=jacobi,
                                         kmax=kmax, rtol=0.0, **kw)
            assert k == 0 and status == 0 and np.all(x == 0.0), what
            assert hist.shape == (1,) and hist[0] == 0.0, what


# ---- 6. frozen after convergence -------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_after_convergence(comm, problems, nt, shape):
    """poll_every = 255 and kmax far beyond the stop: every iteration is
    enqueued, so every kernel launched after `done` had the chance to touch x;
    poll_every = 1: the host stops enqueuing early."""
    P = problems[shape]
    for kw in ({}, {"consumer_reductions": False}):
        want = P.solve(comm, "sas", "rand", **kw)
        k = want[0]
        assert 1 < k and k + 80 < 255 and want[3] == 0
        for poll in (255, 1):
            got = P.solve(comm, "sas", "rand", kmax=k + 80, poll_every=poll, **kw)
            _same(want, got, (shape, kw, poll))
        got = P.solve(comm, "sas", "rand", kmax=k, **kw)
        _same(want, got, (shape, kw, "kmax = k"))


# ---- 7. breakdown 1 ----------------------------------------------------------------
def test_breakdown_1_on_the_cyclic_shift(exec_, comm, nt):
    """A = the cyclic shift (row i has the single entry (i, (i + 1) mod N) = 1),
    b = e_0: v = A b = e_(N-1), so rhat . v == 0 exactly.  The solver returns 0
    with status 1; x = 0 (iteration 1 wrote nothing), the history is [1.0]."""
    N = 1331
    rp = np.arange(N + 1, dtype=np.int32)
    ci = ((np.arange(N) + 1) % N).astype(np.int32)
    va = np.ones(N)
    b = np.zeros(N)
    b[0] = 1.0
    ref = _bicgstab_ref(lambda q: oracle.csr_spmv(rp, ci, va, q), oracle.ddot, b,
                        None, KMAX, RTOL)
    assert ref[1] == 0 and ref[3] == 1 and np.all(ref[0] == 0.0)
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [], False,
                                  host.P2P_NONBLOCKING)
    d_b, d_x = exec_.alloc(N), exec_.alloc(N + 2 * GUARD)
    d_one = exec_.alloc(N)
    exec_.copy_from_host(d_b, b)
    exec_.copy_from_host(d_one, np.ones(N))
    for dinv in (None, d_one):
        for kw in ({}, {"consumer_reductions": False}, {"poll_every": 255}):
            for x_off in (GUARD, GUARD + 1):
                exec_.copy_from_host(d_x, np.full(N + 2 * GUARD, SENTINEL))
                k, hist, status = host.bicgstab(comm, exec_, A, d_b,
                                                d_x + 8 * x_off, dinv, KMAX,
                                                RTOL, **kw)
                buf = exec_.copy_to_host(d_x, N + 2 * GUARD)
                what = (dinv is not None, kw, x_off)
                assert (k, status) == (0, 1), what
                assert np.array_equal(hist, [1.0]), what
                assert np.all(buf[x_off:x_off + N] == 0.0), what
                assert np.all(buf[:x_off] == SENTINEL), what
                assert np.all(buf[x_off + N:] == SENTINEL), what
    A.close()
    for p in (d_b, d_x, d_one):
        exec_.free(p)


# ---- 8. symmetric storage ----------------------------------------------------------
def test_symmetric_storage(exec_, comm, nt):
    """The scaled Poisson matrix of test_gpu_pcg.py in symmetric storage with
    the Jacobi dinv, both right-hand sides: the solver does not care how the
    matrix is stored.  Same reference, same bars.

    The size is 8^3, the one test_gpu_pcg.py uses for its slab tests.  A case
    is only a case while its reference agrees with itself (dev_ref <= 1e-5, see
    the top of the file), and of the three sizes of that file only this one
    does.  Measured on the CPU, k in both summation orders and dev_ref over
    min(k, 50) entries, A.1 / A.uniform:
      poisson8    25, 25, 2.2e-7   /  25, 25, 1.1e-7
      poisson11   35, 36, 3.7      /  35, 35, 9.3e-4
      poisson24   71, 71, 0.79     /  70, 70, 0.25
    The streaming shapes (odd sizes, more than one unit) are covered by the
    tests above; what this one adds is the SpMV of the other storage."""
    csr = _scaled(_csr("poisson8"))
    N = len(csr[0]) - 1
    spmv = lambda q: oracle.csr_spmv(*csr, q)  # noqa: E731
    A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], True,
                                  host.P2P_NONBLOCKING)
    d_b, d_x, d_dinv = exec_.alloc(N), exec_.alloc(N + 2 * GUARD), exec_.alloc(N)
    A.diagonal(d_dinv)
    host.jacobi_inverse(exec_, d_dinv, d_dinv, N)
    u = np.random.default_rng(N + 1).uniform(-1, 1, N)
    for rhs, b in (("ones", spmv(np.ones(N))), ("rand", spmv(u))):
        if (N, rhs) not in _SYM_REFS:
            _SYM_REFS[(N, rhs)] = _Ref(spmv, oracle.ddot, b,
                                       1.0 / _diag_of(csr))
        exec_.copy_from_host(d_b, b)
        exec_.copy_from_host(d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist, status = host.bicgstab(comm, exec_, A, d_b, d_x + 8 * GUARD,
                                        d_dinv, KMAX, RTOL)
        buf = exec_.copy_to_host(d_x, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL), rhs
        assert np.all(buf[GUARD + N:] == SENTINEL), rhs
        assert k < KMAX
        _vs_ref(k, hist, buf[GUARD:GUARD + N], status, _SYM_REFS[(N, rhs)], spmv,
                ("symmetric storage", rhs))
    A.close()
    for p in (d_b, d_x, d_dinv):
        exec_.free(p)


_SYM_REFS = {}  # computed once, shared by both instantiations


# ---- 9. errors ---------------------------------------------------------------------
def _current_stream(exec_):
    s = C.c_void_p()
    _lib.call("spmv_hip_get_stream", exec_.context, C.byref(s))
    return s.value


def test_errors_leave_the_executor_as_it_was(comm, problems):
    P = problems["convdiff11"]
    e, A, N = P.exec_, P.A["plain"], P.N
    dinv = P.d_dinv["plain"]
    mine = C.c_void_p()
    _lib.call("spmv_hip_stream_create", e.context, C.byref(mine))
    _lib.call("spmv_hip_set_stream", e.context, mine)
    try:
        e.copy_from_host(P.d_b, P.rhs["plain"]["ones"])
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.bicgstab(comm, e, A, P.d_b, P.d_b, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.bicgstab(comm, e, A, P.d_b, P.d_b + 8 * (N - 1), dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.bicgstab(comm, e, A, P.d_b, P.d_b, None, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.bicgstab(comm, e, A, P.d_b, dinv, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="overlaps"):
            host.bicgstab(comm, e, A, P.d_b, dinv + 8, dinv, 5, 1e-10)
        with pytest.raises(host.SpmvHostError, match="kmax"):
            host.bicgstab(comm, e, A, P.d_b, P.d_x, dinv, -1, 1e-10)
        assert _current_stream(e) == mine.value
        # dinv and b are as they were
        assert np.array_equal(e.copy_to_host(dinv, N), 1.0 / P.diag["plain"])
        assert np.array_equal(e.copy_to_host(P.d_b, N), P.rhs["plain"]["ones"])
        # ... and after a solve that went through
        k, _, status = host.bicgstab(comm, e, A, P.d_b, P.d_x, dinv, 3, 0.0, P.ws)
        assert (k, status) == (3, 0)
        assert _current_stream(e) == mine.value
    finally:
        _lib.call("spmv_hip_set_stream", e.context, None)
        e.synchronize()
        _lib.call("spmv_hip_stream_destroy", e.context, mine)


# ---- 10. ABI -----------------------------------------------------------------------
def test_abi_refuses_short_destinations_and_bad_iterations(exec_):
    """spmv_hip_bicg_ws_read_async copies nothing into a buffer that is too
    short; slots and kernels refuse an iteration outside their range."""
    h, ctx = _lib.hip, exec_.context
    ws = C.c_void_p()
    _lib.call("spmv_hip_bicg_ws_create", ctx, 5, C.byref(ws))
    try:
        kmax = C.c_int()
        _lib.call("spmv_hip_bicg_ws_capacity", ws, C.byref(kmax))
        assert kmax.value == 5
        flags = np.full(3, 99, np.int32)
        rrho = np.full(12, -7.0)
        fp, zp = flags.ctypes.data_as(C.c_void_p), rrho.ctypes.data_as(C.c_void_p)
        assert h.spmv_hip_bicg_ws_read_async(ws, fp, zp, 11, None) == -1
        assert h.spmv_hip_bicg_ws_read_async(ws, None, zp, 6, None) == -1
        assert h.spmv_hip_bicg_ws_read_async(ws, fp, zp, 0, None) == -1
        exec_.synchronize()
        assert np.all(flags == 99) and np.all(rrho == -7.0)
        _lib.call("spmv_hip_bicg_ws_reset", ws, 1e-8, None)
        _lib.call("spmv_hip_bicg_ws_read_async", ws, fp, zp, 12, None)
        exec_.synchronize()
        assert list(flags) == [0, -1, 0] and np.all(rrho == 0.0)
        # the pairs are adjacent: slot k + 1 is 16 bytes further
        s0, s1, slot = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for get in ("spmv_hip_bicg_ws_ts_tt", "spmv_hip_bicg_ws_rr_rho"):
            _lib.call(get, ws, 0, C.byref(s0))
            _lib.call(get, ws, 1, C.byref(s1))
            assert s1.value - s0.value == 16, get
        for get in (h.spmv_hip_bicg_ws_rv, h.spmv_hip_bicg_ws_ts_tt,
                    h.spmv_hip_bicg_ws_rr_rho):
            assert get(ws, 6, C.byref(slot)) == -1
            assert get(ws, -1, C.byref(slot)) == -1
        assert h.spmv_hip_bicg_reduce_rr_rho(ctx, ws, 6, None) == -1
        assert h.spmv_hip_bicg_reduce_rr_rho(ctx, ws, -1, None) == -1
        for k in (0, 6):
            assert h.spmv_hip_bicg_reduce_rv(ctx, ws, k, None) == -1
            assert h.spmv_hip_bicg_reduce_ts_tt(ctx, ws, k, None) == -1
            assert h.spmv_hip_bicg_dot_rv_f64(ctx, ws, k, 4, s0, s0, None) == -1
            assert h.spmv_hip_bicg_dot_ts_tt_f64(ctx, ws, k, 4, s0, s0,
                                                 None) == -1
            for form in ("_f64", "_cs_f64"):
                for name in ("spmv_hip_bicg_update_s", "spmv_hip_bicg_update_p"):
                    assert getattr(h, name + form)(ctx, ws, k, 4, s0, s0, s0, s0,
                                                   s0, None) == -1
                assert getattr(h, "spmv_hip_bicg_update_xr" + form)(
                    ctx, ws, k, 4, s0, s0, s0, s0, s0, s0, s0, None) == -1
        exec_.synchronize()
        _lib.call("spmv_hip_bicg_ws_read_async", ws, fp, zp, 12, None)
        exec_.synchronize()
        assert list(flags) == [0, -1, 0] and np.all(rrho == 0.0)  # nothing ran
    finally:
        exec_.synchronize()
        _lib.call("spmv_hip_bicg_ws_destroy", ws)


# ---- 11. several ranks -----------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded_bicgstab(world):
    """Ranks as threads (tests/thread_world.py), convdiff8 in slabs, plain and
    S A S with the Jacobi dinv, general storage, a blocking and an overlapping
    halo model, ONE workspace per rank over all solves; against the numpy
    reference on oracle.dist_spmv with the rank-ordered dot product."""
    from thread_world import ThreadWorld
    plain = _csr("convdiff8")
    N = len(plain[0]) - 1
    csrs = {"plain": plain, "sas": _scaled(plain)}
    rng = np.random.default_rng(world)
    u = rng.uniform(-1, 1, N)
    ranges = oracle.owner_ranges(world, N)
    models = (host.P2P_BLOCKING, host.P2P_NONBLOCKING)

    def dist_dot(a, b):
        s = 0.0
        for r in range(world):
            s += oracle.ddot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
        return s

    cases = {}
    for var, (rp, ci, va) in csrs.items():
        bs = [oracle.csr_spmv(rp, ci, va, np.ones(N)),
              oracle.csr_spmv(rp, ci, va, u)]
        for cm in models:
            def spmv(q, rp=rp, ci=ci, va=va, cm=cm):
                return oracle.dist_spmv(world, rp, ci, va, q, False, cm)
            cases[(var, cm)] = (spmv, bs, [
                _Ref(spmv, dist_dot, b, 1.0 / _diag_of((rp, ci, va)))
                for b in bs])
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        ws = host.BicgstabWorkspace(exec_)
        d_b, d_dinv = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        for (var, cm), (spmv, bs, refs) in cases.items():
            lrp, lci, lva, gh = oracle.localise_rows(*csrs[var], r0, r1)
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            A.diagonal(d_dinv)
            host.jacobi_inverse(exec_, d_dinv, d_dinv, M)
            for j, b in enumerate(bs):
                exec_.copy_from_host(d_b, b[r0:r1])
                exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
                k, hist, status = host.bicgstab(comm, exec_, A, d_b,
                                                d_x + 8 * GUARD, d_dinv, KMAX,
                                                RTOL, ws)
                buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
                assert np.all(buf[:GUARD] == SENTINEL)
                assert np.all(buf[GUARD + M:] == SENTINEL)
                ks = tw.gather(rank, np.array([k, status]))
                assert np.all(ks.reshape(-1, 2) == [k, status]), ks
                xs = tw.gather(rank, buf[GUARD:GUARD + M])
                assert k < KMAX
                _vs_ref(k, hist, xs, status, refs[j], spmv, (world, var, cm, j))
            A.close()
        for p in (d_b, d_dinv, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
