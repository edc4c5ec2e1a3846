"""spmv::lobpcg with B: whole solves on one rank (and two slab ranks as threads).

B = I stored as a CSR matrix returns the bits of lobpcg() without B: BX goes
through the arithmetic of X (0.0 + 1.0 * x is x).  On general storage of A and
B the count, the Ritz values, the history, X and the true residuals equal
lobpcg_gen_cases.lobpcg_gen_ref bit for bit, with every preconditioner.
Symmetric storage of A and / or B and two ranks are held to the theorem of
lobpcg_gen_cases.theorem_check_gen, because oracle.csr_spmv adds a row in
another order than symmetric storage and the Gram sums cross ranks in another
order; there rtol 1e-6 and kmax 300 come from the restatement's own runs
(lobpcg_gen_cases.K_GEN: 98 and 83 iterations on one rank, 58 on mass8)."""
import numpy as np
import pytest

import ilu0_cases as ic
import lobpcg_cases as lc
import lobpcg_gen_cases as lg
import oracle
import test_gpu_amg as ta
import test_gpu_sgs as ts
from spmv_amd import host
from test_gpu_lobpcg_kernels import same_values
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -777.25, 4


def _matrix(comm, exec_, csr, sym=False, ghosts=()):  # noqa: F811
    n = len(csr[0]) - 1
    return host.Matrix.create_matrix(comm, exec_, *csr, n, n, [], list(ghosts),
                                     sym, host.P2P_NONBLOCKING)


class _Problem:
    def __init__(self, exec_, comm, name):  # noqa: F811
        self.exec_, self.comm, self.name = exec_, comm, name
        self.pencil = P = lg.pencil(name)
        self.N = N = P.N
        self.A = {sym: _matrix(comm, exec_, P.A, sym) for sym in (False, True)}
        self.B = {sym: _matrix(comm, exec_, P.B, sym) for sym in (False, True)}
        self.d_dinv = exec_.alloc(N + 1)
        exec_.copy_from_host(self.d_dinv, P.dinv())
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD + 1)
        self.ws = host.LobpcgWorkspace(exec_)
        self.M, self._pre_ref = {}, {}

    def pre(self, kind):
        if kind == "none":
            return {}
        if kind == "dinv":
            return dict(dinv=self.d_dinv)
        if kind not in self.M:
            A = self.A[False]
            self.M[kind] = (
                host.SgsPreconditioner(self.exec_, A) if kind == "sgs" else
                host.Ilu0Preconditioner(self.exec_, A) if kind == "ilu0" else
                host.AmgPreconditioner(self.exec_, A))
        return dict(amg=self.M[kind]) if kind == "amg" else dict(sgs=self.M[kind])

    def precond_ref(self, kind):
        """r -> M^-1 r restated for general storage of A (made once), or None"""
        if kind in ("none", "dinv"):
            return None
        if kind not in self._pre_ref:
            csr, N = self.pencil.A, self.N
            if kind == "amg":
                self.pre(kind)
                self._pre_ref[kind] = ta.restate(csr, N, False).apply
            else:
                colours = self.pre(kind)["sgs"].colors()
                if kind == "sgs":
                    sw = ts.Sweeps(csr, N, colours, False)
                    dinv = 1.0 / self.pencil.diag
                    self._pre_ref[kind] = lambda r: sw.apply(dinv, r)
                else:
                    ref = ic.Ilu0Ref(csr, N, colours, False)
                    fac = ref.factor()
                    self._pre_ref[kind] = lambda r: ref.apply(fac, r)
        return self._pre_ref[kind]

    def solve(self, X0, kmax, rtol, kind="none", sym_a=False, sym_b=False,
              ws=None, x_off=GUARD, atol=0.0, B="own", **kw):
        e, N = self.exec_, self.N
        nev = X0.shape[1]
        size = N * 8 + 2 * GUARD + 1
        buf = np.full(size, SENTINEL)
        buf[x_off:x_off + N * nev] = X0.ravel()
        e.copy_from_host(self.d_x, buf)
        stats = {}
        k, theta, hist, status = host.lobpcg(
            self.comm, e, self.A[sym_a], self.d_x + 8 * x_off, nev, kmax, rtol,
            atol, workspace=ws or self.ws, stats=stats,
            B=self.B[sym_b] if isinstance(B, str) else B, **self.pre(kind), **kw)
        out = e.copy_to_host(self.d_x, size)
        lo, hi = x_off, x_off + N * nev
        assert np.all(out[:lo] == SENTINEL) and np.all(out[hi:] == SENTINEL)
        return (k, theta.copy(), hist.copy(), status,
                out[lo:hi].reshape(N, nev).copy(), stats)

    def close(self):
        self.ws.close()
        for M in self.M.values():
            M.close()
        for A in list(self.A.values()) + list(self.B.values()):
            A.close()
        self.exec_.free(self.d_dinv)
        self.exec_.free(self.d_x)


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


def _same(a, b, what):
    """two device solves: no tolerance"""
    assert (a[0], a[3]) == (b[0], b[3]), (what, a[0], a[3], b[0], b[3])
    for i in (1, 2, 4):
        assert same_values(a[i], b[i]), (what, i)
    assert same_values(a[5]["true_resnorm"], b[5]["true_resnorm"]), what
    assert a[5]["restarts"] == b[5]["restarts"], what


def _same_as_ref(got, ref, what):
    k, theta, hist, status, X, stats = got
    assert (k, status) == (ref["k"], ref["status"]), (what, k, status, ref["k"])
    assert same_values(theta, ref["theta"]), what
    assert same_values(hist, ref["hist"]), what
    assert same_values(X, ref["X"]), what
    assert same_values(stats["true_resnorm"], ref["true_resnorm"]), what
    assert stats["restarts"] == ref["restarts"], what


# ---- 1. B = I: the bits of the solve without B ---------------------------------------
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("kind", ["none", "dinv", "sgs", "amg"])
@pytest.mark.parametrize("nev", [4, 8])
def test_identity_b_is_the_standard_solve(problems, nt, nev, kind, largest):  # noqa: F811
    P = problems("identity11")
    X0 = lc.x0(P.N, nev, 1)
    std = P.solve(X0, 14, 1e-2, kind, B=None, largest=largest)
    gen = P.solve(X0, 14, 1e-2, kind, largest=largest)
    assert std[0] > 0
    _same(gen, std, (nev, kind, largest))
    gen = P.solve(X0, 14, 1e-2, kind, largest=largest, x_off=GUARD + 1)
    _same(gen, std, (nev, kind, largest, "offset"))


# ---- 2. three pencils, bit for bit against the restatement --------------------------
@pytest.mark.parametrize("kind", ["none", "dinv", "sgs", "ilu0", "amg"])
@pytest.mark.parametrize("name,nev", [("tri200", 3), ("lumped11", 4),
                                      ("mass11", 4), ("mass11", 8)])
def test_bits_on_the_pencils(problems, nt, name, nev, kind):  # noqa: F811
    """rtol 1e-2 and kmax 12: where columns meet their test within kmax (the
    Poisson pencils behind SGS, ILU(0), AMG) soft locking and the frozen P, AP,
    BP are in the compared bits"""
    P = problems(name)
    X0 = lc.x0(P.N, nev, 1)
    ref = P.pencil.ref(X0, 12, 1e-2, kind, precond=P.precond_ref(kind))
    for poll in (0, 1):
        got = P.solve(X0, 12, 1e-2, kind, poll_every=poll)
        _same_as_ref(got, ref, (name, nev, kind, poll))
    got = P.solve(X0, 12, 1e-2, kind, x_off=GUARD + 1)  # 8 bytes off
    _same_as_ref(got, ref, (name, nev, kind, "offset"))


@pytest.mark.parametrize("name,nev", [("tri200", 2), ("mass11", 3)])
def test_bits_largest_and_other_widths(problems, name, nev):  # noqa: F811
    P = problems(name)
    X0 = lc.x0(P.N, nev, 2)
    for kind in ("none", "dinv"):
        ref = P.pencil.ref(X0, 10, 1e-3, kind, largest=True)
        _same_as_ref(P.solve(X0, 10, 1e-3, kind, largest=True), ref, (name, kind))
    X0 = lc.x0(P.N, 5, 3)  # the run-time width; kmax 0; atol met at once
    _same_as_ref(P.solve(X0, 6, 1e-3), P.pencil.ref(X0, 6, 1e-3), (name, 5))
    _same_as_ref(P.solve(X0, 0, 1e-6), P.pencil.ref(X0, 0, 1e-6), (name, "k0"))
    ref = P.pencil.ref(X0, 6, 0.0, atol=100.0)
    got = P.solve(X0, 6, 0.0, atol=100.0)
    _same_as_ref(got, ref, (name, "atol"))
    assert got[0] == 0


# ---- 3. held to the theorem -----------------------------------------------------------
@pytest.mark.parametrize("name,kind,sym_a,sym_b", [
    ("mass11", "none", True, False), ("mass11", "dinv", False, True),
    ("mass11", "dinv", True, True), ("lumped11", "none", True, True),
    ("lumped11", "dinv", True, False)])
def test_theorem_on_symmetric_storage(problems, name, kind, sym_a, sym_b):  # noqa: F811
    P = problems(name)
    nev, kmax, rtol = 4, lg.KMAX_GEN, 1e-6
    X0 = lc.x0(P.N, nev, 1)
    k, theta, hist, status, X, stats = P.solve(X0, kmax, rtol, kind, sym_a, sym_b)
    print(name, kind, sym_a, sym_b, "k", k, "theta", theta, "true",
          stats["true_resnorm"])
    assert status == 0 and k < kmax
    for c in range(nev):  # every column met its test before kmax
        h = hist[c]
        last = int(np.nonzero(h >= 0.0)[0][-1])
        assert last <= k and h[last] < rtol * abs(theta[c]), (c, last, h[last])
    lg.theorem_check_gen(P.pencil, theta, X, False, (name, kind, sym_a, sym_b))
    Bd, eps = P.pencil.dense()[1], np.finfo(np.float64).eps
    cond_b = P.pencil.eig()[3]  # (the bound: test_lobpcg_gen_host.py)
    assert np.abs(X.T @ Bd @ X - np.eye(nev)).max() <= (
        64 * 3 * nev * cond_b + P.N * np.sqrt(cond_b)) * eps
    # the restatement's count, other summation orders
    assert abs(k - lg.K_GEN[(name, nev, kind, False)]) <= 2, k


# ---- 4. not positive definite, poisons, the workspace ---------------------------------
def test_b_not_positive_definite_nan_and_the_workspace(problems):  # noqa: F811
    P = problems("lumped11")
    e, comm_ = P.exec_, P.comm
    good = lc.x0(P.N, 3, 6)
    ws = host.LobpcgWorkspace(e)
    fresh = host.LobpcgWorkspace(e)
    want_gen = P.solve(good, 8, 1e-3, "dinv", ws=fresh)
    fresh.close()
    fresh = host.LobpcgWorkspace(e)
    want_std = P.solve(good, 8, 1e-3, "dinv", ws=fresh, B=None)
    fresh.close()
    assert not same_values(want_gen[1], want_std[1])
    # one workspace: with B, without, with B again: each solve's own bits
    _same(P.solve(good, 8, 1e-3, "dinv", ws=ws), want_gen, "gen 1")
    _same(P.solve(good, 8, 1e-3, "dinv", ws=ws, B=None), want_std, "std")
    _same(P.solve(good, 8, 1e-3, "dinv", ws=ws), want_gen, "gen 2")
    # one negative diagonal entry of B; column 0 of X0 is the unit vector there,
    # so the first pivot is negative (no other test of definiteness is made)
    bad_x = good.copy()
    bad_x[:, 0] = 0.0
    bad_x[5, 0] = 1.0
    for poison in (-1.0, np.nan):
        rp, ci, va = P.pencil.B
        va = va.copy()
        va[5] = poison
        Bm = _matrix(comm_, e, (rp, ci, va))
        k, theta, hist, status, X, _ = P.solve(bad_x, 8, 1e-3, "dinv", ws=ws, B=Bm)
        assert (k, status) == (0, 1) and np.array_equal(X, bad_x), poison
        assert np.all(hist == -1.0)
        ref = lg.lobpcg_gen_ref(P.pencil.spmv_a,
                                lambda v: oracle.csr_spmv(rp, ci, va, v), None,
                                bad_x, 8, 1e-3, dinv=P.pencil.dinv())
        assert (ref["k"], ref["status"]) == (0, 1)
        if np.isnan(poison):  # any X0 meets the NaN in the first Gram sums
            k, _, _, status, _, _ = P.solve(good, 8, 1e-3, "dinv", ws=ws, B=Bm)
            assert (k, status) == (0, 1)
        Bm.close()
        _same(P.solve(good, 8, 1e-3, "dinv", ws=ws), want_gen, "usable")
    ws.close()


# ---- 5. the rule ------------------------------------------------------------------------
def test_pencil_rule(problems, exec_, comm):  # noqa: F811
    P = problems("lumped11")
    other = _matrix(comm, exec_, lg.identity(200))
    with pytest.raises(host.SpmvHostError, match="pencil"):
        host.lobpcg(comm, exec_, P.A[False], P.d_x, 2, 5, 1e-6, B=other)
    other.close()
    # the other rules come first and are the standard solve's
    with pytest.raises(host.SpmvHostError, match="nev"):
        host.lobpcg(comm, exec_, P.A[False], P.d_x, 9, 5, 1e-6, B=P.B[False])
    stats = {}
    exec_.copy_from_host(P.d_x, lc.x0(P.N, 2, 1))
    k, _, _, _ = host.lobpcg(comm, exec_, P.A[False], P.d_x, 2, 3, 1e-12,
                             time_spmv=True, stats=stats, workspace=P.ws,
                             B=P.B[False])
    assert k == 3 and stats["spmv_launches"] == 3 and stats["spmv_ms_total"] > 0.0


# ---- 6. two slab ranks ------------------------------------------------------------------
@pytest.mark.parametrize("asynchronous", [False, True],
                         ids=["blocking", "stream-ordered"])
def test_two_slab_ranks_threaded(asynchronous):
    """Ranks as threads, Poisson 8^3 with B = I + 0.1 pattern in slabs (both have
    the same ghosts), nev = 3 with dinv: held to the theorem.  rtol 1e-6, kmax
    300: the restatement takes 58 iterations on one rank.  A B assembled without
    its ghosts breaks the rule on every rank before anything is launched.

    stream-ordered: thread_world's delayed asynchronous transport, where the
    exchange is only enqueued (as with RCCL) and the data moves late.  One
    exchange on A's column map serves both products, and B's own map has nothing
    in flight: a product of B that is not ordered behind A's exchange (the
    prologue's BX = B X comes with no product of A in front) reads the zeroed
    ghost tail, BX lacks the ghost columns' share, and X^T B X = I and the
    theorem below fail.  The blocking transport drains the stream and cannot
    see that."""
    from thread_world import ThreadWorld
    world, nev = 2, 3
    P = lg.pencil("mass8")
    N = P.N
    ranges = oracle.owner_ranges(world, N)
    loc = [[oracle.localise_rows(*csr, int(ranges[r]), int(ranges[r + 1]))
            for r in range(world)] for csr in (P.A, P.B)]
    X0 = lc.x0(N, nev, 9)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        d_x, d_dinv = exec_.alloc(M * nev), exec_.alloc(M)
        exec_.copy_from_host(d_dinv, np.full(M, 1.0 / 6.0))
        (arp, aci, ava, agh), (brp, bci, bva, bgh) = loc[0][rank], loc[1][rank]
        assert list(agh) == list(bgh) and len(agh) > 0
        # B's diagonal block alone: no ghosts
        own = bci < M
        rp0 = np.concatenate([[0], np.cumsum(np.bincount(
            np.repeat(np.arange(M), np.diff(brp))[own], minlength=M))])
        B0 = host.Matrix.create_matrix(
            comm, exec_, rp0.astype(brp.dtype), bci[own], bva[own], M, M, [], [],
            False, host.P2P_NONBLOCKING)
        A0 = host.Matrix.create_matrix(comm, exec_, arp, aci, ava, M, M, [], agh,
                                       False, host.P2P_NONBLOCKING)
        with pytest.raises(host.SpmvHostError, match="pencil"):
            host.lobpcg(comm, exec_, A0, d_x, nev, 5, 1e-6, B=B0)
        A0.close()
        B0.close()
        for sym_a, sym_b in ((False, False), (True, False), (True, True)):
            A = host.Matrix.create_matrix(comm, exec_, arp, aci, ava, M, M, [],
                                          agh, sym_a, host.P2P_NONBLOCKING)
            B = host.Matrix.create_matrix(comm, exec_, brp, bci, bva, M, M, [],
                                          bgh, sym_b, host.P2P_NONBLOCKING)
            exec_.copy_from_host(d_x, np.ascontiguousarray(X0[r0:r1]))
            k, theta, hist, status = host.lobpcg(comm, exec_, A, d_x, nev, 300,
                                                 1e-6, dinv=d_dinv, B=B)
            X = exec_.copy_to_host(d_x, M * nev).reshape(M, nev)
            ks = tw.gather(rank, np.array([k, status], np.int32)).reshape(world, 2)
            assert np.all(ks == ks[0]) and status == 0 and k < 300, ks
            for c in range(nev):
                h = hist[c]
                assert h[int(np.nonzero(h >= 0.0)[0][-1])] < 1e-6 * abs(theta[c])
            full = np.stack([tw.gather(rank, np.ascontiguousarray(X[:, c]))
                             for c in range(nev)], axis=1)
            lg.theorem_check_gen(P, theta, full, False, (rank, sym_a, sym_b))
            Bd, eps = P.dense()[1], np.finfo(np.float64).eps
            cond_b = P.eig()[3]
            assert np.abs(full.T @ Bd @ full - np.eye(nev)).max() <= (
                64 * 3 * nev * cond_b + N * np.sqrt(cond_b)) * eps
            A.close()
            B.close()
        exec_.free(d_x), exec_.free(d_dinv)

    tw.run(rank_body, gpu=True, asynchronous=asynchronous)


def test_two_slab_ranks_with_a_late_halo():
    """The stream-ordered transport with the data moving VERY late (2000 filler
    kernels, some tens of ms, in front of every copy) and kmax = 0: the solve is
    the prologue and the epilogue, three exchanges.  The prologue's BX = B X has
    no product of A in front of it, and B's own column map has nothing in
    flight, so only an explicit wait for A's exchange keeps B's product from
    reading the zeroed ghost tail of W.  Stale ghosts take the ghost columns'
    share (entries 0.1) out of BX on the 64 boundary rows of a rank: X^T B X
    then misses I by about 1e-2, and the recurrence's residual of it = 0 (from
    the implicit BX) differs from the epilogue's true residual (explicit BX, A's
    product first) by as much.  Asserted: X^T B X = I to the bound of
    test_lobpcg_gen_host.py, and the two residual norms equal to 1e-9 relative
    (they differ by the m roundings of one implicit update of AX and BX, some
    1e-14).  With the 40 filler kernels of the test above the copy usually lands
    before the host has launched B's product, and a missing wait passes."""
    from thread_world import ThreadWorld
    world, nev = 2, 3
    P = lg.pencil("mass8")
    N = P.N
    ranges = oracle.owner_ranges(world, N)
    loc = [[oracle.localise_rows(*csr, int(ranges[r]), int(ranges[r + 1]))
            for r in range(world)] for csr in (P.A, P.B)]
    X0 = lc.x0(N, nev, 9)
    tw = ThreadWorld(world, timeout=45.0)
    tw.delay_launches = 2000

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        d_x = exec_.alloc(M * nev)
        (arp, aci, ava, agh), (brp, bci, bva, bgh) = loc[0][rank], loc[1][rank]
        for sym_b in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, arp, aci, ava, M, M, [],
                                          agh, False, host.P2P_NONBLOCKING)
            B = host.Matrix.create_matrix(comm, exec_, brp, bci, bva, M, M, [],
                                          bgh, sym_b, host.P2P_NONBLOCKING)
            exec_.copy_from_host(d_x, np.ascontiguousarray(X0[r0:r1]))
            stats = {}
            k, theta, hist, status = host.lobpcg(comm, exec_, A, d_x, nev, 0, 1e-6,
                                                 B=B, stats=stats)
            assert (k, status) == (0, 0)
            X = exec_.copy_to_host(d_x, M * nev).reshape(M, nev)
            full = np.stack([tw.gather(rank, np.ascontiguousarray(X[:, c]))
                             for c in range(nev)], axis=1)
            Bd, eps = P.dense()[1], np.finfo(np.float64).eps
            cond_b = P.eig()[3]
            orth = np.abs(full.T @ Bd @ full - np.eye(nev)).max()
            assert orth <= (64 * 3 * nev * cond_b + N * np.sqrt(cond_b)) * eps, orth
            assert np.allclose(stats["true_resnorm"], hist[:, 0], rtol=1e-9,
                               atol=0.0), (stats["true_resnorm"], hist[:, 0])
            A.close()
            B.close()
        exec_.free(d_x)

    tw.run(rank_body, gpu=True, asynchronous=True)
