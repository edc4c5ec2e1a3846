"""spmv::lobpcg: whole solves on one rank (and two slab ranks as threads).

On general storage, with no preconditioner, dinv, SGS, ILU(0) and AMG, the
count, the Ritz values, the residual history and X equal
lobpcg_cases.lobpcg_ref bit for bit: mult_block has oracle.csr_spmv's bits per
column, sgs_apply_block those of test_gpu_sgs.Sweeps and of
ilu0_cases.Ilu0Ref, amg_apply_block those of amg_cases.AmgRef (the block
references test_gpu_sgs_block.py and test_gpu_amg_block.py hold them to).
Symmetric storage and several ranks are held to the theorem for symmetric A --
every theta_c lies within ||A x_c - theta_c x_c|| / ||x_c|| of an eigenvalue,
the residual computed independently by oracle.csr_spmv -- because lobpcg_ref is
composed on oracle.csr_spmv, whose row sums symmetric storage adds in another
order, and because Gram sums cross ranks in another order."""
import numpy as np
import pytest

import ilu0_cases as ic
import lobpcg_cases as lc
import oracle
import test_gpu_amg as ta
import test_gpu_sgs as ts
from spmv_amd import host
from test_gpu_lobpcg_kernels import same_values
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -777.25, 4


class _Problem:
    def __init__(self, exec_, comm, name):  # noqa: F811
        self.exec_, self.name = exec_, name
        self.case = P = lc.case(name)
        self.N = N = P.N
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *P.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.d_dinv = exec_.alloc(N + 1)
        exec_.copy_from_host(self.d_dinv, P.dinv())
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD + 1)
        self.ws = host.LobpcgWorkspace(exec_)
        self.M, self._pre_ref = {}, {}

    def pre(self, kind, sym=False):
        if kind == "none":
            return {}
        if kind == "dinv":
            return dict(dinv=self.d_dinv)
        if (kind, sym) not in self.M:
            A = self.A[sym]
            self.M[(kind, sym)] = (
                host.SgsPreconditioner(self.exec_, A) if kind == "sgs" else
                host.Ilu0Preconditioner(self.exec_, A) if kind == "ilu0" else
                host.AmgPreconditioner(self.exec_, A))
        M = self.M[(kind, sym)]
        return dict(amg=M) if kind == "amg" else dict(sgs=M)

    def precond_ref(self, kind):
        """r -> M^-1 r restated for general storage (made once), or None"""
        if kind in ("none", "dinv"):
            return None
        if kind not in self._pre_ref:
            P = self.case
            colours = self.pre(kind)["amg" if kind == "amg" else "sgs"]
            if kind == "amg":
                ref = ta.restate(P.csr, P.N, False)
                self._pre_ref[kind] = ref.apply
            else:
                colours = colours.colors()
                assert np.array_equal(
                    colours, host.sgs_color(P.csr[0], P.csr[1], P.N, P.N, False)[0])
                if kind == "sgs":
                    sw = ts.Sweeps(P.csr, P.N, colours, False)
                    dinv = 1.0 / P.diag
                    self._pre_ref[kind] = lambda r: sw.apply(dinv, r)
                else:
                    ref = ic.Ilu0Ref(P.csr, P.N, colours, False)
                    fac = ref.factor()
                    self._pre_ref[kind] = lambda r: ref.apply(fac, r)
        return self._pre_ref[kind]

    def solve(self, comm, X0, kmax, rtol, kind="none", sym=False,  # noqa: F811
              ws=None, x_off=GUARD, atol=0.0, **kw):
        e, N = self.exec_, self.N
        nev = X0.shape[1]
        size = N * 8 + 2 * GUARD + 1
        buf = np.full(size, SENTINEL)
        buf[x_off:x_off + N * nev] = X0.ravel()
        e.copy_from_host(self.d_x, buf)
        stats = {}
        k, theta, hist, status = host.lobpcg(
            comm, e, self.A[sym], self.d_x + 8 * x_off, nev, kmax, rtol, atol,
            workspace=ws or self.ws, stats=stats, **self.pre(kind, sym), **kw)
        out = e.copy_to_host(self.d_x, size)
        lo, hi = x_off, x_off + N * nev
        assert np.all(out[:lo] == SENTINEL) and np.all(out[hi:] == SENTINEL)
        return (k, theta.copy(), hist.copy(), status,
                out[lo:hi].reshape(N, nev).copy(), stats)

    def close(self):
        self.ws.close()
        for M in self.M.values():
            M.close()
        for A in self.A.values():
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


def _same_as_ref(got, ref, what):
    k, theta, hist, status, X, stats = got
    assert (k, status) == (ref["k"], ref["status"]), (what, k, status, ref["k"])
    assert same_values(theta, ref["theta"]), what
    assert same_values(hist, ref["hist"]), what
    assert same_values(X, ref["X"]), what
    assert same_values(stats["true_resnorm"], ref["true_resnorm"]), what
    assert stats["restarts"] == ref["restarts"], what


# ---- 1. bit for bit against the restatement ---------------------------------------
@pytest.mark.parametrize("kind", ["none", "dinv", "sgs", "ilu0", "amg"])
@pytest.mark.parametrize("nev", lc.NEV)
def test_bits_on_poisson11(comm, problems, nt, nev, kind):  # noqa: F811
    """rtol 1e-2: the first columns meet their test within kmax = 14, the last
    ones do not, so soft locking, the frozen history and P of an inactive
    column are all in the compared bits"""
    P = problems("poisson11")
    X0 = lc.x0(P.N, nev, 1)
    ref = P.case.ref(nev, kind, 14, 1e-2, X0=X0, precond=P.precond_ref(kind))
    for poll in (0, 1):
        got = P.solve(comm, X0, 14, 1e-2, kind, poll_every=poll)
        _same_as_ref(got, ref, (nev, kind, poll))
    got = P.solve(comm, X0, 14, 1e-2, kind, x_off=GUARD + 1)  # 8 bytes off
    _same_as_ref(got, ref, (nev, kind, "offset"))


@pytest.mark.parametrize("name,nev,largest", [
    ("shift11", 2, False), ("shift11", 3, True), ("diag300", 4, False),
    ("aniso480", 4, False), ("poisson11", 2, True)])
def test_bits_on_the_other_matrices(comm, problems, name, nev, largest):  # noqa: F811
    P = problems(name)
    X0 = lc.x0(P.N, nev, 2)
    for kind in ("none", "dinv"):
        ref = P.case.ref(nev, kind, 10, 1e-3, largest=largest, X0=X0)
        got = P.solve(comm, X0, 10, 1e-3, kind, largest=largest)
        _same_as_ref(got, ref, (name, nev, kind, largest))


def test_kmax_zero_and_atol(comm, problems):  # noqa: F811
    P = problems("poisson11")
    X0 = lc.x0(P.N, 3, 3)
    ref = P.case.ref(3, "none", 0, 1e-6, X0=X0)
    got = P.solve(comm, X0, 0, 1e-6)
    _same_as_ref(got, ref, "kmax 0")
    assert got[0] == 0 and np.all(got[2][:, 0] > 0.0)
    ref = P.case.ref(3, "none", 6, 0.0, atol=10.0, X0=X0)  # met at once
    got = P.solve(comm, X0, 6, 0.0, atol=10.0)
    _same_as_ref(got, ref, "atol")
    assert got[0] == 0


# ---- 2. held to the theorem ---------------------------------------------------------
@pytest.mark.parametrize("kind,sym", [("ilu0", False), ("amg", False),
                                      ("sgs", True), ("none", True),
                                      ("dinv", True)])
def test_theorem_on_poisson11(comm, problems, kind, sym):  # noqa: F811
    P = problems("poisson11")
    nev, kmax, rtol = 4, lc.KMAX_DEFAULT, 1e-6
    X0 = lc.x0(P.N, nev, 1)
    k, theta, hist, status, X, stats = P.solve(comm, X0, kmax, rtol, kind, sym)
    print(kind, sym, "k", k, "theta", theta, "true", stats["true_resnorm"])
    assert status == 0
    lc.theorem_check(P.case.csr, P.case.norm_a, P.case.eigvals(), theta, X,
                     False, (kind, sym))
    assert np.abs(X.T @ X - np.eye(nev)).max() <= 1e-12
    k_ref = lc.K_REF[("poisson11", nev, "none", False)]
    if kind in ("ilu0", "amg", "sgs"):  # a preconditioner pays
        assert k < k_ref, (kind, k, k_ref)
    else:  # the restatement's count, other summation orders
        assert abs(k - lc.K_REF[("poisson11", nev, kind, False)]) <= 2, (kind, k)


def test_symmetric_against_general_storage(comm, problems):  # noqa: F811
    P = problems("poisson11")
    X0 = lc.x0(P.N, 4, 4)
    a = P.solve(comm, X0, 30, 1e-5, "dinv", False)
    b = P.solve(comm, X0, 30, 1e-5, "dinv", True)
    assert abs(a[0] - b[0]) <= 1 and a[3] == b[3] == 0
    assert np.allclose(a[1], b[1], rtol=1e-9, atol=0.0)


def test_clustered_spectrum(comm, problems):  # noqa: F811
    """1, 2, 2, 2, 3: the cluster of three is found whole"""
    P = problems("diag300")
    X0 = lc.x0(P.N, 5, 5)
    k, theta, hist, status, X, _ = P.solve(comm, X0, 200, 1e-6, "none")
    assert status == 0 and k < 200
    lc.theorem_check(P.case.csr, P.case.norm_a, P.case.eigvals(), theta, X,
                     False, "diag300")
    assert np.allclose(theta, [1.0, 2.0, 2.0, 2.0, 3.0], rtol=1e-9)


# ---- 3. breakdowns --------------------------------------------------------------------
def test_rank_deficient_and_nan(comm, problems):  # noqa: F811
    P = problems("poisson11")
    e = P.exec_
    good = lc.x0(P.N, 3, 6)
    fresh_ws = host.LobpcgWorkspace(e)
    want = P.solve(comm, good, 8, 1e-3, "dinv", ws=fresh_ws)
    fresh_ws.close()
    ws = host.LobpcgWorkspace(e)
    # two equal columns.  The last pivot is then b - (b / sqrt(b))^2 - r12^2 in
    # rounded arithmetic: whether it fails `piv > 0` depends on the data (no
    # threshold other than > 0 decides), and seed 6 was chosen as one for which
    # the restatement's pivot does fail -- asserted below
    bad = good.copy()
    bad[:, 2] = bad[:, 0]
    k, theta, hist, status, X, _ = P.solve(comm, bad, 8, 1e-3, "dinv", ws=ws)
    assert (k, status) == (0, 1) and np.array_equal(X, bad)
    assert np.all(hist == -1.0)
    ref = P.case.ref(3, "dinv", 8, 1e-3, X0=bad)
    assert (ref["k"], ref["status"]) == (0, 1)
    got = P.solve(comm, good, 8, 1e-3, "dinv", ws=ws)  # the workspace is usable
    for a, b in zip(got[:5], want[:5]):
        assert same_values(a, b)
    bad = good.copy()
    bad[7, 1] = np.nan
    k, theta, hist, status, X, _ = P.solve(comm, bad, 8, 1e-3, "dinv", ws=ws)
    assert (k, status) == (0, 1)
    got = P.solve(comm, good, 8, 1e-3, "dinv", ws=ws)
    for a, b in zip(got[:5], want[:5]):
        assert same_values(a, b)
    # NaN in A
    rp, ci, va = P.case.csr
    va = va.copy()
    va[5] = np.nan
    A = host.Matrix.create_matrix(comm, e, rp, ci, va, P.N, P.N, [], [], False,
                                  host.P2P_NONBLOCKING)
    d_x = e.alloc(P.N * 3)
    e.copy_from_host(d_x, good)
    k, _, _, status = host.lobpcg(comm, e, A, d_x, 3, 8, 1e-3, workspace=ws)
    assert (k, status) == (0, 1)
    e.free(d_x)
    A.close()
    got = P.solve(comm, good, 8, 1e-3, "dinv", ws=ws)
    for a, b in zip(got[:5], want[:5]):
        assert same_values(a, b)
    ws.close()


def test_argument_rules(comm, problems):  # noqa: F811
    P = problems("poisson11")
    X0 = lc.x0(P.N, 2, 1)
    other = problems("diag300")
    sgs = other.pre("sgs")["sgs"]
    for match, kw in (("kmax", dict(kmax=-1)), ("tol", dict(rtol=0.0)),
                      ("tol", dict(rtol=np.nan)), ("rows", dict(sgs=sgs)),
                      ("preconditioner", dict(sgs=sgs, dinv=P.d_dinv))):
        args = dict(kmax=5, rtol=1e-6)
        args.update(kw)
        with pytest.raises(host.SpmvHostError, match=match):
            host.lobpcg(comm, P.exec_, P.A[False], P.d_x, 2, args["kmax"],
                        args["rtol"], dinv=args.get("dinv"), sgs=args.get("sgs"))
    for nev in (0, 9):
        with pytest.raises(host.SpmvHostError, match="nev"):
            host.lobpcg(comm, P.exec_, P.A[False], P.d_x, nev, 5, 1e-6)
    stats = {}
    P.exec_.copy_from_host(P.d_x, X0)
    k, _, _, _ = host.lobpcg(comm, P.exec_, P.A[False], P.d_x, 2, 3, 1e-12,
                             time_spmv=True, stats=stats, workspace=P.ws)
    assert k == 3 and stats["spmv_launches"] == 3 and stats["spmv_ms_total"] > 0.0


# ---- 4. two slab ranks ------------------------------------------------------------------
def test_two_slab_ranks_threaded():
    """Ranks as threads, the Poisson matrix of 8^3 in slabs, nev = 3 with dinv:
    held to the theorem (the Gram sums cross the ranks in another order)."""
    from thread_world import ThreadWorld
    import gmres_cases as gc
    world, n, nev = 2, 8, 3
    csr = gc.poisson(n)
    rp, ci, va = csr
    N = n ** 3
    eig = np.linalg.eigvalsh(lc.dense(csr))
    ranges = oracle.owner_ranges(world, N)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]
    X0 = lc.x0(N, nev, 9)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        d_x, d_dinv = exec_.alloc(M * nev), exec_.alloc(M)
        exec_.copy_from_host(d_dinv, np.full(M, 1.0 / 6.0))
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, sym, host.P2P_NONBLOCKING)
            exec_.copy_from_host(d_x, np.ascontiguousarray(X0[r0:r1]))
            k, theta, hist, status = host.lobpcg(comm, exec_, A, d_x, nev, 80,
                                                 1e-6, dinv=d_dinv)
            X = exec_.copy_to_host(d_x, M * nev).reshape(M, nev)
            ks = tw.gather(rank, np.array([k, status], np.int32)).reshape(world, 2)
            assert np.all(ks == ks[0]) and status == 0 and k < 80, ks
            full = np.stack([tw.gather(rank, np.ascontiguousarray(X[:, c]))
                             for c in range(nev)], axis=1)
            lc.theorem_check(csr, 12.0, eig, theta, full, False, (rank, sym))
            assert np.abs(full.T @ full - np.eye(nev)).max() <= 1e-12
            A.close()
        exec_.free(d_x), exec_.free(d_dinv)

    tw.run(rank_body, gpu=True)
