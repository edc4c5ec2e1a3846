"""spmv::pcg_block with an AmgPreconditioner on the device.

Per column against the restatement of amg_block_cases.py (block_ref with
AmgRef.apply per column) through test_gpu_chebyshev._vs_ref unchanged: the same
k, the history within its bar, for the columns test_amg_block_host.py keeps
(dev_ref below a tenth of the bar).  Exact claims beside it: a column does not
see its neighbours, stopped columns are frozen, a zero column stops at k = 0,
nrhs = 1 is pcg_amg bit for bit.  X sits between guard words."""
import numpy as np
import pytest

import amg_block_cases as abc
import test_gpu_cg_block as tb
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
from spmv_amd import host
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
KMAX, RTOL = abc.KMAX, abc.RTOL


class _Problem:
    def __init__(self, exec_, comm, name):  # noqa: F811
        self.name, self.exec_ = name, exec_
        self.case = P = abc.case(name)
        self.N = N = P.N
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *P.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.M = {sym: host.AmgPreconditioner(exec_, A)
                  for sym, A in self.A.items()}
        self.d_b = exec_.alloc(N * 8)
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD + 1)
        self.ws = host.PcgBlockWorkspace(exec_)

    def solve(self, comm, B, kmax=KMAX, rtol=RTOL, symmetric=False,  # noqa: F811
              ws=None, x_off=GUARD, **kw):
        e, (N, nrhs) = self.exec_, B.shape
        size = N * 8 + 2 * GUARD + 1
        e.copy_from_host(self.d_b, np.ascontiguousarray(B))
        e.copy_from_host(self.d_x, np.full(size, SENTINEL))
        its, hist, _ = host.pcg_block(comm, e, self.A[symmetric], self.d_b,
                                      self.d_x + 8 * x_off, nrhs, kmax, rtol,
                                      workspace=ws or self.ws,
                                      amg=self.M[symmetric], **kw)
        buf = e.copy_to_host(self.d_x, size)
        lo, hi = x_off, x_off + N * nrhs
        assert np.all(buf[:lo] == SENTINEL) and np.all(buf[hi:] == SENTINEL)
        X = buf[lo:hi].reshape(N, nrhs).copy()
        assert not np.any(X == SENTINEL)
        return its.copy(), hist.copy(), X

    def vs_ref(self, names, its, hist, X, what, kmax=KMAX, rtol=RTOL):
        tb._check_history_tail(its, hist, what)
        for c, col in enumerate(names):
            k = int(its[c])
            if col == "zero":
                assert k == 0 and hist[c, 0] == 0.0 and np.all(X[:, c] == 0.0)
                continue
            ref = self.case.ref(col, kmax, rtol)
            assert k == ref.k, (what, col, k, ref.k)
            tc._vs_ref(k, hist[c, :k + 1], X[:, c], ref, self.case.norm_a,
                       what + (col,), kmax, rtol)

    def close(self):
        self.ws.close()
        for M in self.M.values():
            M.close()
        for A in self.A.values():
            A.close()
        for p in (self.d_b, self.d_x):
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
@pytest.mark.parametrize("shape,nrhs", [
    ("poisson11", 1), ("poisson11", 2), ("poisson11", 3), ("poisson11", 4),
    ("poisson11", 8), ("banded4097", 2), ("banded4097", 5), ("banded4097", 8),
    ("poisson24", 4)])
def test_per_column_against_the_restatement(comm, problems, nt,  # noqa: F811
                                            shape, nrhs):
    P = problems(shape)
    names = abc.POOL[shape][:nrhs]
    for symmetric in (False, True):
        its, hist, X = P.solve(comm, P.case.block(names), symmetric=symmetric)
        assert its.max() < KMAX
        assert np.all(np.isfinite(X))
        P.vs_ref(names, its, hist, X, (shape, nrhs, symmetric))


# ---- 2. independence, frozen columns, the zero column ---------------------------------
@pytest.mark.parametrize("nrhs", [4, 3])
@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_a_column_does_not_see_the_others(comm, problems, shape, nrhs):  # noqa: F811
    """The kept column beside two sets of neighbours -- swapped, one of them
    zero (it stops at once), one the slow eigenvector column, and one poisoned
    with NaN and Inf: its x, history and count keep their bits."""
    P = problems(shape)
    cols = P.case.cols
    others_a = ["rand1", "rand2", "rand3"]
    others_b = ["zero", "eig" if P.case.base.n_grid else "rand4", "rand1"]
    poison = cols["rand2"].copy()
    poison[::7] = np.nan
    poison[3::11] = np.inf
    for slot in (0, nrhs - 1):
        got = []
        for variant in ("a", "b", "poisoned"):
            B = np.empty((P.N, nrhs))
            others = others_a if variant != "b" else others_b
            o = iter(others)
            for c in range(nrhs):
                B[:, c] = cols["rand0"] if c == slot else cols[next(o)]
            if variant == "poisoned":
                B[:, (slot + 1) % nrhs] = poison
            its, hist, X = P.solve(comm, B)
            got.append((int(its[slot]), hist[slot].copy(), X[:, slot].copy()))
            if variant == "b":
                z = [c for c in range(nrhs) if c != slot][0]
                assert its[z] == 0 and np.all(X[:, z] == 0.0)
        for k, h, x in got[1:]:
            assert k == got[0][0], (shape, nrhs, slot)
            assert np.array_equal(h, got[0][1]), (shape, nrhs, slot)
            assert np.array_equal(x, got[0][2]), (shape, nrhs, slot)
        assert got[0][0] == P.case.ref("rand0").k


def test_stopped_columns_are_frozen(comm, problems):  # noqa: F811
    """Columns that stop at different k: what a column holds when it stops is
    what the solve returns, however long the others go on -- the same block
    cut at kmax = that column's k gives the column the same bits."""
    P = problems("poisson11")
    names = ["ones", "zero", "eig", "rand0"]
    its, hist, X = P.solve(comm, P.case.block(names))
    assert its[1] == 0 and hist[1, 0] == 0.0 and np.all(X[:, 1] == 0.0)
    assert np.all(hist[1, 1:] == -1.0)
    assert len(set(its.tolist())) >= 3, its
    for c, col in enumerate(names):
        k = int(its[c])
        if col == "zero" or k == its.max():
            continue
        i1, h1, x1 = P.solve(comm, P.case.block(names), kmax=k)
        assert int(i1[c]) == k, col
        assert np.array_equal(h1[c, :k + 1], hist[c, :k + 1]), col
        assert np.array_equal(x1[:, c], X[:, c]), col


@pytest.mark.parametrize("shape", ["poisson11", "banded4097"])
def test_one_column_is_pcg_amg(comm, problems, shape):  # noqa: F811
    """nrhs = 1 against pcg_amg on the same objects: the same k and the bits
    of the history and of x (a block of one column is handed to pcg_amg)."""
    P = problems(shape)
    e, N = P.exec_, P.N
    d_x1 = e.alloc(N)
    ws = host.AmgPcgWorkspace(e)
    try:
        for symmetric in (False, True):
            for col in ("ones", "rand0"):
                its, hist, X = P.solve(comm, P.case.block([col]),
                                       symmetric=symmetric)
                e.copy_from_host(P.d_b, P.case.cols[col])
                k, h = host.pcg_amg(comm, e, P.A[symmetric], P.M[symmetric],
                                    P.d_b, d_x1, KMAX, RTOL, ws)
                dev = float(np.abs(hist[0, :k + 1] / h - 1).max()) \
                    if int(its[0]) == k else np.inf
                print(shape, symmetric, col, "k", int(its[0]), k,
                      "history deviation", dev)
                assert int(its[0]) == k, (shape, symmetric, col)
                assert np.array_equal(hist[0, :k + 1], h), (shape, symmetric, col)
                assert np.array_equal(X[:, 0], e.copy_to_host(d_x1, N))
    finally:
        ws.close()
        e.free(d_x1)


# ---- 3. workspace reuse, an unaligned X, errors -----------------------------------------
def test_workspace_reuse_and_an_unaligned_x(comm, problems):  # noqa: F811
    """One workspace over solves of different nrhs and kmax, a fresh one, and X
    8 bytes off: the same bits."""
    P = problems("poisson11")
    names = abc.POOL["poisson11"]
    ws = host.PcgBlockWorkspace(P.exec_)
    try:
        first = P.solve(comm, P.case.block(names[:4]), ws=ws)
        P.solve(comm, P.case.block(names[:8]), ws=ws, kmax=5)
        P.solve(comm, P.case.block(names[:2]), ws=ws, kmax=300)
        again = P.solve(comm, P.case.block(names[:4]), ws=ws)
        off = P.solve(comm, P.case.block(names[:4]), x_off=GUARD + 1)
        for other in (again, off):
            for a, b in zip(first, other):
                assert np.array_equal(a, b)
    finally:
        ws.close()


def test_error_paths(comm, problems):  # noqa: F811
    P, Q = problems("poisson11"), problems("banded4097")
    e = P.exec_
    args = (comm, e, P.A[False], P.d_b, P.d_x, 4, 10, 1e-8)
    with pytest.raises(host.SpmvHostError, match="rows"):
        host.pcg_block(*args, amg=Q.M[False])
    with pytest.raises(host.SpmvHostError, match="preconditioner"):
        host.pcg_block(*args, amg=P.M[False], dinv=P.d_b)
    with pytest.raises(host.SpmvHostError, match="nrhs"):
        host.pcg_block(comm, e, P.A[False], P.d_b, P.d_x, 9, 10, 1e-8,
                       amg=P.M[False])
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.pcg_block(comm, e, P.A[False], P.d_b, P.d_x, 4, -1, 1e-8,
                       amg=P.M[False])
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.pcg_block(comm, e, P.A[False], P.d_b, P.d_b + 8, 4, 10, 1e-8,
                       amg=P.M[False])
    # the stream is restored and the next solve is the usual one
    names = abc.POOL["poisson11"][:2]
    its, hist, X = P.solve(comm, P.case.block(names))
    P.vs_ref(names, its, hist, X, ("after errors",))


# ---- 4. several ranks ------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slab_ranks_threaded(world):
    """Ranks as threads, the Poisson matrix of 8^3 in slabs, a blocking and an
    overlapping halo model, nrhs = 4, the cycle block-Jacobi over the ranks
    (no halo exchange), ONE workspace per rank over all solves; every column
    against the restatement on oracle.dist_spmv with the rank-ordered sum."""
    from thread_world import ThreadWorld
    S = abc.slab_case(world)
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
        for cm, ref in refs.items():
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, cm)
            pre = host.AmgPreconditioner(exec_, A, **S.OPTIONS)
            assert pre.levels() >= 2
            exec_.copy_from_host(d_b, np.ascontiguousarray(B[r0:r1]))
            exec_.copy_from_host(d_x, np.full(M * 4 + 2 * GUARD, SENTINEL))
            its, hist, _ = host.pcg_block(comm, exec_, A, d_b, d_x + 8 * GUARD, 4,
                                          kmax, rtol, amg=pre, workspace=ws)
            buf = exec_.copy_to_host(d_x, M * 4 + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL)
            assert np.all(buf[GUARD + M * 4:] == SENTINEL)
            X = buf[GUARD:GUARD + M * 4].reshape(M, 4)
            all_its = tw.gather(rank, its).reshape(world, 4)
            assert np.all(all_its == all_its[0]), all_its
            tb._check_history_tail(its, hist, (cm,))
            for c in range(4):
                xs = tw.gather(rank, np.ascontiguousarray(X[:, c]))
                k = int(its[c])
                assert k < kmax and k == ref[c].k, (world, cm, c, k, ref[c].k)
                tc._vs_ref(k, hist[c, :k + 1], xs, ref[c], norm_a,
                           (world, cm, c), kmax, rtol)
            pre.close()
            A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)
