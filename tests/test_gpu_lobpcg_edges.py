"""Whole solves of host.lobpcg on the cases of lobpcg_edges.py: restarts that
recover and restarts that collapse, blocks that fill the space, exact
arithmetic, poisoned data and the workspace after it, systems scaled by powers
of two or negated, symmetric storage and two ranks.

On general storage no comparison has a tolerance: k, status, restarts, theta,
the history, X and true_resnorm equal lobpcg_cases.lobpcg_ref (what
test_lobpcg_edges_host.py holds the table to is not assumed here: the device is
compared with the restatement run on the same input), or keep a relation
between two GPU solves bit for bit.  Symmetric storage and two ranks add in
another order and are held to what survives it.

X sits between guard words (test_gpu_lobpcg._Problem.solve); the `nt` fixture
runs both instantiations of every vector kernel; poll_every = 16 lets the host
enqueue 16 iterations behind a stop."""
import numpy as np
import pytest

import lobpcg_cases as lc
import lobpcg_edges as le
import oracle
from lobpcg_edges import BY_ID, TABLE, same
from spmv_amd import host
from test_gpu_lobpcg import GUARD, _Problem, _same_as_ref
from test_gpu_lobpcg_kernels import same_values
from test_gpu_pcg import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

RESTARTED = [e for e in TABLE if e.cls in ("recovered", "kmax", "collapsed")]


class _Storages(dict):
    """general (False) and symmetric (True) storage, created on first use"""

    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, sym):
        self[sym] = self.make(sym)
        return self[sym]


class _Small(_Problem):
    """_Problem on a lobpcg_edges.Mat: any csr, the storages made on demand,
    dinv written before each solve that uses it"""

    def __init__(self, exec_, comm, M):  # noqa: F811
        self.exec_, self.name, self.case, self.N = exec_, M.name, M, M.N
        N = M.N
        self.A = _Storages(lambda sym: host.Matrix.create_matrix(
            comm, exec_, *M.csr, N, N, [], [], sym, host.P2P_NONBLOCKING))
        self.d_dinv = exec_.alloc(N + 1)
        self.d_x = exec_.alloc(N * 8 + 2 * GUARD + 1)
        self.ws = host.LobpcgWorkspace(exec_)
        self.M, self._pre_ref = {}, {}

    def set_dinv(self, dinv):
        self.exec_.copy_from_host(self.d_dinv, np.append(dinv, 0.0))


@pytest.fixture(scope="module")
def smalls(exec_, comm):  # noqa: F811
    made = {}

    def get(M):
        if M.name not in made:
            made[M.name] = _Small(exec_, comm, M)
        return made[M.name]
    yield get
    for p in made.values():
        p.close()


_REF = {}


def _ref(e, key="none", **kw):
    """the restatement on entry e (made once per key and never changed)"""
    if (e.id, key) not in _REF:
        _REF[(e.id, key)] = le.reference(e, **kw)
    return _REF[(e.id, key)]


def _solve(P, comm, e, kind=None, dinv=None, **kw):  # noqa: F811
    kind = kind or e.kind
    if kind == "dinv":
        P.set_dinv(e.dinv() if dinv is None else dinv)
    kw.setdefault("X0", e.X0())
    return P.solve(comm, kw.pop("X0"), e.kmax, e.rtol, kind, atol=e.atol,
                   largest=kw.pop("largest", e.largest), **kw)


def _held(got, ref, e, what):
    if e.bits:
        _same_as_ref(got, ref, what)
    else:
        assert (got[0], got[3]) == (ref["k"], ref["status"]), what
    assert bool(np.all(np.isfinite(got[4]))) == e.finite, what


# ---- 1. the table, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("e", [e for e in TABLE if e.want], ids=repr)
def test_table_on_general_storage(comm, smalls, nt, e):  # noqa: F811
    P = smalls(e.mat())
    ref = _ref(e)
    print(e.id, le.decisions(ref))
    for poll, x_off in ((1, GUARD), (16, GUARD), (16, GUARD + 1)):
        got = _solve(P, comm, e, poll_every=poll, x_off=x_off)
        _held(got, ref, e, (e.id, poll, x_off))


@pytest.mark.parametrize("e", RESTARTED, ids=repr)
def test_restarts_behind_a_preconditioner(comm, smalls, e):  # noqa: F811
    """group a with a dinv that varies, and on the tri matrices with SGS: the
    restart path with W = dinv * R from the residual kernel, and with the
    W-less residual call and sgs_apply_block"""
    P = smalls(e.mat())
    dinv = le.vary_dinv(P.N)
    ref = _ref(e, "dinv", dinv=dinv)
    print(e.id, "dinv", le.decisions(ref))
    for poll in (1, 16):
        got = _solve(P, comm, e, "dinv", dinv, poll_every=poll)
        _same_as_ref(got, ref, (e.id, "dinv", poll))
    if e.matrix.startswith("tri"):
        ref = _ref(e, "sgs", precond=P.precond_ref("sgs"))
        print(e.id, "sgs", le.decisions(ref))
        for poll in (1, 16):
            got = _solve(P, comm, e, "sgs", poll_every=poll)
            _same_as_ref(got, ref, (e.id, "sgs", poll))


# ---- 2. scaled and negated systems ------------------------------------------------------
def _relation(base, got, s, what):
    """2^s A (s = 0: another X0): every output of `got` from `base`"""
    assert (got[0], got[3]) == (base[0], base[3]), (what, got[0], got[3])
    assert same(got[1], np.ldexp(base[1], s)), what
    assert same(got[2], le.scaled_hist(base[2], s)), what
    assert same(got[4], base[4]) and np.all(np.isfinite(got[4])), what
    assert same(got[5]["true_resnorm"], np.ldexp(base[5]["true_resnorm"], s)), what
    assert got[5]["restarts"] == base[5]["restarts"], what


@pytest.mark.parametrize("id", ["e_none", "e_dinv"])
def test_scaled_systems(comm, smalls, id):  # noqa: F811
    e = BY_ID[id]
    P = smalls(e.mat())
    base = _solve(P, comm, e)
    _same_as_ref(base, _ref(e), id)
    d = e.dinv()
    for kind, eid, edge, (point, _) in le.EDGES:
        if eid != id:
            continue
        for v, inside in ((edge, True), (point, False)):
            if kind == "a":
                S = _Small(P.exec_, comm, le.Mat(
                    "%s*2^%d" % (e.matrix, v), le.scale_csr(e.mat().csr, v)))
                try:
                    with np.errstate(all="ignore"):
                        dv = None if d is None else np.ldexp(d, -v)
                    got = _solve(S, comm, e, dinv=dv)
                finally:
                    S.close()
            else:
                got = _solve(P, comm, e, X0=np.ldexp(
                    e.X0(), np.array(le.x_exponents(v))[None, :]))
            if inside:
                _relation(base, got, v if kind == "a" else 0, (id, kind, v))
            else:  # outside: whatever the restatement gives
                r, _ = (le.a_scaled if kind == "a" else le.x_scaled)(e, v)
                _same_as_ref(got, r, (id, kind, v, "outside"))


@pytest.mark.parametrize("id", le.NEGATED)
def test_negated_matrix(comm, smalls, id):  # noqa: F811
    e = BY_ID[id]
    P = smalls(e.mat())
    base = _solve(P, comm, e)
    S = _Small(P.exec_, comm, le.Mat("-" + e.matrix,
                                     le.scale_csr(e.mat().csr, 0, -1.0)))
    try:
        got = _solve(S, comm, e, largest=not e.largest)
    finally:
        S.close()
    r = dict(k=got[0], theta=got[1], hist=got[2], status=got[3], X=got[4],
             restarts=got[5]["restarts"])
    b = dict(k=base[0], theta=base[1], hist=base[2], status=base[3], X=base[4],
             restarts=base[5]["restarts"])
    assert base[0] == e.kmax and base[3] == 0
    assert le.negation_relation(b, r), id


# ---- 3. one workspace through everything ----------------------------------------------------
def test_the_workspace_after_every_exit(comm, smalls):  # noqa: F811
    """good, restart then collapse, good, poison, good, N = nev, good with
    another nev (the scalars are created again), theta = 0 exactly, good: every
    good solve equals the one on a fresh workspace in all five outputs"""
    good3, good4 = BY_ID["e_dinv"], BY_ID["e_shift_l"]
    e_ = smalls(good3.mat()).exec_
    ws = host.LobpcgWorkspace(e_)
    try:
        want = {}
        for g in (good3, good4):
            fresh = host.LobpcgWorkspace(e_)
            want[g.id] = _solve(smalls(g.mat()), comm, g, ws=fresh)
            fresh.close()
            assert want[g.id][0] == g.kmax and want[g.id][3] == 0

        def good(g, after):
            got = _solve(smalls(g.mat()), comm, g, ws=ws)
            for a, b in zip(got[:5], want[g.id][:5]):
                assert same_values(a, b), (g.id, "after", after)
            assert same_values(got[5]["true_resnorm"],
                               want[g.id][5]["true_resnorm"]), after

        good(good3, "nothing")
        for id, g in (("a_diag7", good3), ("d_dinv_nan", good3),
                      ("b_full3", good4), ("c_theta0", good3)):
            e = BY_ID[id]
            got = _solve(smalls(e.mat()), comm, e, ws=ws)
            _held(got, _ref(e), e, (id, "on the shared workspace"))
            good(g, id)
    finally:
        ws.close()


# ---- 4. symmetric storage ------------------------------------------------------------------
@pytest.mark.parametrize("e", RESTARTED, ids=repr)
def test_restart_cases_on_symmetric_storage(comm, smalls, e):  # noqa: F811
    """another summation order in the SpMV: the decisions may differ, k is not
    asserted.  The theorem is checked in rounded arithmetic, whose slack is
    n eps ||A||: it is not asked of Ritz values beyond 2 ||A|| (a_diag8 on the
    restatement, lobpcg_edges.is_wild), where the residual itself is rounded at
    eps |theta|"""
    P = smalls(e.mat())
    k, theta, hist, status, X, stats = _solve(P, comm, e, sym=True)
    print(e.id, "symmetric", k, status, stats["restarts"])
    assert status in (0, 1) and np.all(np.isfinite(X))
    M = e.mat()
    if status == 0 and np.abs(theta).max() <= 2.0 * M.norm_a:
        lc.theorem_check(M.csr, M.norm_a, M.eigvals(), theta, X, e.largest,
                         (e.id, "symmetric"))


# ---- 5. two ranks ----------------------------------------------------------------------------
def test_two_ranks_take_the_same_branch():
    """tri(16) in two slabs of 8 rows, the case that collapses under every
    summation order tried: the branch is taken from all-reduced Gram sums, which
    every transport here leaves with the same bits on every rank (DESIGN.md
    7u), so both ranks return the same k, status and restarts"""
    from thread_world import ThreadWorld
    e = BY_ID[le.TWO_RANKS]
    M = e.mat()
    rp, ci, va = M.csr
    N, nev, world = M.N, e.nev, 2
    ranges = oracle.owner_ranges(world, N)
    assert [int(r) for r in ranges] == [0, 8, 16]
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]
    X0 = e.X0()
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        m = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        d_x = exec_.alloc(m * nev)
        A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, m, m, [], gh,
                                      False, host.P2P_NONBLOCKING)
        exec_.copy_from_host(d_x, np.ascontiguousarray(X0[r0:r1]))
        stats = {}
        k, theta, hist, status = host.lobpcg(comm, exec_, A, d_x, nev, e.kmax,
                                             e.rtol, stats=stats)
        X = exec_.copy_to_host(d_x, m * nev).reshape(m, nev)
        mine = np.array([k, status, stats["restarts"]], np.int32)
        ks = tw.gather(rank, mine).reshape(world, 3)
        print("rank", rank, "k, status, restarts", ks.tolist())
        assert np.all(ks == ks[0]), ks
        th = tw.gather(rank, theta.copy()).reshape(world, nev)
        assert same(th[0], th[1])
        full = np.stack([tw.gather(rank, np.ascontiguousarray(X[:, c]))
                         for c in range(nev)], axis=1)
        assert status in (0, 1) and np.all(np.isfinite(full))
        if status == 0:
            lc.theorem_check(M.csr, M.norm_a, M.eigvals(), theta, full, False,
                             ("two ranks", rank))
        A.close()
        exec_.free(d_x)

    tw.run(rank_body, gpu=True)
