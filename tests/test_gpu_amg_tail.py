"""The fused tail of the AMG V-cycle on the GPU, bit for bit.

1. The object: AmgPreconditioner.set_tail_rows on the matrices of
   test_gpu_amg.py.  Every case asserts tail_levels() BEFORE it compares, so
   none passes by running the plain cycle; amg_apply then equals AmgRef.apply
   and the same object with the tail off.  refresh, toggling, poisoned
   right-hand sides, and the solvers (pcg_amg, gmres with amg; one case on two
   slab ranks) against the same solve with the tail off: k, x and the whole
   history.
2. The kernel alone: spmv_hip_amg_tail_run_f64 on the hand-built levels of
   amg_tail_cases.py against amg_tail_cases.tail_ref, outputs between guard
   words and pre-filled with a sentinel, inputs read back.

Comparisons are np.array_equal (special_values.same_bits where a NaN may
occur).  Nothing here has a tolerance."""
import numpy as np
import pytest

import amg_cases as ac
import amg_tail_cases as tc
import oracle
import test_gpu_amg as ta
import test_gpu_pcg as tp
from special_values import same_bits
from spmv_amd import _lib, hip, host
from test_gpu_amg import problems  # noqa: F401  (fixture)
from test_gpu_amg_kernels import Pool, kexec, pool  # noqa: F401  (fixtures)
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = ta.SENTINEL, ta.GUARD
OFFSETS = ta.OFFSETS


def _off_after(Ms):
    for M in Ms:
        M.set_tail_rows(0)
        assert M.tail_levels() == 0


def _check_object(P, expect, what, rhs=("rand",)):
    """every setting of `expect` on every storage of P: tail_levels, then the
    bits of the reference and of the tail-off object"""
    nl = len(P.ref[False].levels)
    try:
        for sym in P.storages:
            M, ref = P.M[sym], P.ref[sym]
            assert M.levels() == nl
            for name in rhs:
                r = P.rhs[name]
                want = ref.apply(r)
                M.set_tail_rows(0)
                assert M.tail_levels() == 0
                off = P.apply(r, sym)
                assert np.array_equal(off, want), (what, sym, "tail off")
                for tail_rows, levels in expect.items():
                    M.set_tail_rows(tail_rows)
                    assert M.tail_levels() == levels, \
                        (what, sym, tail_rows, M.tail_levels(), levels)
                    for r_off, z_off in OFFSETS:
                        z = P.apply(r, sym, r_off, z_off)
                        bad = int(np.sum(z != want))
                        assert np.array_equal(z, want), \
                            (what, sym, tail_rows, r_off, bad)
                        assert np.array_equal(z, off), (what, sym, tail_rows)
    finally:
        _off_after(P.M.values())


# ---- 1. the object ------------------------------------------------------------------------
@pytest.mark.parametrize("options", [
    {}, {"smooth_degree": 1}, {"smooth_degree": 3}, {"coarse_degree": 1},
    {"coarse_scale": 1.6},
    {"smooth_degree": 1, "coarse_degree": 1, "coarse_scale": 1.6},
    {"smooth_degree": 3, "coarse_degree": 1, "coarse_scale": 1.6}],
    ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_poisson24(problems, options):  # noqa: F811
    name, _, sizes, expect = tc.POISSON24
    P = problems(name, False, **options)
    assert tuple(L["n"] for L in P.ref[False].levels) == sizes
    assert expect == {149: 0, 150: 1, 1685: 2, 10 ** 9: 2}
    _check_object(P, expect, (name, options))


@pytest.mark.parametrize("case", tc.FURTHER, ids=lambda c: c[0])
def test_further_matrices(problems, case):  # noqa: F811
    name, options, sizes, expect = case
    P = problems(name, False, **options)
    assert tuple(L["n"] for L in P.ref[False].levels) == sizes
    _check_object(P, expect, (name, options), rhs=("rand", "ones"))


def test_ragged_level_1_runs_the_vector_order(problems):  # noqa: F811
    """its level 1 is the whole tail, and the plan says which order ran"""
    P = problems("ragged3001", False)
    try:
        for sym in P.storages:
            M, ref = P.M[sym], P.ref[sym]
            lanes = ac.vector_lanes(ref.levels[1]["csr"])
            assert lanes == 64
            M.set_tail_rows(77)
            assert M.tail_levels() == 1
            assert M.tail_lanes(1) == lanes and M.tail_lanes(0) == -1
            r = P.rhs["rand"]
            z = P.apply(r, sym)
            assert np.array_equal(z, ref.apply(r)), sym
            # the sequential order would not have given these bits
            seq = ta.ac.AmgRef(P.csr, P.N) if not sym else None
            if seq is not None:
                assert np.any(seq.apply(r) != z)
    finally:
        _off_after(P.M.values())


def test_one_level_has_no_tail_and_a_negative_setting_is_refused(problems):  # noqa: F811
    P = problems("diag200", False)
    M = P.M[False]
    for tail_rows in (1, 200, 10 ** 9):
        M.set_tail_rows(tail_rows)
        assert M.tail_levels() == 0
        assert np.array_equal(P.apply(P.rhs["rand"]),
                              P.ref[False].apply(P.rhs["rand"]))
    with pytest.raises(host.SpmvHostError, match="tail_rows"):
        M.set_tail_rows(-1)
    M.set_tail_rows(0)


def test_plan_bytes_include_the_table(problems):  # noqa: F811
    P = problems("poisson24", False)
    M = P.M[False]
    M.set_tail_rows(0)
    base = M.plan_bytes()
    try:
        M.set_tail_rows(150)
        one = M.plan_bytes()
        M.set_tail_rows(1685)
        two = M.plan_bytes()
        assert base < one < two and two - one == one - base
    finally:
        _off_after([M])


def test_toggling(problems):  # noqa: F811
    P = problems("poisson24", False)
    M, r = P.M[False], P.rhs["rand"]
    got = []
    try:
        for tail_rows, levels in ((0, 0), (1685, 2), (0, 0), (1685, 2)):
            M.set_tail_rows(tail_rows)
            assert M.tail_levels() == levels
            got.append(P.apply(r))
        assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
        assert np.array_equal(got[0], got[1])
    finally:
        _off_after([M])


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf, 1e300],
                         ids=["nan", "pinf", "ninf", "1e300"])
def test_poison_then_clean(problems, poison):  # noqa: F811
    """a poisoned r gives the bits of the tail-off object, NaN where that has
    one; the next clean application gives the bits it gave before"""
    P = problems("poisson24", False)
    M, e, N = P.M[False], P.exec_, P.N
    clean = P.rhs["rand"]

    def applied(r):  # (P.apply insists on finite results)
        e.copy_from_host(P.d_b, r)
        e.copy_from_host(P.d_x, np.full(N + 2 * GUARD, SENTINEL))
        host.amg_apply(e, M, P.d_b, P.d_x + 8 * GUARD)
        buf = e.copy_to_host(P.d_x, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + N:] == SENTINEL)
        return buf[GUARD:GUARD + N].copy()
    try:
        for row in (0, N // 2, N - 1):
            r = clean.copy()
            r[row] = poison
            M.set_tail_rows(0)
            off, off_clean = applied(r), applied(clean)
            M.set_tail_rows(1685)
            assert M.tail_levels() == 2
            before = applied(clean)
            on = applied(r)
            assert same_bits(on, off), (poison, row)
            assert not np.all(np.isfinite(on)) or poison == 1e300
            after = applied(clean)
            assert np.array_equal(after, before), (poison, row)
            assert np.array_equal(after, off_clean), (poison, row)
    finally:
        _off_after([M])


def test_refresh_keeps_the_tail_consistent(exec_, comm):  # noqa: F811
    """new values in place change lmax of the tail's levels: apply equals the
    restatement with frozen aggregates; a refresh that throws leaves the object
    unusable, a good one restores it with the tail still on"""
    e = exec_
    csr = tp._scaled(ta._make_csr("poisson11"))
    N = len(csr[0]) - 1
    d_r, d_z = e.alloc(N), e.alloc(N)
    opts = {"min_coarse_rows": 20}

    def applied(pre, r):
        e.copy_from_host(d_r, r)
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.amg_apply(e, pre, d_r, d_z)
        return e.copy_to_host(d_z, N)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        M = host.AmgPreconditioner(e, A, **opts)
        old = ta.restate(csr, N, sym, **opts)
        nl = len(old.levels)
        assert nl >= 3 and M.levels() == nl
        M.set_tail_rows(10 ** 9)
        assert M.tail_levels() == nl - 1
        new = ta._changed(csr, 0.05)
        r = oracle.csr_spmv(*new, np.random.default_rng(3).uniform(-1, 1, N))
        assert np.array_equal(applied(M, r), old.apply(r))
        ta._write_values(e, A, new, sym)
        M.refresh(A)
        assert M.tail_levels() == nl - 1
        ref = ta.restate(new, N, sym, frozen=old, **opts)
        for l in range(1, nl):
            assert ref.levels[l]["lmax"] != old.levels[l]["lmax"]
            assert M.lmax(l) == ref.levels[l]["lmax"]
        want = ref.apply(r)
        assert np.array_equal(applied(M, r), want), (sym, "refreshed")
        assert np.any(want != old.apply(r))
        on = np.flatnonzero(new[1] == tp._row_of(new[0])[:len(new[1])])
        bad = (new[0], new[1], new[2].copy())
        bad[2][on[5 % len(on)]] = -1.0
        ta._write_values(e, A, bad, sym)
        with pytest.raises(host.SpmvHostError, match="diagonal is not positive"):
            M.refresh(A)
        with pytest.raises(host.SpmvHostError, match="refresh"):
            host.amg_apply(e, M, d_r, d_z)
        ta._write_values(e, A, new, sym)
        M.refresh(A)
        assert M.tail_levels() == nl - 1
        assert np.array_equal(applied(M, r), want), (sym, "again")
        M.set_tail_rows(0)
        assert np.array_equal(applied(M, r), want), (sym, "off")
        M.close()
        A.close()
    e.free(d_r), e.free(d_z)


SOLVE_CASES = [("poisson24", {}, 1685, 2),
               ("convdiff8", {"min_coarse_rows": 20}, 72, 2)]


@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: c[0])
def test_solvers_keep_their_bits(comm, problems, case):  # noqa: F811
    name, options, tail_rows, levels = case
    P = problems(name, False, **options)
    M = P.M[False]
    try:
        M.set_tail_rows(0)
        gm_off = P.gmres(comm, "rand", 30)
        pcg_off = P.solve(comm, "rand") if name != "convdiff8" else None
        M.set_tail_rows(tail_rows)
        assert M.tail_levels() == levels
        gm_on = P.gmres(comm, "rand", 30)
        assert gm_on[0] == gm_off[0] and gm_on[3] == gm_off[3]
        assert np.array_equal(gm_on[1], gm_off[1]), (name, "gmres history")
        assert np.array_equal(gm_on[2], gm_off[2]), (name, "gmres x")
        if pcg_off is not None:  # (CG is for the symmetric matrix)
            pcg_on = P.solve(comm, "rand")
            assert pcg_on[0] == pcg_off[0] and pcg_on[0] > 1
            assert np.array_equal(pcg_on[1], pcg_off[1]), (name, "pcg history")
            assert np.array_equal(pcg_on[2], pcg_off[2]), (name, "pcg x")
    finally:
        _off_after([M])


def test_pcg_amg_on_convdiff_keeps_its_bits(comm, problems):  # noqa: F811
    """(nonsymmetric: CG need not converge; a fixed number of iterations,
    the same bits with and without the tail)"""
    P = problems("convdiff8", False, min_coarse_rows=20)
    M = P.M[False]
    e, N = P.exec_, P.N

    def solve():
        e.copy_from_host(P.d_b, P.rhs["rand"])
        e.copy_from_host(P.d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist = host.pcg_amg(comm, e, P.A[False], M, P.d_b,
                               P.d_x + 8 * GUARD, 12, 0.0, P.ws)
        return k, hist.copy(), e.copy_to_host(P.d_x, N + 2 * GUARD)
    try:
        M.set_tail_rows(0)
        off = solve()
        M.set_tail_rows(72)
        assert M.tail_levels() == 2
        on = solve()
        assert on[0] == off[0] == 12
        assert same_bits(on[1], off[1]) and same_bits(on[2], off[2])
    finally:
        _off_after([M])


def test_two_slab_ranks_pcg_amg():
    """ranks as threads, the scaled Poisson matrix of 8^3 in two slabs, one
    halo model: k, x and the history with the tail equal those without"""
    from thread_world import ThreadWorld
    world = 2
    (rp, ci, va), _ = tp._slab_inputs(8)
    N = len(rp) - 1
    b = oracle.csr_spmv(rp, ci, va, np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        ws = host.AmgPcgWorkspace(exec_)
        d_b, d_x = exec_.alloc(M), exec_.alloc(M + 2 * GUARD)
        A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [], gh,
                                      False, host.P2P_NONBLOCKING)
        pre = host.AmgPreconditioner(exec_, A, min_coarse_rows=20)
        assert pre.levels() >= 2
        got = []
        for tail_rows in (0, 10 ** 9):
            pre.set_tail_rows(tail_rows)
            assert pre.tail_levels() == (pre.levels() - 1 if tail_rows else 0)
            exec_.copy_from_host(d_b, b[r0:r1])
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
            k, hist = host.pcg_amg(comm, exec_, A, pre, d_b, d_x + 8 * GUARD,
                                   ta.KMAX, ta.RTOL, ws)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL)
            assert np.all(buf[GUARD + M:] == SENTINEL)
            got.append((k, hist.copy(), buf[GUARD:GUARD + M].copy()))
        assert got[0][0] == got[1][0] and 1 < got[0][0] < ta.KMAX
        assert np.array_equal(got[0][1], got[1][1]), "history"
        assert np.array_equal(got[0][2], got[1][2]), "x"
        pre.close()
        A.close()
        exec_.free(d_b), exec_.free(d_x)
        ws.close()

    tw.run(rank_body, gpu=True)


# ---- 2. the kernel alone ------------------------------------------------------------------
class _Built:
    """a hand-built tail on the device: guarded vectors, plans, the handle"""

    def __init__(self, pool, t, corrupt=None):  # noqa: F811
        self.t, self.vec, self.inputs, self.desc = t, [], [], []
        self.ctx, self.tail = pool.e.context, None
        for l, L in enumerate(t.levels):
            rp, ci, va = L.csr
            values, dinv = pool.vec(va), pool.vec(L.dinv)
            r = pool.vec(t.r) if l == 0 else pool.out(L.n)
            v = dict(r=r, w=pool.out(L.n), dd=pool.out(L.n), z=pool.out(L.n))
            self.vec.append(v)
            self.inputs += [values, dinv] + ([r] if l == 0 else [])
            self.desc.append(dict(
                rows=L.n, lanes_per_row=L.lanes, nnz=len(ci),
                rowptr=pool.raw(np.ascontiguousarray(rp, np.int32)),
                colind=pool.raw(np.ascontiguousarray(ci, np.int32)),
                values=values.ptr, dinv=dinv.ptr, r=r.ptr, w=v["w"].ptr,
                dd=v["dd"].ptr, z=v["z"].ptr,
                step=pool.plan(L.step) if L.step is not None else None,
                a=L.a, b=L.b))
        if corrupt:
            corrupt(self.desc, pool)
        else:
            self.create()

    def create(self):
        t = self.t
        self.tail = hip.AmgTail(self.ctx, self.desc, t.s, t.c, t.scale)

    def untouched(self, what):
        for l, v in enumerate(self.vec):
            for k, x in v.items():
                if l == 0 and k == "r":
                    x.unchanged(what)
                else:
                    assert np.all(x.read(what) == SENTINEL), (what, l, k)


def _run(pool, t):  # noqa: F811
    built = _Built(pool, t)
    try:
        assert built.tail.bytes() > 0
        built.tail.run()
        rs, zs = t.ref()
        for l, v in enumerate(built.vec):
            v["z"].expect(zs[l], (t.name, "z", l))
            if l > 0:
                v["r"].expect(rs[l], (t.name, "r", l))
            v["w"].read((t.name, "w", l))  # the guards
            v["dd"].read((t.name, "dd", l))
        for x in built.inputs:
            x.unchanged(t.name)
    finally:
        pool.e.synchronize()
        built.tail.close()


@pytest.mark.parametrize("n", tc.SIZES)
def test_kernel_level_sizes(pool, n):  # noqa: F811
    _run(pool, tc.size_case(n))


def test_kernel_aggregates_and_a_coarse_level_of_one_row(pool):  # noqa: F811
    _run(pool, tc.aggregate_case())
    _run(pool, tc.one_coarse_row_case())


def test_kernel_sequential_order(pool):  # noqa: F811
    _run(pool, tc.sequential_lens_case())


@pytest.mark.parametrize("lanes", [4, 64])
def test_kernel_vector_order(pool, lanes):  # noqa: F811
    t = tc.vector_case(lanes)
    _run(pool, t)
    # (the two orders differ on these rows: the case tells them apart)
    seq = tc.Tail.__new__(tc.Tail)
    seq.__dict__.update(t.__dict__)
    seq.levels = [tc.Level(L.csr, L.dinv, L.a, L.b, L.step, 0) for L in t.levels]
    assert not same_bits(seq.ref()[1][0], t.ref()[1][0])


@pytest.mark.parametrize("s,c,scale", [(1, 1, 1.0), (1, 8, 1.6), (2, 1, 1.6),
                                       (3, 8, 1.0), (16, 16, 1.0)])
def test_kernel_degrees(pool, s, c, scale):  # noqa: F811
    _run(pool, tc.degree_case(s, c, scale))


def test_kernel_special_values(pool):  # noqa: F811
    for t in tc.special_cases():
        _run(pool, t)


@pytest.mark.parametrize("s,c,lanes", [(2, 3, 0), (1, 1, 0), (3, 8, [0, 8, 4])])
def test_kernel_three_levels(pool, s, c, lanes):  # noqa: F811
    _run(pool, tc.depth_case(s, c, lanes))


def test_kernel_set_coefficients(pool):  # noqa: F811
    t = tc.degree_case(2, 3, 1.0)
    built = _Built(pool, t)
    try:
        for l, L in enumerate(t.levels):
            L.a, L.b = L.a * 0.5, L.b * 1.25
            built.tail.set_coefficients(l, L.a, L.b)
        built.tail.run()
        rs, zs = t.ref()
        built.vec[0]["z"].expect(zs[0], "new coefficients")
        built.vec[1]["z"].expect(zs[1], "new coefficients, coarse")
    finally:
        pool.e.synchronize()
        built.tail.close()


def test_kernel_refusals_write_nothing(pool):  # noqa: F811
    t = tc.degree_case(2, 3, 1.0)

    def field(level, key, value):
        def corrupt(desc, pool):  # noqa: F811
            desc[level][key] = value(desc[level], pool) if callable(value) else value
        return corrupt

    def bad_colind(d, pool):  # noqa: F811
        ci = t.levels[1].csr[1].copy()
        ci[len(ci) // 2] = t.levels[1].n
        return pool.raw(ci.astype(np.int32))

    def bad_rowptr(d, pool):  # noqa: F811
        rp = t.levels[0].csr[0].copy()
        rp[3] = rp[-1] + 1
        return pool.raw(rp.astype(np.int32))
    cases = [("unaligned z", field(0, "z", lambda d, p: d["z"] + 4)),
             ("unaligned r", field(1, "r", lambda d, p: d["r"] + 4)),
             ("unaligned rowptr", field(0, "rowptr", lambda d, p: d["rowptr"] + 2)),
             ("NULL w", field(0, "w", None)),
             ("NULL dinv", field(1, "dinv", None)),
             ("NULL z", field(1, "z", None)),
             ("colind out of range", field(1, "colind", bad_colind)),
             ("rowptr beyond the entries", field(0, "rowptr", bad_rowptr)),
             ("rows that are not the step's", field(1, "rows", 39)),
             ("no step between the levels", field(0, "step", None)),
             ("a lane count the kernel never has", field(0, "lanes_per_row", 3))]
    for what, corrupt in cases:
        other = Pool(pool.e)
        try:
            built = _Built(other, t, corrupt)
            with pytest.raises(_lib.SpmvHipError):
                built.create()
            assert built.tail is None, what
            # no handle, so nothing to run: nothing was written
            assert _lib.hip.spmv_hip_amg_tail_run_f64(built.ctx, None, None) != 0
            other.e.synchronize()
            built.untouched(what)
        finally:
            other.close()
