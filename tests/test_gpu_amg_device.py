"""The device setup of AmgPreconditioner on the GPU: AmgOptions setup = device,
spmv_hip_amg_aggregate and spmv_hip_amg_plan_build (hip/spmv_amg_build.hip).

Everything is an equality unless it says otherwise.
  order = "natural"   the object IS the host-built one of the same matrix:
                      levels, rows, aggregates, coarse operators (pattern and
                      value bits), bounds, every array of every step's plan,
                      plan_bytes, amg_apply, and k and the history of pcg_amg
                      and gmres
  order = "hashed"    every array is the restatement's (amg_device_cases on
                      amg_cases), amg_apply is AmgRef.apply bit for bit, pcg_amg
                      stops at the restatement's k.  The history is held to the
                      bars of test_gpu_amg.py under that file's rule: dev_ref is
                      computed for the new hierarchy, and a case whose dev_ref
                      is not below a tenth of the bar asserts k, convergence and
                      the error of x only (it is printed)
  the C entries       on raw arrays: aggregates and rounds against the
                      restatement, plans from the caller's own aggregates, the
                      reason codes of refused input

The matrices are test_gpu_amg.py's."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as ac
import amg_device_cases as dc
import oracle
import test_gpu_amg as ta
import test_gpu_chebyshev as tc
import test_gpu_gmres as tg
import test_gpu_pcg as tp
from spmv_amd import _lib, hip, host
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD, KMAX, RTOL = ta.GUARD, ta.KMAX, ta.RTOL
EINVAL = -1
STEP_KEYS = ("agg", "member_ptr", "member", "src_ptr", "src")


class _Problem(ta._Problem):
    """test_gpu_amg._Problem (M: the host-built objects, ref: the restatement in
    row order) plus D[order][sym], the device-built objects, and dref[sym], the
    restatement with hashed priorities (made on first use)"""

    def __init__(self, exec_, comm, name, scaled, **options):  # noqa: F811
        super().__init__(exec_, comm, name, scaled, **options)
        self.D = {order: {sym: host.AmgPreconditioner(
            exec_, A, setup="device", order=order, **options)
            for sym, A in self.A.items()} for order in dc.ORDERS}
        self._dref = {}
        self.hashed = False

    def dref(self, sym):
        if sym not in self._dref:
            self._dref[sym] = dc.restate("hashed", ta.restate, self.csr, self.N,
                                         sym, **self.options)
        return self._dref[sym]

    def precond(self, r):  # (the references of the solves)
        return (self.dref(False) if self.hashed else self.ref[False]).apply(r)

    def close(self):
        for per in self.D.values():
            for M in per.values():
                M.close()
        super().close()


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    ps = {}

    def get(name, scaled=False, hashed=False, **options):
        key = (name, scaled, hashed, tuple(sorted(options.items())))
        if key not in ps:
            ps[key] = _Problem(exec_, comm, name, scaled, **options)
            ps[key].hashed = hashed
        return ps[key]
    yield get
    for p in ps.values():
        p.close()


OPTS = [pytest.param({}, id="defaults"),
        pytest.param({"min_coarse_rows": 20}, id="coarse20")]


def _same_objects(D, M, what):
    assert D.levels() == M.levels(), (what, D.levels(), M.levels())
    assert D.plan_bytes() == M.plan_bytes(), what
    for l in range(M.levels()):
        assert D.rows(l) == M.rows(l) and D.non_zeros(l) == M.non_zeros(l)
        assert D.lmax(l) == M.lmax(l), (what, l)
        if l + 1 < M.levels():
            assert np.array_equal(D.aggregates(l), M.aggregates(l)), (what, l)
        if l >= 1:
            for a, b in zip(D.level_matrix(l), M.level_matrix(l)):
                assert a.dtype == b.dtype and np.array_equal(
                    a.view(np.uint8), b.view(np.uint8)), (what, l)
        got, want = D.step_arrays(l), M.step_arrays(l)
        assert got.keys() == want.keys(), (what, l, got.keys(), want.keys())
        for k in want:
            assert np.array_equal(got[k], want[k]), (what, l, k)


# ---- 1. natural: the host-built object ----------------------------------------------------
@pytest.mark.parametrize("options", OPTS)
@pytest.mark.parametrize("name", ta.NAMES)
def test_natural_is_the_host_built_object(problems, name, options):
    P = problems(name, **options)
    for sym in P.storages:
        D, M = P.D["natural"][sym], P.M[sym]
        _same_objects(D, M, (name, sym, options))
        print(name, sym, options, "rows", [D.rows(l) for l in range(D.levels())],
              "rounds", [D.rounds(l) for l in range(D.levels())],
              D.setup_detail())
        assert M.rounds(0) == (0, 0) and M.setup_detail()["temp_bytes"] == 0
        if D.levels() > 1:
            assert min(D.rounds(0)) >= 1 and D.setup_detail()["temp_bytes"] > 0
        assert D.rounds(D.levels() - 1) == (0, 0)
    if name.startswith("diag"):  # a step that merges nothing
        assert P.D["natural"][False].levels() == 1
    if name == "arrow130" and options:  # one aggregate
        assert P.D["natural"][False].rows(1) == 1
    if name == "poisson11" and options:
        assert P.D["natural"][False].levels() >= 3
    if name == "poisson24" and options:  # four levels
        assert P.D["natural"][False].levels() >= 4
    if name == "ragged3001":
        st = P.D["natural"][False].step_arrays(0)
        assert np.diff(st["src_ptr"]).max() > 1024
        assert "xrow_ptr" in P.D["natural"][True].step_arrays(0)


@pytest.mark.parametrize("name", ["poisson11", "ragged3001", "convdiff8", "arrow130"])
def test_natural_apply_has_the_host_built_bits(problems, name):
    P = problems(name, min_coarse_rows=20)
    for sym in P.storages:
        for rhs in ("rand", "ones"):
            for r_off, z_off in ta.OFFSETS:  # aligned and 8 bytes off
                want = P.apply(P.rhs[rhs], sym, r_off, z_off)
                got = P.apply(P.rhs[rhs], sym, r_off, z_off,
                              M=P.D["natural"][sym])
                assert np.array_equal(got, want), (name, sym, rhs, r_off)


@pytest.mark.parametrize("name", ["poisson11", "banded4097"])
def test_natural_solves_are_the_host_built_solves(comm, problems, name):  # noqa: F811
    P = problems(name, True)
    e = P.exec_
    for sym in P.storages:
        out = []
        for M in (P.M[sym], P.D["natural"][sym]):
            e.copy_from_host(P.d_b, P.rhs["rand"])
            k, hist = host.pcg_amg(comm, e, P.A[sym], M, P.d_b, P._guarded(GUARD),
                                   KMAX, RTOL, P.ws)
            out.append((k, hist.copy(), P._read_guarded(GUARD)))
        assert out[0][0] == out[1][0] < KMAX
        assert np.array_equal(out[0][1], out[1][1])
        assert np.array_equal(out[0][2], out[1][2])
    out = []
    for M in (P.M[False], P.D["natural"][False]):
        e.copy_from_host(P.d_b, P.rhs["rand"])
        k, hist, status = host.gmres(comm, e, P.A[False], P.d_b, P._guarded(GUARD),
                                     30, tg.KMAX, tg.RTOL, amg=M, ws=P.gws)
        out.append((k, hist.copy(), status, P._read_guarded(GUARD)))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][3], out[1][3])


# ---- 2. hashed: the restatement ------------------------------------------------------------
@pytest.mark.parametrize("options", OPTS)
@pytest.mark.parametrize("name", ta.NAMES)
def test_hashed_is_the_restatement(problems, name, options):
    P = problems(name, **options)
    for sym in P.storages:
        D, ref = P.D["hashed"][sym], P.dref(sym)
        ta._same_hierarchy(D, ref, (name, sym, options, "hashed"))
        for l, L in enumerate(ref.levels):
            got = D.step_arrays(l)
            if "step" in L:
                for k in STEP_KEYS:
                    assert np.array_equal(got[k], L["step"][k]), (name, sym, l, k)
            if sym and l == 0:
                ptr, col, src = ac.expand(*L["csr"][:2], L["n"], True)
                assert np.array_equal(got["xrow_ptr"], ptr)
                assert np.array_equal(got["xrow_src"], src)
        print(name, sym, options, "rows", [L["n"] for L in ref.levels], "rounds",
              [D.rounds(l) for l in range(D.levels())])
    if name == "poisson24" and not options:  # other aggregates than the host's
        assert not np.array_equal(P.D["hashed"][False].aggregates(0),
                                  P.M[False].aggregates(0))
        assert sum(P.D["hashed"][False].rounds(0)) < \
            sum(P.D["natural"][False].rounds(0))


@pytest.mark.parametrize("name", ["poisson11", "ragged3001", "convdiff8", "arrow130"])
def test_hashed_apply_is_exact(problems, name):
    P = problems(name, min_coarse_rows=20)
    for sym in P.storages:
        want = P.dref(sym).apply(P.rhs["rand"])
        for r_off, z_off in ta.OFFSETS:
            got = P.apply(P.rhs["rand"], sym, r_off, z_off, M=P.D["hashed"][sym])
            assert np.array_equal(got, want), (name, sym, r_off)


@pytest.mark.parametrize("name", ["poisson11", "poisson24", "banded4097",
                                  "ragged3001"])
def test_hashed_pcg_amg_against_the_reference(comm, problems, name):  # noqa: F811
    P = problems(name, True, hashed=True)
    ref = P.pcg_ref("rand")
    dev_ref = ref.dev(min(ref.k, 50) + 1)
    under_the_bar = dev_ref <= 1e-7
    print(name, "hashed k_ref", ref.k, "dev_ref", dev_ref,
          "history held to the bars" if under_the_bar else
          "DROPPED from the bars: k, convergence and the error of x only")
    e = P.exec_
    e.copy_from_host(P.d_b, P.rhs["rand"])
    k, hist = host.pcg_amg(comm, e, P.A[False], P.D["hashed"][False], P.d_b,
                           P._guarded(GUARD), KMAX, RTOL, P.ws)
    x = P._read_guarded(GUARD)
    assert k == ref.k < KMAX, (name, k, ref.k)
    if under_the_bar:
        tc._vs_ref(k, hist.copy(), x, ref, P.norm_a, (name, "hashed"))
    else:
        assert len(hist) == k + 1 and hist[k] / hist[0] < RTOL
        assert np.linalg.norm(x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)


# ---- 3. the C entries on raw arrays ---------------------------------------------------------
class _Device:
    """numpy arrays on the device, through the executor"""

    def __init__(self, e):
        self.e, self.ptrs = e, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.e.alloc(max(1, (a.nbytes + 7) // 8))
        if a.nbytes:
            self.e.copy_from_host(p, a)
        self.ptrs.append(p)
        return p

    def zeros(self, count, dtype):
        return self.put(np.zeros(count, dtype))

    def get(self, p, count, dtype):
        out = np.zeros(count, dtype)  # (exactly count elements: an array the
        if count:                     # library returned is no longer than that)
            host.call("spmvh_exec_copy_to_host", self.e.h,
                      out.ctypes.data_as(C.c_void_p), p, out.nbytes)
        return out

    def close(self):
        for p in self.ptrs:
            self.e.free(p)


def _raw(e, csr, n, ncols, sym, diag, theta, order, agg=None):
    """aggregate (unless agg is given) and build on raw arrays -> dict of the
    plan's arrays, the coarse pattern, n_agg, rounds"""
    d = _Device(e)
    nnz = len(csr[1])
    rp = d.put(csr[0].astype(np.int32)) if nnz else None
    ci = d.put(csr[1].astype(np.int32)) if nnz else None
    va = d.put(csr[2].astype(np.float64)) if nnz else None
    dg = d.put(diag) if sym else None
    d_agg = d.zeros(n, np.int32)
    out = {}
    try:
        if agg is None:
            n_agg, rounds, info = hip.amg_aggregate(
                e.context, n, ncols, nnz, rp, ci, va, dg, sym, theta,
                hip.AMG_NATURAL if order == "natural" else hip.AMG_HASHED, d_agg)
            out.update(rounds=rounds, temp=int(info[1]))
            out["agg_only"] = d.get(d_agg, n, np.int32)
        else:
            n_agg = int(np.max(agg, initial=-1)) + 1
            e.copy_from_host(d_agg, np.ascontiguousarray(agg, np.int32))
        out["n_agg"] = n_agg
        c_rp = d.zeros(n_agg + 1, np.int32)
        plan = hip.AmgBuiltPlan(e.context, n, ncols, nnz, rp, ci, sym, d_agg,
                                n_agg, c_rp)
        try:
            out.update(plan.export())
            out["rowptr"] = d.get(c_rp, n_agg + 1, np.int32)
            out["colind"] = d.get(plan.coarse_colind, plan.coarse_nnz, np.int32) \
                if plan.coarse_nnz else np.zeros(0, np.int32)
            out["bytes"] = plan.bytes()
            if nnz and plan.coarse_nnz:  # the values, through the old kernel
                c_va = d.zeros(plan.coarse_nnz, np.float64)
                _lib.call("spmv_hip_amg_galerkin_f64", e.context, plan.h, va, dg,
                          c_va, None)
                e.synchronize()
                out["values"] = d.get(c_va, plan.coarse_nnz, np.float64)
        finally:
            plan.close()
    finally:
        d.close()
    return out


def _with_ghosts(csr, n, extra=5):
    """every third row gets an entry in a ghost column >= n, in front"""
    rp, ci, va = csr
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 3 == 0:
            rows.append(i), cols.append(n + i % extra), vals.append(-9.0)
        for e in range(rp[i], rp[i + 1]):
            rows.append(i), cols.append(ci[e]), vals.append(va[e])
    nrp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (nrp.astype(np.int32), np.array(cols, np.int32), np.array(vals)), \
        n + extra


RAW = [("poisson11", False, 0.25), ("poisson11", True, 0.25),
       ("duplicates", False, 0.25), ("duplicates", True, 0.0),
       ("weak_row", False, 0.25), ("weak_row", True, 1.0),
       ("arrow130", False, 0.25), ("convdiff8", False, 0.0),
       ("ragged3001", True, 0.25), ("ghosts", False, 0.25), ("empty7", False, 0.25)]


@pytest.mark.parametrize("order", dc.ORDERS)
@pytest.mark.parametrize("name,sym,theta", RAW)
def test_c_entries_on_raw_arrays(exec_, name, sym, theta, order):  # noqa: F811
    """unsorted rows, a column twice in a row, entries that are 0.0 or NaN,
    ghost columns, an empty block: the aggregates AND the rounds are the
    restatement's, the plan is amg_cases.coarsen's for those aggregates"""
    if name == "ghosts":
        base = dc.matrix("poisson5")
        n = len(base[0]) - 1
        csr, ncols = _with_ghosts(base, n)
    else:
        csr = dc.matrix(name)
        n = ncols = len(csr[0]) - 1
    st, diag = dc.storages(csr, n, sym)
    got = _raw(exec_, st, n, ncols, sym, diag, theta, order)
    ptr, col, src = ac.expand(st[0], st[1], n, sym)
    val = ac.values_of(src, st[2], diag)
    agg, n_agg, rounds = dc.aggregate_in_rounds(ptr, col, val, n, theta, order)
    want = dc.coarsen(st, n, sym, diag, theta, order)
    assert np.array_equal(agg, want["agg"])  # (the definition, once more)
    print(name, sym, theta, order, "n_agg", n_agg, "rounds", rounds,
          "temp bytes", got["temp"])
    assert got["n_agg"] == n_agg and got["rounds"] == rounds
    assert np.array_equal(got["agg_only"], agg)
    for k in STEP_KEYS + ("rowptr", "colind"):
        assert np.array_equal(got[k], want[k]), (name, sym, order, k)
    if sym:
        assert np.array_equal(got["xrow_ptr"], ptr)
        assert np.array_equal(got["xrow_src"], src)
    else:
        assert "xrow_ptr" not in got
    if "values" in got:
        c_val = ac.seq_sum(want["src_ptr"], ac.values_of(want["src"], st[2], diag))
        assert np.array_equal(got["values"], c_val, equal_nan=True)


@pytest.mark.parametrize("sym", [False, True])
def test_plan_from_the_callers_aggregates(exec_, sym):  # noqa: F811
    """aggregates no pass would make: i mod 7 (n_agg no power of two, members
    far apart), and a single aggregate"""
    csr = dc.matrix("poisson5")
    n = len(csr[0]) - 1
    st, diag = dc.storages(csr, n, sym)
    for agg in (np.arange(n) % 7, np.zeros(n, np.int64), (np.arange(n) * 7) % n):
        got = _raw(exec_, st, n, n, sym, diag, 0.25, "hashed", agg=agg)
        want = dc.coarsen(st, n, sym, diag, 0.25, "hashed", agg=agg)
        for k in STEP_KEYS + ("rowptr", "colind"):
            assert np.array_equal(got[k], want[k]), (sym, k)
        c_val = ac.seq_sum(want["src_ptr"], ac.values_of(want["src"], st[2], diag))
        assert np.array_equal(got["values"], c_val)
        # plan_bytes is the host builder's count: every array, nothing else
        size = 4 * (2 * n + want["n_agg"] + 1 + len(want["src"])) \
            + 8 * len(want["src_ptr"])
        if sym:
            size += 8 * (n + 1) + 4 * len(want["xrow_src"])
        assert got["bytes"] == size


def _live():
    """device arrays this thread's plan builders hold (plans, temporaries)"""
    n = C.c_int64()
    _lib.call("spmv_hip_plan_live_allocations", C.byref(n))
    return n.value


def test_bad_input_is_refused_with_its_reason(exec_):  # noqa: F811
    """EINVAL from the check on the device, before anything is indexed; no plan
    and no coarse array comes back, the builders' bookkeeping of live device
    arrays stands where it stood (nothing is left allocated), and a good build
    on the same context works afterwards and gives everything back on close"""
    rp, ci, va = (a.copy() for a in dc.matrix("poisson5"))
    n, nnz = len(rp) - 1, len(ci)
    good_agg = (np.arange(n) // 4).astype(np.int32)
    n_agg = int(good_agg.max()) + 1

    def build(rp_, ci_, agg_, n_agg_=n_agg):
        d = _Device(exec_)
        live = _live()
        try:
            with pytest.raises(_lib.SpmvHipError) as err:
                hip.AmgBuiltPlan(exec_.context, n, n, nnz, d.put(rp_), d.put(ci_),
                                 False, d.put(agg_), n_agg_,
                                 d.zeros(n_agg_ + 1, np.int32))
        finally:
            d.close()
        assert err.value.code == EINVAL
        assert _live() == live, "a refused call left device arrays behind"
        return int(err.value.info[0])

    def aggregate(rp_, ci_):
        d = _Device(exec_)
        live = _live()
        try:
            with pytest.raises(_lib.SpmvHipError) as err:
                hip.amg_aggregate(exec_.context, n, n, nnz, d.put(rp_), d.put(ci_),
                                  d.put(va), None, False, 0.25, hip.AMG_HASHED,
                                  d.zeros(n, np.int32))
        finally:
            d.close()
        assert err.value.code == EINVAL
        assert _live() == live, "a refused call left device arrays behind"
        return int(err.value.info[0])
    bad_rp = rp.copy()
    bad_rp[7], bad_rp[8] = rp[8], rp[7]
    short_rp = rp.copy()
    short_rp[-1] -= 1
    bad_ci = ci.copy()
    bad_ci[11] = n
    neg_ci = ci.copy()
    neg_ci[3] = -1
    for r, c, reason in ((bad_rp, ci, 1), (short_rp, ci, 1), (rp, bad_ci, 2),
                         (rp, neg_ci, 2)):
        assert build(r, c, good_agg) == reason
        assert aggregate(r, c) == reason
    high, low = good_agg.copy(), good_agg.copy()
    high[5], low[9] = n_agg, -1
    assert build(rp, ci, high) == 3 and build(rp, ci, low) == 3
    hole = good_agg.copy()
    hole[hole == 2] = 3
    assert build(rp, ci, hole) == 4
    with pytest.raises(_lib.SpmvHipError):  # theta outside [0, 1]
        d = _Device(exec_)
        try:
            hip.amg_aggregate(exec_.context, n, n, nnz, d.put(rp), d.put(ci),
                              d.put(va), None, False, 1.5, 0, d.zeros(n, np.int32))
        finally:
            d.close()
    live = _live()
    got = _raw(exec_, (rp, ci, va), n, n, False, None, 0.25, "hashed", agg=good_agg)
    assert got["n_agg"] == n_agg
    assert _live() == live  # (plan destroyed; the coarse colind was the caller's)
    hip.amg_aggregate(exec_.context, 0, 0, 0, None, None, None, None, False, 0.25,
                      0, None)
    d = _Device(exec_)
    try:
        hip.amg_aggregate(exec_.context, n, n, nnz, d.put(rp), d.put(ci), d.put(va),
                          None, False, 0.25, 0, d.zeros(n, np.int32))
    finally:
        d.close()
    assert _live() == live, "the aggregation's temporaries are all given back"


# ---- 4. after the build ----------------------------------------------------------------------
def test_options_are_checked(exec_, comm, problems):  # noqa: F811
    A = problems("poisson11").A[False]
    with pytest.raises(host.SpmvHostError, match="order"):
        host.AmgPreconditioner(exec_, A, setup="host", order="natural")
    with pytest.raises(host.SpmvHostError, match="order"):
        host.AmgPreconditioner(exec_, A, order="hashed")
    with pytest.raises(ValueError):
        host.AmgPreconditioner(exec_, A, setup="gpu")
    with pytest.raises(ValueError):
        host.AmgPreconditioner(exec_, A, setup="device", order="random")
    M = host.AmgPreconditioner(exec_, A, setup="device")  # hashed by default
    try:
        assert np.array_equal(M.aggregates(0),
                              problems("poisson11").D["hashed"][False].aggregates(0))
    finally:
        M.close()


@pytest.mark.parametrize("order", dc.ORDERS)
def test_refresh_keeps_the_aggregates(exec_, comm, order):  # noqa: F811
    """values rewritten in place: the refreshed object is the restatement with
    frozen aggregates"""
    name, opts = "poisson11", {"min_coarse_rows": 20}
    csr = tp._scaled(ta._make_csr(name))
    N = len(csr[0]) - 1
    d_r, d_z = exec_.alloc(N), exec_.alloc(N)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        M = host.AmgPreconditioner(exec_, A, setup="device", order=order, **opts)
        old = dc.restate(order, ta.restate, csr, N, sym, **opts)
        ta._same_hierarchy(M, old, (name, sym, order, "old"))
        new = ta._changed(csr, 0.05)
        r = oracle.csr_spmv(*new, np.random.default_rng(3).uniform(-1, 1, N))
        ta._write_values(exec_, A, new, sym)
        M.refresh(A)
        ref = ta.restate(new, N, sym, frozen=old, **opts)
        ta._same_hierarchy(M, ref, (name, sym, order, "refreshed"))
        exec_.copy_from_host(d_r, r)
        host.amg_apply(exec_, M, d_r, d_z)
        assert np.array_equal(exec_.copy_to_host(d_z, N), ref.apply(r))
        M.close()
        A.close()
    exec_.free(d_r), exec_.free(d_z)


def test_tail_block_cycle_and_pcg_block_take_the_object(comm, problems):  # noqa: F811
    P = problems("poisson11", min_coarse_rows=20)
    e, N, M = P.exec_, P.N, P.D["hashed"][False]
    want = P.apply(P.rhs["rand"], M=M)
    M.set_tail_rows(8192)
    try:
        assert M.tail_levels() == M.levels() - 1
        assert np.array_equal(P.apply(P.rhs["rand"], M=M), want)
    finally:
        M.set_tail_rows(0)
    nrhs = 3
    R = np.stack([P.rhs["rand"], P.rhs["ones"], -P.rhs["rand"]], axis=1)
    d_R, d_Z = e.alloc(N * nrhs), e.alloc(N * nrhs)
    try:
        e.copy_from_host(d_R, np.ascontiguousarray(R).ravel())
        host.amg_apply_block(e, M, d_R, d_Z, nrhs)
        Z = e.copy_to_host(d_Z, N * nrhs).reshape(N, nrhs)
        for c in range(nrhs):
            assert np.array_equal(Z[:, c], P.apply(R[:, c].copy(), M=M)), c
        e.copy_from_host(d_Z, np.zeros(N * nrhs))
        its, _ = host.pcg_block(comm, e, P.A[False], d_R, d_Z, nrhs, KMAX, RTOL,
                                amg=M)[:2]
        assert all(0 < k < KMAX for k in its)
    finally:
        M.release_block_scratch()
        e.free(d_R), e.free(d_Z)


def test_a_released_matrix_is_refused(comm):  # noqa: F811
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    N = len(csr[0]) - 1
    A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], False,
                                  host.P2P_BLOCKING)
    assert A.release_csr() > 0
    with pytest.raises(host.SpmvHostError, match="released"):
        host.AmgPreconditioner(e, A, setup="device")
    A.close()
    e.synchronize()
    e.close()


# ---- 5. two slab ranks ------------------------------------------------------------------------
def test_device_setup_on_two_slab_ranks():
    """Two ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking (one block with ghost columns) and an overlapping halo
    model: the device setup sees a Matrix whose block really has ghost columns.
    natural: the host-built object, its amg_apply and its pcg_amg in general storage (k,
    history and x as bits).  hashed: the per-rank restatement (hierarchy, amg_apply bit
    for bit); pcg_amg (general storage) stops at the k of the reference on
    oracle.dist_spmv with the block-diagonal hashed preconditioner, and its
    history is held to the bars only where dev_ref is below 1e-7 (printed).
    (The restatements are made before the threads start: swapping the
    aggregate function is not thread-safe.)"""
    import test_gpu_sgs as ts
    from test_gpu_bicgstab import _dot_chunked
    from thread_world import ThreadWorld
    world, opts = 2, {"min_coarse_rows": 20}
    (rp, ci, va), _ = tp._slab_inputs(8)
    N = len(rp) - 1
    norm_a = tp._norm_inf((rp, ci, va))
    b = oracle.csr_spmv(rp, ci, va, np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]), int(ranges[r + 1]))
              for r in range(world)]
    drefs = []  # per rank: {sym: the hashed restatement of the diagonal block}
    for r in range(world):
        lrp, lci, lva = (np.asarray(a) for a in blocks[r][:3])
        M = int(ranges[r + 1] - ranges[r])
        keep = lci < M
        brp = np.concatenate([[0], np.cumsum(np.bincount(
            ta.gc.row_of(lrp)[keep], minlength=M))]).astype(np.int32)
        block = (brp, np.ascontiguousarray(lci[keep]),
                 np.ascontiguousarray(lva[keep]))
        drefs.append({sym: dc.restate("hashed", ta.restate, block, M, sym, **opts)
                      for sym in (False, True)})
        assert len(drefs[r][False].levels) >= 2

    def dist_dot(dot):
        def f(u, v):
            s = 0.0
            for r in range(world):
                s += dot(u[ranges[r]:ranges[r + 1]], v[ranges[r]:ranges[r + 1]])
            return s
        return f

    def precond(v):
        return np.concatenate([drefs[r][False].apply(v[ranges[r]:ranges[r + 1]])
                               for r in range(world)])
    refs = {}
    for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
        def spmv(p, cm=cm):
            return oracle.dist_spmv(world, rp, ci, va, p, False, cm)
        refs[cm] = ts._Ref(spmv, dist_dot(oracle.ddot), dist_dot(_dot_chunked),
                           b, precond)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = blocks[rank]
        assert np.any(np.asarray(lci) >= M)  # ghost columns are there
        ws = host.AmgPcgWorkspace(exec_)
        d_b, d_r = exec_.alloc(M), exec_.alloc(M)
        d_x = exec_.alloc(M + 2 * GUARD)
        r = b[r0:r1]

        def applied(pre):
            exec_.copy_from_host(d_r, r)
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, ta.SENTINEL))
            host.amg_apply(exec_, pre, d_r, d_x + 8 * GUARD)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == ta.SENTINEL)
            assert np.all(buf[GUARD + M:] == ta.SENTINEL)
            return buf[GUARD:GUARD + M].copy()

        def solved(A, pre):
            exec_.copy_from_host(d_b, r)
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, ta.SENTINEL))
            k, hist = host.pcg_amg(comm, exec_, A, pre, d_b, d_x + 8 * GUARD,
                                   KMAX, RTOL, ws)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == ta.SENTINEL)
            assert np.all(buf[GUARD + M:] == ta.SENTINEL)
            return k, hist.copy(), buf[GUARD:GUARD + M].copy()
        for sym in (False, True):
            for cm, rf in refs.items():
                what = (rank, sym, cm)
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                H = host.AmgPreconditioner(exec_, A, **opts)
                Dn = host.AmgPreconditioner(exec_, A, setup="device",
                                            order="natural", **opts)
                Dh = host.AmgPreconditioner(exec_, A, setup="device", **opts)
                _same_objects(Dn, H, what)
                assert np.array_equal(applied(Dn), applied(H)), what
                ta._same_hierarchy(Dh, drefs[rank][sym], what)
                assert np.array_equal(applied(Dh), drefs[rank][sym].apply(r)), what
                if sym:  # (the solves: general storage, as test_gpu_amg's)
                    for h in (H, Dn, Dh, A):
                        h.close()
                    continue
                # (every rank takes the three solves in the same order)
                kh, hh, xh = solved(A, H)
                kn, hn, xn = solved(A, Dn)
                assert kn == kh < KMAX and np.array_equal(hn, hh), what
                assert np.array_equal(xn, xh), what
                k, hist, x = solved(A, Dh)
                ks = tw.gather(rank, np.array([k]))
                xs = tw.gather(rank, x)
                assert np.all(ks == k) and k < KMAX, ks
                dev_ref = rf.dev(min(rf.k, 50) + 1)
                print(what, "hashed k", k, "k_ref", rf.k, "dev_ref", dev_ref)
                assert k == rf.k, (what, k, rf.k)
                if dev_ref <= 1e-7:
                    tc._vs_ref(k, hist, xs, rf, norm_a, what)
                else:  # dropped from the history bar, not widened
                    assert hist[k] / hist[0] < RTOL
                    err = np.linalg.norm(xs - rf.x) / np.linalg.norm(rf.x)
                    assert err <= 1e-8, (what, err)
                for h in (H, Dn, Dh, A):
                    h.close()
        for p in (d_b, d_r, d_x):
            exec_.free(p)
        ws.close()

    tw.run(rank_body, gpu=True)
