"""The device setup of spmv::Ilu0Preconditioner: SgsOptions{setup = device} and
spmv_hip_ilu0_plan_build (hip/spmv_mcgs_build.hip).

Everything here is equality of integers or of fp64 bit patterns.  With the
natural colours the device-built object is held against the host-built one:
colours, every array of the sweep plan (values and dinv as bits, after the
factorisation), the part arrays ptr / cpos / src / slot, pattern(), factor(),
the sweeps and whole solves.  With hashed and caller-supplied colours it is
held against the numpy restatement of ilu0_device_cases.py, which
test_ilu0_device_host.py proves against the host builder.

Matrices are the smallest that reach each edge of the layout (see the table in
_SHAPES).  Unsorted columns, duplicates, one-way entries and ghost columns go
through the C entry on raw device arrays.

No test provokes a fault: every out-of-range input is one the builder's check
kernel refuses before anything is indexed with it."""
import numpy as np
import pytest

import ilu0_cases as ic
import ilu0_device_cases as idc
import oracle
import sgs_device_cases as dc
import test_gpu_pcg as tp
from spmv_amd import _lib, host
from test_gpu_ilu0 import _changed, _write_values
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)
from test_ilu0_device_host import ilu_matrix

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
EINVAL = -1
KMAX, RTOL = 200, 1e-10

# name -> symmetric pattern?   the edge it reaches
_SHAPES = {
    "poisson11": True,    # two colours, many slices
    "poisson24": True,
    "banded4097": True,   # the chain: 4097 rounds; one row past a slice boundary
    "ragged3001": True,   # 24 colours
    "clique70": True,     # 70 colours, parts of up to 69 entries (long rows)
    "arrow300": False,    # a row of 299 `before` entries: beyond the LDS slab
    "hand320": True,      # colour sizes 63 / 64 / 65 / 128
    "lonely130": True,    # a row without off-diagonal entries
    "diag200": True,      # no off-diagonal entries at all
    "diag1": True,
}


def _storages():
    return [pytest.param(n, s, id=f"{n}-{'symmetric' if s else 'general'}")
            for n, symm in _SHAPES.items() for s in ((False, True) if symm
                                                     else (False,))]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class _Case:
    """One matrix in its storages: the host-built object and, built when first
    asked for and kept, the device-built ones."""

    def __init__(self, exec_, comm, name):  # noqa: F811
        self.exec_, self.comm, self.name = exec_, comm, name
        self.csr = ilu_matrix(name)
        self.N = N = len(self.csr[0]) - 1
        self.storages = (False, True) if _SHAPES[name] else (False,)
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in self.storages}
        self.Mhost = {sym: host.Ilu0Preconditioner(exec_, A)
                      for sym, A in self.A.items()}
        self._dev = {}
        self.d_r = exec_.alloc(N + 2)
        self.d_z = exec_.alloc(N + 2 * GUARD + 2)
        rng = np.random.default_rng(N + 7)
        self.r = rng.uniform(-1, 1, N)
        self.b = oracle.csr_spmv(*self.csr, rng.uniform(-1, 1, N))

    def device(self, sym, order=None, colors=None, key=None):
        k = (sym, order, key)
        if k not in self._dev:
            self._dev[k] = host.Ilu0Preconditioner(
                self.exec_, self.A[sym], setup="device", order=order,
                colors=colors)
        return self._dev[k]

    def stored(self, sym):
        """the arrays src counts in, and the diagonal"""
        if sym:
            return dc.lower_of(self.csr)
        return self.csr, dc.diagonal_of(self.csr, self.N)

    def apply(self, M, r):
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_r, r)
        e.copy_from_host(self.d_z, np.full(N + 2 * GUARD + 1, SENTINEL))
        host.ilu0_apply(e, M, self.d_r, self.d_z + 8 * GUARD)
        buf = e.copy_to_host(self.d_z, N + 2 * GUARD + 1)
        assert np.all(buf[:GUARD] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[GUARD + N:] == SENTINEL), (self.name, "guard behind")
        return buf[GUARD:GUARD + N].copy()

    def pcg(self, M, sym):
        e = self.exec_
        e.copy_from_host(self.d_r, self.b)
        e.copy_from_host(self.d_z, np.zeros(self.N))
        k, hist = host.pcg_sgs(self.comm, e, self.A[sym], M, self.d_r, self.d_z,
                               KMAX, RTOL)
        return k, hist.copy(), e.copy_to_host(self.d_z, self.N)

    def gmres(self, M, sym):
        e = self.exec_
        e.copy_from_host(self.d_r, self.b)
        e.copy_from_host(self.d_z, np.zeros(self.N))
        k, hist, status = host.gmres(self.comm, e, self.A[sym], self.d_r,
                                     self.d_z, 30, KMAX, RTOL, sgs=M)
        return k, hist.copy(), status, e.copy_to_host(self.d_z, self.N)

    def close(self):
        for M in list(self._dev.values()) + list(self.Mhost.values()):
            M.close()
        for A in self.A.values():
            A.close()
        self.exec_.free(self.d_r), self.exec_.free(self.d_z)


@pytest.fixture(scope="module")
def cases(exec_, comm):  # noqa: F811
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(exec_, comm, name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _same_objects(c, M, H, sym, what):
    """a device-built object against a host-built one: every array and bit"""
    assert M.rows() == H.rows() == c.N and M.num_colors() == H.num_colors(), what
    assert np.array_equal(M.colors(), H.colors()), what
    assert dc.same_plan(M.plan_arrays(), H.plan_arrays()) is None, what
    assert idc.same_ilu(M.ilu_arrays(), H.ilu_arrays()) is None, what
    for got, want in zip(M.pattern(), H.pattern()):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for got, want, part in zip(M.factor(), H.factor(), "lud"):
        assert np.array_equal(_bits(got), _bits(want)), (what, part)
    assert M.negative_pivots() == H.negative_pivots(), what
    assert M.plan_bytes() == H.plan_bytes(), what
    assert np.array_equal(_bits(c.apply(M, c.r)), _bits(c.apply(H, c.r))), what


# ---- 1. natural colours: the host-built object ---------------------------------------------
@pytest.mark.parametrize("name,symmetric", _storages())
def test_natural_colours_give_the_host_built_object(cases, name, symmetric):
    c = cases(name)
    M, H = c.device(symmetric, "natural"), c.Mhost[symmetric]
    _same_objects(c, M, H, symmetric, (name, symmetric))
    # the record of the device setup
    d = M.setup_detail()
    print(name, symmetric, "rounds", M.rounds(), "colours", M.num_colors(), d)
    assert 1 <= M.rounds() <= max(c.N, 1) and H.rounds() == 0
    assert d["color_ms"] > 0 and d["build_ms"] > 0 and d["temp_bytes"] > 0
    symbolic_ms, numeric_ms = M.setup_ms()
    assert symbolic_ms > 0 and numeric_ms > 0
    if name == "banded4097":
        assert M.rounds() >= 4097
    if name == "arrow300":
        assert np.diff(M.ilu_arrays()["before"]["ptr"]).max() == 299
    if name in ("diag200", "diag1", "arrow300", "clique70"):
        return  # (no solve to speak of, or one that M = A ends at once)
    got, want = c.gmres(M, symmetric), c.gmres(H, symmetric)
    assert got[0] == want[0] and got[2] == want[2], (name, got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (name, "gmres history")
    assert np.array_equal(_bits(got[3]), _bits(want[3])), (name, "gmres x")
    got, want = c.pcg(M, symmetric), c.pcg(H, symmetric)
    assert got[0] == want[0] and 1 <= got[0] < KMAX, (name, got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (name, "pcg history")
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (name, "pcg x")


def test_the_one_argument_form_and_the_host_setup_are_the_old_constructor(cases):
    c = cases("poisson11")
    M = host.Ilu0Preconditioner(c.exec_, c.A[False], setup="host")
    try:
        _same_objects(c, M, c.Mhost[False], False, "setup=host")
        assert M.rounds() == 0 and M.setup_detail()["temp_bytes"] == 0
    finally:
        M.close()


# ---- 2. hashed colours and the caller's: the restatement -----------------------------------
def _swapped(colours, a, b):
    out = colours.copy()
    out[colours == a], out[colours == b] = b, a
    return out


def _against_the_restatement(c, M, sym, colours, what):
    csr, diag = c.stored(sym)
    plan, ilu, ref = idc.ilu_ref(csr, c.N, sym, colours)
    assert np.array_equal(M.colors(), colours), what
    assert idc.same_ilu(M.ilu_arrays(), ilu) is None, what
    fac = ref.factor(diag=diag)
    for got, want, part in zip(M.factor(), fac, "lud"):
        assert np.array_equal(_bits(got), _bits(want)), (what, part)
    assert dc.same_plan(M.plan_arrays(), idc.with_factor(plan, ilu, ref, fac)) \
        is None, what
    assert np.array_equal(_bits(c.apply(M, c.r)), _bits(ref.apply(fac, c.r))), what


@pytest.mark.parametrize("name,symmetric", _storages())
def test_hashed_and_callers_colours_give_the_restatement(cases, name, symmetric):
    c = cases(name)
    hashed, nc = dc.colour_ref(c.csr, c.N, symmetric, "hashed")
    M = c.device(symmetric, "hashed")
    assert M.num_colors() == nc and M.rounds() >= 1
    _against_the_restatement(c, M, symmetric, hashed, (name, symmetric, "hashed"))
    greedy = c.Mhost[symmetric].colors()
    ncg = int(greedy.max()) + 1
    if ncg >= 2:  # the host's colours with the first and the last swapped
        mine = _swapped(greedy, 0, ncg - 1)
        M = c.device(symmetric, colors=mine, key="swapped")
        assert M.rounds() == 0 and M.num_colors() == ncg
        _against_the_restatement(c, M, symmetric, mine, (name, symmetric, "swapped"))
    if name == "hand320":
        hand = dc.hand_coloured()[1]
        M = c.device(symmetric, colors=hand, key="hand")
        assert np.diff(M.plan_arrays()["color_start"]).tolist() == [63, 64, 65, 128]
        _against_the_restatement(c, M, symmetric, hand, (name, symmetric, "hand"))


def test_the_solvers_take_a_hashed_object(cases):
    """pcg_sgs, gmres and pcg_block converge with it on poisson24; the iteration
    counts are printed for the record, not asserted against a guess"""
    c = cases("poisson24")
    e, N = c.exec_, c.N
    for sym in (False, True):
        M, H = c.device(sym, "hashed"), c.Mhost[sym]
        k, hist, x = c.pcg(M, sym)
        kh = c.pcg(H, sym)[0]
        assert 1 <= k < KMAX and hist[k] / hist[0] < RTOL
        kg, hg, status, xg = c.gmres(M, sym)
        kgh = c.gmres(H, sym)[0]
        assert status == 0 and 1 <= kg < KMAX and hg[kg] / hg[0] < RTOL
        nrhs = 2
        d_b, d_x = e.alloc(N * nrhs), e.alloc(N * nrhs)
        try:
            e.copy_from_host(d_b, np.repeat(c.b, nrhs))
            e.copy_from_host(d_x, np.zeros(N * nrhs))
            its, bh, _ = host.pcg_block(c.comm, e, c.A[sym], d_b, d_x, nrhs, KMAX,
                                        RTOL, sgs=M)
            X = e.copy_to_host(d_x, N * nrhs).reshape(N, nrhs)
        finally:
            e.free(d_b), e.free(d_x)
        assert np.all(its < KMAX) and np.all(its >= 1)
        res = c.b - oracle.csr_spmv(*c.csr, np.ascontiguousarray(X[:, 0]))
        assert np.linalg.norm(res) <= 1e-8 * np.linalg.norm(c.b)
        print("poisson24", "symmetric" if sym else "general", "colours",
              M.num_colors(), "vs", H.num_colors(), "pcg_sgs", k, "vs", kh,
              "gmres", kg, "vs", kgh, "pcg_block", its.tolist())


# ---- 3. and 4. the C entry on raw arrays ---------------------------------------------------
def _raw_equals_the_restatement(exec_, csr, n, ncols, sym, colours,  # noqa: F811
                                threshold=64):
    rc, info, plan, ilu = idc.raw_ilu_build(_lib.hip, exec_, csr, n, ncols, sym,
                                            colours, threshold=threshold)
    assert rc == 0 and info[0] == 0 and info[1] == 0 and info[2] > 0, info
    want_plan, want_ilu, _ = idc.ilu_ref(csr, n, sym, colours, threshold)
    assert dc.same_plan(plan, want_plan) is None
    assert idc.same_ilu(ilu, want_ilu) is None
    return plan, ilu


def test_long_threshold_through_the_c_entry(exec_):  # noqa: F811
    csr = ilu_matrix("ragged3001")
    n = len(csr[0]) - 1
    for sym in (False, True):
        colours, _ = host.sgs_color(csr[0], csr[1], n, n, sym)
        plan, ilu = _raw_equals_the_restatement(exec_, csr, n, n, sym, colours, 4)
        for h in ("before", "after"):
            assert len(plan[h]["long_pos"]) > 0
            assert np.sum(ilu[h]["slot"] < 0) == len(plan[h]["long_col"])
        # ... and the plan's own arrays cost what plan_create's cost
        assert ilu["bytes"] == sum(
            ilu[h][k].nbytes for h in ("before", "after") for k, _ in idc.ILU_KEYS
        ) + 8 * (len(ilu["before"]["cpos"]) + len(ilu["after"]["cpos"])) \
            + 16 * n + 16


def test_the_empty_block_through_the_c_entry(exec_):  # noqa: F811
    csr = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    rc, info, plan, ilu = idc.raw_ilu_build(_lib.hip, exec_, csr, 0, 0, False,
                                            np.zeros(0, np.int32), num_colors=0)
    assert rc == 0 and info[1] == 0
    want_plan, want_ilu, _ = idc.ilu_ref(csr, 0, False, np.zeros(0, np.int32))
    assert dc.same_plan(plan, want_plan) is None
    assert idc.same_ilu(ilu, want_ilu) is None and ilu["bytes"] == 16


RAW = {"oneway97": dc.one_way,
       "ghosts130": lambda: dc.with_ghost_columns(dc.lonely_row(), 130)[0]}


@pytest.mark.parametrize("order", ["natural", "hashed"])
@pytest.mark.parametrize("name", sorted(RAW))
def test_raw_arrays_build_and_equal_the_restatement(exec_, name, order):  # noqa: F811
    csr = RAW[name]()
    n = len(csr[0]) - 1
    ncols = n + 5 if name == "ghosts130" else n
    colours, _ = dc.colour_ref(csr, n, False, order)
    _raw_equals_the_restatement(exec_, csr, n, ncols, False, colours)
    if name == "ghosts130":  # the ghost columns are ignored: the plan without
        plain = dc.lonely_row()
        rc, _, plan, _ = idc.raw_ilu_build(_lib.hip, exec_, plain, n, n, False,
                                           colours)
        assert rc == 0
        assert dc.same_plan(plan, idc.ilu_ref(csr, n, False, colours)[0]) is None


def test_unsorted_columns_build_and_duplicates_are_refused(exec_, comm):  # noqa: F811
    # unsorted columns, every column once: the duplicates of the generator taken out
    rp, ci, va = dc.unsorted_duplicates()
    n = len(rp) - 1
    rows = dc._row_of(rp)
    _, first = np.unique(rows * n + ci, return_index=True)
    first.sort()
    once = dc.from_triplets(n, rows[first], ci[first], va[first])
    assert np.any(np.diff(once[1]) < 0)
    for sym in (False, True):
        for order in ("natural", "hashed"):
            colours, _ = dc.colour_ref(once, n, sym, order)
            _raw_equals_the_restatement(exec_, once, n, n, sym, colours)
    # a column twice in a row; symmetric storage: a stored lower entry twice, so
    # the row sees two stored entries and its column's row two mirror images
    for (csr, row), sym in ((idc.duplicate_general(), False),
                            (idc.duplicate_mirrored(), True),
                            ((dc.unsorted_duplicates(), None), False),
                            ((dc.unsorted_duplicates(), None), True)):
        m = len(csr[0]) - 1
        colours, _ = dc.colour_ref(csr, m, sym, "natural")
        rc, info, plan, ilu = idc.raw_ilu_build(_lib.hip, exec_, csr, m, m, sym,
                                                colours)
        assert rc == EINVAL and info[1] == idc.DUPLICATE and plan is None, info
        if row is not None:
            assert info[3] == row
        # the sweep plan takes the same arrays: both copies count there
        diag = dc.diagonal_of(csr, m) + 1.0 if sym else None
        assert dc.raw_build(_lib.hip, exec_, csr, m, m, sym, colours,
                            diagonal=diag)[0] == 0
    # Through the mirror the duplicate cannot be said from here: create_matrix
    # adds the two copies into one entry, so neither setup sees a duplicate (the
    # mirror's "duplicate" message for SPMV_HIP_ILU0_DUPLICATE is reached from
    # C++ callers that hand over their own arrays).  What CAN be held: the
    # merged matrix builds on both paths, and to the same object.
    csr, row = idc.duplicate_general()
    m = len(csr[0]) - 1
    A = host.Matrix.create_matrix(comm, exec_, *csr, m, m, [], [], False,
                                  host.P2P_NONBLOCKING)
    try:
        assert A.blocks()["local"][2] == len(csr[1]) - 1  # merged
        H = host.Ilu0Preconditioner(exec_, A)
        M = host.Ilu0Preconditioner(exec_, A, setup="device", order="natural")
        assert idc.same_ilu(M.ilu_arrays(), H.ilu_arrays()) is None
        for got, want in zip(M.factor(), H.factor()):
            assert np.array_equal(_bits(got), _bits(want))
        M.close(), H.close()
    finally:
        A.close()


# ---- 5. bad structure and bad colours ------------------------------------------------------
def test_bad_structure_and_bad_colours_are_refused(cases):
    c = cases("poisson11")
    e, n = c.exec_, c.N
    rp, ci, va = c.csr
    parity = c.Mhost[False].colors()
    improper = parity.copy()
    improper[5] = 1 - improper[5]
    tries = [
        ("column >= num_cols", 2, rp, np.where(np.arange(len(ci)) == 77, n, ci), parity, None),
        ("negative column", 2, rp, np.where(np.arange(len(ci)) == 9, -1, ci), parity, None),
        ("rowptr not monotone", 1, np.where(np.arange(n + 1) == 40, rp[39] - 1, rp), ci, parity, None),
        ("rowptr past nnz", 1, np.where(np.arange(n + 1) == n, len(ci) + 3, rp), ci, parity, None),
        ("colour out of range", 3, rp, ci, parity, 1),
        ("unworn colour", 4, rp, ci, parity * 2, None),
        ("improper colouring", 5, rp, ci, improper, None),
    ]
    for what, code, brp, bci, colours, nc in tries:
        bad = (brp.astype(np.int32), bci.astype(np.int32), va)
        rc, info, plan, ilu = idc.raw_ilu_build(_lib.hip, e, bad, n, n, False,
                                                colours, num_colors=nc)
        assert rc == EINVAL and info[1] == code and plan is None, (what, info)
        if code == 5:
            assert info[3] == 4  # the smallest row of the clash: 5's neighbour
    # ... and a build on the same executor still works and costs the same
    rc, info, plan, ilu = idc.raw_ilu_build(_lib.hip, e, c.csr, n, n, False, parity)
    assert rc == 0
    assert ilu["total_bytes"] + 8 * n == c.Mhost[False].plan_bytes()
    # through the mirror, with the messages of the SGS setup
    for colours, msg in ((improper, "not proper"), (parity * 2, "colour"),
                         (np.where(np.arange(n) == 0, -1, parity), "colour")):
        with pytest.raises(host.SpmvHostError, match=msg):
            host.Ilu0Preconditioner(e, c.A[False], setup="device", colors=colours)
    with pytest.raises(host.SpmvHostError, match="neither colors nor an order"):
        host.Ilu0Preconditioner(e, c.A[False], setup="host", colors=parity)


# ---- 6. pivots -----------------------------------------------------------------------------
def test_pivots_are_the_factorisations_business(exec_, comm):  # noqa: F811
    """2 x 2 blocks [[a, 1], [1, b]]: the second pivot is b - 1 / a.  A zero
    DIAGONAL entry builds on the device and fails in the factorisation, like
    on the host"""
    n = 64
    i = np.arange(n // 2)
    rows = np.concatenate([2 * i, 2 * i + 1, 2 * i, 2 * i + 1])
    cols = np.concatenate([2 * i, 2 * i + 1, 2 * i + 1, 2 * i])
    order = np.lexsort((cols, rows))
    rp = np.arange(0, 2 * n + 1, 2).astype(np.int32)
    ci = cols[order].astype(np.int32)

    def values(a, b):
        return np.concatenate([a, b, np.ones(n)])[order]

    a = np.full(n // 2, 2.0)
    a_zero = a.copy()
    a_zero[7] = 0.0  # a diagonal entry that is zero
    b = np.full(n // 2, 3.0)
    b_neg = b.copy()
    b_neg[[3, 9]] = 0.25  # 0.25 - 0.5 < 0
    d_b, d_x = exec_.alloc(n), exec_.alloc(n)
    exec_.copy_from_host(d_b, np.ones(n))
    for sym in (False, True):
        A_zero, A_neg = (host.Matrix.create_matrix(
            comm, exec_, rp, ci, va, n, n, [], [], sym, host.P2P_NONBLOCKING)
            for va in (values(a_zero, b), values(a, b_neg)))
        for kw in (dict(), dict(setup="device"), dict(setup="device", order="natural")):
            with pytest.raises(host.SpmvHostError, match="pivot") as err:
                host.Ilu0Preconditioner(exec_, A_zero, **kw)
            assert "diagonal" not in str(err.value)
        H = host.Ilu0Preconditioner(exec_, A_neg)
        M = host.Ilu0Preconditioner(exec_, A_neg, setup="device", order="natural")
        assert M.negative_pivots() == H.negative_pivots() == 2
        for got, want in zip(M.factor(), H.factor()):
            assert np.array_equal(_bits(got), _bits(want))
        hists = []
        for P in (M, H):
            with pytest.raises(host.SpmvHostError, match="pivot"):
                host.pcg_sgs(comm, exec_, A_neg, P, d_b, d_x, 10, 1e-10)
            exec_.copy_from_host(d_x, np.zeros(n))
            k, hist, status = host.gmres(comm, exec_, A_neg, d_b, d_x, 30, 50,
                                         1e-10, sgs=P)
            assert status in (0, 1) and k <= 2 and hist[k] / hist[0] < 1e-10
            hists.append((k, status, _bits(hist[:k + 1]).tolist()))
        assert hists[0] == hists[1]
        for obj in (M, H, A_zero, A_neg):
            obj.close()
    exec_.free(d_b), exec_.free(d_x)


# ---- 7. refactor ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "hashed"])
def test_refactor_on_a_device_built_object(exec_, comm, order):  # noqa: F811
    csr = tp._scaled(ilu_matrix("ragged3001"))
    new = _changed(csr)
    N = len(csr[0]) - 1
    r = np.random.default_rng(3).uniform(-1, 1, N)
    d_r, d_z = exec_.alloc(N), exec_.alloc(N)
    exec_.copy_from_host(d_r, r)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        M = host.Ilu0Preconditioner(exec_, A, setup="device", order=order)
        old = M.factor()
        _write_values(exec_, A, new, sym)
        M.refactor(A)
        A2 = host.Matrix.create_matrix(comm, exec_, *new, N, N, [], [], sym,
                                       host.P2P_NONBLOCKING)
        fresh = host.Ilu0Preconditioner(exec_, A2, setup="device", order=order)
        got = M.factor()
        for g, w, part in zip(got, fresh.factor(), "lud"):
            assert np.array_equal(_bits(g), _bits(w)), (sym, part)
        assert np.any(got[2] != old[2]) and np.any(got[2] != 2.0 * old[2])
        assert dc.same_plan(M.plan_arrays(), fresh.plan_arrays()) is None
        assert idc.same_ilu(M.ilu_arrays(), fresh.ilu_arrays()) is None
        host.ilu0_apply(exec_, fresh, d_r, d_z)
        want = exec_.copy_to_host(d_z, N)
        exec_.copy_from_host(d_z, np.full(N, SENTINEL))
        host.ilu0_apply(exec_, M, d_r, d_z)
        assert np.array_equal(_bits(exec_.copy_to_host(d_z, N)), _bits(want))
        for obj in (fresh, A2, M, A):
            obj.close()
    exec_.free(d_r), exec_.free(d_z)


# ---- 8. what the block rules refuse --------------------------------------------------------
def test_a_released_matrix_is_refused_and_release_afterwards_is_fine(comm):  # noqa: F811
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(tp._csr("banded4097"))
    N = len(csr[0]) - 1
    r = oracle.gaussian_x_fast(N)
    d_r, d_z = e.alloc(N), e.alloc(N)
    e.copy_from_host(d_r, r)
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        M = host.Ilu0Preconditioner(e, A, setup="device")
        host.ilu0_apply(e, M, d_r, d_z)
        want = e.copy_to_host(d_z, N)
        arrays = M.ilu_arrays()
        assert A.release_csr() > 0
        e.copy_from_host(d_z, np.full(N, SENTINEL))
        host.ilu0_apply(e, M, d_r, d_z)  # owns its copy
        assert np.array_equal(_bits(e.copy_to_host(d_z, N)), _bits(want)), sym
        assert idc.same_ilu(M.ilu_arrays(), arrays) is None
        with pytest.raises(host.SpmvHostError, match="released"):
            M.refactor(A)
        for kw in (dict(setup="device"), dict(setup="device", order="natural"),
                   dict()):
            with pytest.raises(host.SpmvHostError, match="released"):
                host.Ilu0Preconditioner(e, A, **kw)
        M.close()
        A.close()
    e.free(d_r), e.free(d_z)
    e.synchronize()
    e.close()


def test_rows_and_owned_columns_must_be_the_same_range(exec_, comm):  # noqa: F811
    """10 rows that own 12 columns: refused with the host path's message"""
    n, ncols = 10, 12
    rp = np.arange(n + 1).astype(np.int32)
    ci = np.arange(n).astype(np.int32)
    A = host.Matrix.create_matrix(comm, exec_, rp, ci, np.full(n, 2.0), n, ncols,
                                  [], [], False, host.P2P_NONBLOCKING)
    try:
        for kw in (dict(), dict(setup="device"), dict(setup="device", order="natural")):
            with pytest.raises(host.SpmvHostError, match="same index range"):
                host.Ilu0Preconditioner(exec_, A, **kw)
    finally:
        A.close()


# ---- 9. slab ranks -------------------------------------------------------------------------
def test_device_setup_on_two_slab_ranks():
    """Two ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages: each rank's device-built object (natural colours) is its
    host-built one, and the two pcg_sgs solves agree bit for bit."""
    from thread_world import ThreadWorld
    world = 2
    (rp, ci, va), diag = tp._slab_inputs(8)
    N = len(rp) - 1
    b_glob = oracle.csr_spmv(rp, ci, va,
                             np.random.default_rng(world).uniform(-1, 1, N))
    ranges = oracle.owner_ranges(world, N)
    tw = ThreadWorld(world, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
        M = r1 - r0
        lrp, lci, lva, gh = oracle.localise_rows(rp, ci, va, r0, r1)
        d_b, d_x = exec_.alloc(M), exec_.alloc(M)
        exec_.copy_from_host(d_b, b_glob[r0:r1])
        for sym in (False, True):
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [], gh,
                                          sym, host.P2P_NONBLOCKING)
            H = host.Ilu0Preconditioner(exec_, A)
            D = host.Ilu0Preconditioner(exec_, A, setup="device", order="natural")
            what = (rank, sym)
            assert np.array_equal(D.colors(), H.colors()), what
            assert dc.same_plan(D.plan_arrays(), H.plan_arrays()) is None, what
            assert idc.same_ilu(D.ilu_arrays(), H.ilu_arrays()) is None, what
            for got, want in zip(D.factor(), H.factor()):
                assert np.array_equal(_bits(got), _bits(want)), what
            runs = []
            for P in (D, H):
                exec_.copy_from_host(d_x, np.zeros(M))
                k, hist = host.pcg_sgs(comm, exec_, A, P, d_b, d_x, 100, 1e-10)
                runs.append((k, _bits(hist).tolist(),
                             _bits(exec_.copy_to_host(d_x, M)).tolist()))
            assert runs[0] == runs[1] and 1 <= runs[0][0] < 100, what
            D.close(), H.close(), A.close()
        exec_.free(d_b), exec_.free(d_x)

    tw.run(rank_body, gpu=True)
