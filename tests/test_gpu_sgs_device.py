"""The device setup of spmv::SgsPreconditioner: SgsOptions{setup = device},
spmv_hip_mcgs_color and spmv_hip_mcgs_plan_build (hip/spmv_mcgs_build.hip).

Everything here is equality.  The colouring is held against host.sgs_color
(natural) and the sequential restatement of sgs_device_cases.py (hashed); the
plan, array by array and dinv as bits, against the plan of the host-built
object (natural colours) and against the numpy plan restatement (hashed and
caller-supplied colours); the sweeps against test_gpu_sgs.Sweeps driven by the
object's colours and against the host-built object.  The restatements are
proved against the host builder in test_sgs_device_host.py.

Matrices are the smallest that reach each edge: see sgs_device_cases.py and
test_gpu_sgs.py (their generators are imported).  Unsorted columns, duplicate
columns and ghost columns go through the C entries on raw device arrays --
create_matrix may normalise what it is given.

No test provokes a fault: every out-of-range input is one the builder's check
kernel refuses before anything is indexed with it."""
import numpy as np
import pytest

import gmres_cases as gc
import oracle
import sgs_device_cases as dc
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
import test_gpu_sgs as ts
from spmv_amd import _lib, host
from test_gpu_bicgstab import _dot_chunked
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)
from test_sgs_device_host import matrix

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
EINVAL = -1
SHAPES = ("poisson11", "poisson24", "banded4097")
OTHERS = ("ragged3001", "diag200", "diag1", "lonely130", "clique70", "hand320")
STORAGE = [pytest.param(False, id="general"), pytest.param(True, id="symmetric")]


class _Case:
    """One matrix in both storages: the host-built object and, built when first
    asked for and kept, the device-built ones."""

    def __init__(self, exec_, comm, name, scaled):  # noqa: F811
        self.exec_, self.name = exec_, (name, scaled)
        csr = matrix(name)
        self.csr = tp._scaled(csr) if scaled else csr
        self.N = N = len(self.csr[0]) - 1
        self.A = {sym: host.Matrix.create_matrix(
            comm, exec_, *self.csr, N, N, [], [], sym, host.P2P_NONBLOCKING)
            for sym in (False, True)}
        self.Mhost = {sym: host.SgsPreconditioner(exec_, A)
                      for sym, A in self.A.items()}
        self._dev, self._host_arrays = {}, {}
        self.d_r = exec_.alloc(4 * N + 2)
        self.d_z = exec_.alloc(4 * N + 2 * GUARD + 2)

    def device(self, sym, order=None, colors=None, key=None):
        k = (sym, order, key)
        if k not in self._dev:
            self._dev[k] = host.SgsPreconditioner(
                self.exec_, self.A[sym], setup="device", order=order,
                colors=colors)
        return self._dev[k]

    def host_arrays(self, sym):
        if sym not in self._host_arrays:
            self._host_arrays[sym] = self.Mhost[sym].plan_arrays()
        return self._host_arrays[sym]

    def apply(self, M, r, r_off=0, z_off=GUARD):
        """sgs_apply between guard words -> z; r is read back unchanged"""
        e, N = self.exec_, self.N
        e.copy_from_host(self.d_r + 8 * r_off, r)
        e.copy_from_host(self.d_z, np.full(N + 2 * GUARD + 1, SENTINEL))
        host.sgs_apply(e, M, self.d_r + 8 * r_off, self.d_z + 8 * z_off)
        buf = e.copy_to_host(self.d_z, N + 2 * GUARD + 1)
        assert np.all(buf[:z_off] == SENTINEL), (self.name, "guard in front")
        assert np.all(buf[z_off + N:] == SENTINEL), (self.name, "guard behind")
        assert np.array_equal(e.copy_to_host(self.d_r + 8 * r_off, N), r)
        return buf[z_off:z_off + N].copy()

    def close(self):
        for M in list(self._dev.values()) + list(self.Mhost.values()):
            M.close()
        for A in self.A.values():
            A.close()
        self.exec_.free(self.d_r), self.exec_.free(self.d_z)


@pytest.fixture(scope="module")
def cases(exec_, comm):  # noqa: F811
    made = {}

    def get(name, scaled=False):
        if (name, scaled) not in made:
            made[(name, scaled)] = _Case(exec_, comm, name, scaled)
        return made[(name, scaled)]

    yield get
    for c in made.values():
        c.close()


_refs = {}


def colours_ref(name, sym, order):
    """the restatement's colours, computed once"""
    k = (name, sym, order)
    if k not in _refs:
        csr = matrix(name)
        _refs[k] = dc.colour_ref(csr, len(csr[0]) - 1, sym, order)
    return _refs[k]


# ---- 1. the colouring -----------------------------------------------------------------
def _colouring_cases():
    """every matrix in both storages; the one-way pattern in general storage
    (symmetric storage would drop half of it)"""
    out = [pytest.param(n, s, id=f"{n}-{'symmetric' if s else 'general'}")
           for n in SHAPES + OTHERS for s in (False, True)]
    return out + [pytest.param("oneway97", False, id="oneway97-general")]


@pytest.mark.parametrize("name,symmetric", _colouring_cases())
def test_colouring(cases, name, symmetric):
    c = cases(name)
    n, csr = c.N, c.csr
    want, nc = host.sgs_color(csr[0], csr[1], n, n, symmetric)
    M = c.device(symmetric, "natural")
    print(name, symmetric, "natural: rounds", M.rounds(), "colours", nc)
    assert M.rows() == n and M.num_colors() == nc
    assert np.array_equal(M.colors(), want)
    assert 1 <= M.rounds() <= n
    want, nc = colours_ref(name, symmetric, "hashed")
    M = c.device(symmetric, "hashed")
    print(name, symmetric, "hashed: rounds", M.rounds(), "colours", nc)
    assert M.num_colors() == nc and np.array_equal(M.colors(), want)
    assert 1 <= M.rounds() <= n
    if name == "clique70":
        assert nc == 70
    if name == "ragged3001":
        assert host.sgs_color(csr[0], csr[1], n, n, symmetric)[1] == 24


def test_default_order_of_the_device_setup_is_hashed(cases):
    c = cases("poisson11")
    M = c.device(False, None)
    assert np.array_equal(M.colors(), colours_ref("poisson11", False, "hashed")[0])
    assert M.num_colors() == 6 and c.Mhost[False].num_colors() == 2


RAW = {"unsorted150": dc.unsorted_duplicates, "oneway97": dc.one_way,
       "ghosts130": lambda: dc.with_ghost_columns(dc.lonely_row(), 130)[0],
       "clique70": dc.clique}


@pytest.mark.parametrize("order", ["natural", "hashed"])
@pytest.mark.parametrize("name", sorted(RAW))
def test_colouring_and_plan_on_raw_arrays(exec_, name, order):  # noqa: F811
    """unsorted columns, a column twice in a row, one-way entries, ghost
    columns >= num_rows: the C entries on the arrays as they are"""
    csr = RAW[name]()
    n = len(csr[0]) - 1
    ncols = n + 5 if name == "ghosts130" else n
    syms = (False,) if name == "ghosts130" else (False, True)
    for sym in syms:
        rc, colours, nc, rounds = dc.raw_color(_lib.hip, exec_, csr, n, ncols, sym,
                                               order)
        assert rc == 0
        want, nc_want = dc.colour_ref(csr, n, sym, order)
        assert nc == nc_want and np.array_equal(colours, want), (name, sym)
        assert 1 <= rounds <= n
        if order == "natural":
            assert np.array_equal(
                colours, host.sgs_color(csr[0], csr[1], n, n, sym)[0])
        diag = dc.diagonal_of(csr, n) + 1.0 if sym else None
        rc, info, got = dc.raw_build(_lib.hip, exec_, csr, n, ncols, sym, colours,
                                     diagonal=diag)
        assert rc == 0 and info[0] == 0 and info[2] > 0, (name, sym, info)
        assert dc.same_plan(got, dc.plan_ref(csr, n, sym, want, diag)) is None, (
            name, sym)


def test_long_threshold_on_raw_arrays(exec_):  # noqa: F811
    """a threshold other than the mirror's 64: rows of 2 entries are long"""
    csr = dc.lonely_row()
    n = len(csr[0]) - 1
    colours, _ = dc.colour_ref(csr, n, False, "natural")
    rc, info, got = dc.raw_build(_lib.hip, exec_, csr, n, n, False, colours,
                                 threshold=1)
    assert rc == 0
    perm, start, parts = dc.parts_ref(csr, n, False, colours)
    want = dict(perm=perm, color_start=start, dinv=1.0 / dc.diagonal_of(csr, n))
    for h, (ptr, col, val) in zip(("before", "after"), parts):
        want[h] = dc.slice_part(start, ptr, col, val, 1)[0]
    assert len(want["before"]["long_pos"]) + len(want["after"]["long_pos"]) > 0
    assert dc.same_plan(got, want) is None


# ---- 2. the plan with the natural colours: the host builder's ---------------------------
def _plan_cases():
    out = [(s, sc) for s in SHAPES for sc in (False, True)]
    return out + [(s, False) for s in OTHERS]


@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("name,scaled", _plan_cases())
def test_plan_with_natural_colours_is_the_host_plan(cases, name, scaled, symmetric):
    c = cases(name, scaled)
    M = c.device(symmetric, "natural")
    assert dc.same_plan(M.plan_arrays(), c.host_arrays(symmetric)) is None
    # 9. the accounting
    assert M.plan_bytes() == c.Mhost[symmetric].plan_bytes()
    assert M.setup_ms() > 0 and c.Mhost[symmetric].setup_ms() > 0
    assert c.Mhost[symmetric].rounds() == 0
    d = M.setup_detail()
    assert d["color_ms"] > 0 and d["build_ms"] > 0 and d["temp_bytes"] > 0


# ---- 3. the plan with other colours: the restatement -----------------------------------
def _parity(n3):
    i = np.arange(n3 ** 3)
    return ((i % n3 + (i // n3) % n3 + i // (n3 * n3)) % 2).astype(np.int32)


def _swapped(colours, a=0, b=1):
    out = colours.copy()
    out[colours == a], out[colours == b] = b, a
    return out


def _other_colours(name):
    csr = matrix(name)
    n = len(csr[0]) - 1
    if name.startswith("poisson"):
        return "parity", _parity(int(name[7:]))
    if name == "hand320":
        return "hand", dc.hand_coloured()[1]
    greedy, nc = host.sgs_color(csr[0], csr[1], n, n, False)
    return "swapped", _swapped(greedy, 0, nc - 1)


@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("name", ["poisson11", "poisson24", "banded4097",
                                  "ragged3001", "clique70", "hand320"])
def test_plan_with_other_colours_is_the_restatement(cases, name, symmetric):
    c = cases(name)
    d = tp._diag_of(c.csr)
    hashed = colours_ref(name, symmetric, "hashed")[0]
    M = c.device(symmetric, "hashed")
    assert dc.same_plan(M.plan_arrays(),
                        dc.plan_ref(c.csr, c.N, symmetric, hashed, d)) is None
    what, colours = _other_colours(name)
    M = c.device(symmetric, colors=colours, key=what)
    assert M.rounds() == 0 and M.num_colors() == colours.max() + 1
    assert np.array_equal(M.colors(), colours)
    assert dc.same_plan(M.plan_arrays(),
                        dc.plan_ref(c.csr, c.N, symmetric, colours, d)) is None
    if name == "hand320":
        assert np.diff(M.plan_arrays()["color_start"]).tolist() == [63, 64, 65, 128]


# ---- 4. and 5. the sweeps ----------------------------------------------------------------
@pytest.mark.parametrize("symmetric", STORAGE)
@pytest.mark.parametrize("name", ["poisson11", "poisson24", "banded4097",
                                  "ragged3001", "clique70", "hand320", "diag1"])
def test_sweep_bits(cases, name, symmetric):
    c = cases(name)
    dinv = 1.0 / tp._diag_of(c.csr)
    r = oracle.csr_spmv(*c.csr, np.random.default_rng(c.N).uniform(-1, 1, c.N))
    objects = [c.device(symmetric, "hashed"), c.device(symmetric, "natural")]
    if name != "diag1":
        what, colours = _other_colours(name)
        objects.append(c.device(symmetric, colors=colours, key=what))
    for M in objects:
        want = ts.Sweeps(c.csr, c.N, M.colors(), symmetric).apply(dinv, r)
        for r_off, z_off in ts.OFFSETS:
            z = c.apply(M, r, r_off, z_off)
            assert np.array_equal(z, want), (name, symmetric, r_off, z_off)
    # the natural colours: the host-built object's bits
    z_host = c.apply(c.Mhost[symmetric], r)
    assert np.array_equal(c.apply(objects[1], r), z_host)


# ---- 6. the consumers ----------------------------------------------------------------------
def test_apply_block_has_the_bits_of_apply(cases):
    c = cases("poisson11")
    e, N = c.exec_, c.N
    M = c.device(False, "hashed")
    rng = np.random.default_rng(3)
    for nrhs in (1, 3, 4):
        R = rng.uniform(-1, 1, (N, nrhs))
        e.copy_from_host(c.d_r, R.reshape(-1))
        e.copy_from_host(c.d_z, np.full(N * nrhs + 2 * GUARD, SENTINEL))
        host.sgs_apply_block(e, M, c.d_r, c.d_z + 8 * GUARD, nrhs)
        buf = e.copy_to_host(c.d_z, N * nrhs + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL)
        Z = buf[GUARD:-GUARD].reshape(N, nrhs)
        for col in range(nrhs):
            want = c.apply(M, np.ascontiguousarray(R[:, col]))
            assert np.array_equal(Z[:, col], want), (nrhs, col)


def test_pcg_sgs_and_gmres_take_the_object(cases, comm):  # noqa: F811
    c = cases("poisson11")
    e, N, A = c.exec_, c.N, c.A[False]
    M = c.device(False, "hashed")
    dinv = 1.0 / tp._diag_of(c.csr)
    sweeps = ts.Sweeps(c.csr, N, M.colors(), False)
    spmv = lambda p: oracle.csr_spmv(*c.csr, p)  # noqa: E731
    precond = lambda r: sweeps.apply(dinv, r)  # noqa: E731
    b = spmv(np.random.default_rng(N + 1).uniform(-1, 1, N))
    d_b, d_x = e.alloc(N), e.alloc(N + 2 * GUARD)
    try:
        e.copy_from_host(d_b, b)
        e.copy_from_host(d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist = host.pcg_sgs(comm, e, A, M, d_b, d_x + 8 * GUARD, ts.KMAX,
                               ts.RTOL)
        buf = e.copy_to_host(d_x, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL)
        ref = ts._Ref(spmv, oracle.ddot, _dot_chunked, b, precond)
        assert k < ts.KMAX
        tc._vs_ref(k, hist.copy(), buf[GUARD:-GUARD].copy(), ref,
                   tp._norm_inf(c.csr), ("poisson11", "hashed", "pcg_sgs"))
        # gmres with the object as right preconditioner
        x_ref, k_ref, _, status_ref = gc.gmres_ref(spmv, oracle.ddot, precond, b,
                                                   30, 200, 1e-10)
        e.copy_from_host(d_x, np.zeros(N + 2 * GUARD))
        k, hist, status = host.gmres(comm, e, A, d_b, d_x, 30, 200, 1e-10, sgs=M)
        print("gmres k", k, "k_ref", k_ref, "status", status)
        assert status == 0 and status_ref == 0 and k == k_ref
        x = e.copy_to_host(d_x, N)
        assert np.linalg.norm(x - x_ref) <= 1e-8 * np.linalg.norm(x_ref)
    finally:
        e.free(d_b), e.free(d_x)


# ---- 7. errors -------------------------------------------------------------------------------
def _good_setup(c):
    """a setup on the same executor still works"""
    M = host.SgsPreconditioner(c.exec_, c.A[False], setup="device")
    try:
        assert np.array_equal(M.colors(),
                              colours_ref(c.name[0], False, "hashed")[0])
    finally:
        M.close()


def test_colours_of_the_caller_are_checked(cases):
    c = cases("poisson11")
    e, A = c.exec_, c.A[False]
    parity = _parity(11)
    improper = parity.copy()
    improper[5] = 1 - improper[5]
    with pytest.raises(host.SpmvHostError, match="not proper"):
        host.SgsPreconditioner(e, A, setup="device", colors=improper)
    _good_setup(c)
    unworn = parity * 2  # colours 0 and 2: 1 is worn by no row
    with pytest.raises(host.SpmvHostError, match="colour"):
        host.SgsPreconditioner(e, A, setup="device", colors=unworn)
    _good_setup(c)
    negative = parity.copy()
    negative[0] = -1
    with pytest.raises(host.SpmvHostError, match="colour"):
        host.SgsPreconditioner(e, A, setup="device", colors=negative)
    _good_setup(c)
    # out of range can only be said through the C entry (the mirror derives the
    # number of colours from the largest)
    rc, info, got = dc.raw_build(_lib.hip, e, c.csr, c.N, c.N, False, parity,
                                 num_colors=1)
    assert rc == EINVAL and info[1] == 3 and got is None
    rc, info, got = dc.raw_build(_lib.hip, e, c.csr, c.N, c.N, False, improper)
    assert rc == EINVAL and info[1] == 5 and got is None
    rc, info, got = dc.raw_build(_lib.hip, e, c.csr, c.N, c.N, False, unworn)
    assert rc == EINVAL and info[1] == 4 and got is None
    _good_setup(c)


def test_bad_structure_is_refused_through_the_abi(cases):
    """a column >= num_cols, a negative column, a rowptr that is not monotone
    or does not end at nnz: SPMV_HIP_EINVAL from the check kernel, which walks
    only rows whose bounds are sound"""
    c = cases("poisson11")
    e, n = c.exec_, c.N
    rp, ci, va = c.csr
    parity = _parity(11)
    for what, code, (brp, bci) in (
            ("column >= num_cols", 2, (rp, np.where(np.arange(len(ci)) == 77, n, ci))),
            ("negative column", 2, (rp, np.where(np.arange(len(ci)) == 9, -1, ci))),
            ("rowptr not monotone", 1,
             (np.where(np.arange(n + 1) == 40, rp[39] - 1, rp), ci)),
            ("rowptr past nnz", 1,
             (np.where(np.arange(n + 1) == n, len(ci) + 3, rp), ci))):
        bad = (brp.astype(np.int32), bci.astype(np.int32), va)
        rc, _, _, _ = dc.raw_color(_lib.hip, e, bad, n, n, False, "hashed")
        assert rc == EINVAL, what
        rc, info, got = dc.raw_build(_lib.hip, e, bad, n, n, False, parity)
        assert rc == EINVAL and info[1] == code and got is None, (what, info)
    _good_setup(c)


def test_a_diagonal_that_is_not_positive_is_refused(exec_, comm):  # noqa: F811
    rp, ci, va = matrix("poisson11")
    N = len(rp) - 1
    on = np.flatnonzero(ci == tp._row_of(rp))
    bad = va.copy()
    bad[on[17]], bad[on[N - 2]], bad[on[5]] = 0.0, -6.0, np.nan
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, exec_, rp, ci, bad, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        with pytest.raises(host.SpmvHostError,
                           match=rf"diagonal is not positive \(3 of {N} "):
            host.SgsPreconditioner(exec_, A, setup="device")
        A.close()
        A = host.Matrix.create_matrix(comm, exec_, rp, ci, va, N, N, [], [], sym,
                                      host.P2P_NONBLOCKING)
        M = host.SgsPreconditioner(exec_, A, setup="device", order="natural")
        assert M.num_colors() == 2
        M.close()
        A.close()


def test_a_released_matrix_is_refused(comm):  # noqa: F811
    e = host.HipExecutor(0)
    _lib.call("spmv_hip_ctx_set_option", e.context, b"sj_min_nnz", 0)
    csr = tp._scaled(matrix("banded4097"))
    N = len(csr[0]) - 1
    for sym in (False, True):
        A = host.Matrix.create_matrix(comm, e, *csr, N, N, [], [], sym,
                                      host.P2P_BLOCKING)
        M = host.SgsPreconditioner(e, A, setup="device")
        want = M.plan_arrays()
        assert A.release_csr() > 0
        assert dc.same_plan(M.plan_arrays(), want) is None  # owns its copy
        with pytest.raises(host.SpmvHostError, match="released"):
            host.SgsPreconditioner(e, A, setup="device")
        M.close()
        A.close()
    e.synchronize()
    e.close()


# ---- 8. slab ranks ------------------------------------------------------------------------
def test_device_setup_on_slab_ranks():
    """Two ranks as threads, the scaled Poisson matrix of 8^3 in slabs, both
    storages, a blocking (one block with ghost columns) and an overlapping halo
    model, as test_gpu_sgs.test_apply_on_slab_ranks builds them."""
    from thread_world import ThreadWorld
    world = 2
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
        local = (np.asarray(lrp), np.asarray(lci), np.asarray(lva))
        r, d = r_glob[r0:r1], diag[r0:r1]
        d_r, d_z = exec_.alloc(M), exec_.alloc(M)
        exec_.copy_from_host(d_r, r)
        for sym in (False, True):
            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M,
                                              [], gh, sym, cm)
                for order in ("natural", "hashed"):
                    pre = host.SgsPreconditioner(exec_, A, setup="device",
                                                 order=order)
                    want, _ = dc.colour_ref(local, M, sym, order)
                    what = (rank, sym, cm, order)
                    assert np.array_equal(pre.colors(), want), what
                    if order == "natural":
                        assert np.array_equal(
                            want, host.sgs_color(lrp, lci, M, M, sym)[0]), what
                    assert dc.same_plan(pre.plan_arrays(), dc.plan_ref(
                        local, M, sym, want, d)) is None, what
                    exec_.copy_from_host(d_z, np.full(M, SENTINEL))
                    host.sgs_apply(exec_, pre, d_r, d_z)
                    assert np.array_equal(
                        exec_.copy_to_host(d_z, M),
                        ts.Sweeps(local, M, want, sym).apply(1.0 / d, r)), what
                    pre.close()
                A.close()
        exec_.free(d_r), exec_.free(d_z)

    tw.run(rank_body, gpu=True)
