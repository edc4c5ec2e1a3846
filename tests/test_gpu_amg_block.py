"""spmv::amg_apply_block on the device: the V-cycle for 1..8 interleaved
right-hand sides.

The criterion is exact: column c of Z = amg_apply_block(R) is np.array_equal to
amg_apply on column c of R on the device, and to the numpy restatement
(amg_cases.AmgRef.apply through test_gpu_amg.restate) -- for every nrhs, aligned
and 8 bytes off, both storages, whatever the other columns hold.

Matrices and problems are test_gpu_amg's (imported, not copied): Poisson 11^3
and 24^3, banded4097, ragged3001 (its second level, 77 rows and 5 507 entries,
takes the sub-wavefront product: the block cycle must keep that order), the
arrow matrix (one aggregate of 130 members), diag200 and diag1 (one level).

R and Z sit between guard words; Z is filled with a sentinel before every call,
and R is read back unchanged."""
import numpy as np
import pytest

import amg_cases as ac
import test_gpu_amg as ta
import test_gpu_pcg as tp
from spmv_amd import host
from test_gpu_pcg import comm, exec_  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tp.SENTINEL, tp.GUARD
OFFSETS = ((0, GUARD), (1, GUARD + 1))
MAXW = 8


def columns(P):
    """eight right-hand sides of different size and sign (computed once)"""
    if not hasattr(P, "block_cols"):
        rng = np.random.default_rng(P.N + 7)
        cols = [P.rhs["rand"], P.rhs["ones"]]
        for j in range(6):
            cols.append(P.spmv(rng.uniform(-1, 1, P.N)) * (-3.0) ** j)
        P.block_cols = np.stack(cols, axis=1)
        P.block_single = {}
    return P.block_cols


class Buffers:
    """device R and Z of a problem, wide enough for 8 columns"""

    def __init__(self, e, N):
        self.e, self.N = e, N
        self.d_r = e.alloc(N * MAXW + 1)
        self.d_z = e.alloc(N * MAXW + 2 * GUARD)

    def apply(self, M, R, r_off=0, z_off=GUARD, finite=True):
        e, (N, nrhs) = self.e, R.shape
        flat = np.ascontiguousarray(R).reshape(-1)
        e.copy_from_host(self.d_r + 8 * r_off, flat)
        e.copy_from_host(self.d_z, np.full(N * MAXW + 2 * GUARD, SENTINEL))
        host.amg_apply_block(e, M, self.d_r + 8 * r_off, self.d_z + 8 * z_off,
                             nrhs)
        buf = e.copy_to_host(self.d_z, N * MAXW + 2 * GUARD)
        assert np.all(buf[:z_off] == SENTINEL), "guard in front"
        assert np.all(buf[z_off + N * nrhs:] == SENTINEL), "guard behind"
        back = e.copy_to_host(self.d_r + 8 * r_off, N * nrhs)
        assert np.array_equal(back, flat, equal_nan=True), "R changed"
        Z = buf[z_off:z_off + N * nrhs].reshape(N, nrhs).copy()
        if finite:
            assert np.all(np.isfinite(Z)) and not np.any(Z == SENTINEL)
        return Z

    def close(self):
        self.e.free(self.d_r), self.e.free(self.d_z)


def buffers(P):
    if not hasattr(P, "block_buf"):
        P.block_buf = Buffers(P.exec_, P.N)
    return P.block_buf


def single(P, sym, c, M=None, cache=True):
    """amg_apply on column c, on the device"""
    cols = columns(P)
    key = (sym, c)
    if not cache:
        return P.apply(cols[:, c].copy(), sym, M=M)
    if key not in P.block_single:
        P.block_single[key] = P.apply(cols[:, c].copy(), sym, M=M)
    return P.block_single[key]


@pytest.fixture(scope="module")
def problems(exec_, comm):  # noqa: F811
    ps = {}

    def get(name, scaled=False, **options):
        key = (name, scaled, tuple(sorted(options.items())))
        if key not in ps:
            ps[key] = ta._Problem(exec_, comm, name, scaled, **options)
        return ps[key]
    yield get
    for p in ps.values():
        if hasattr(p, "block_buf"):
            p.block_buf.close()
        p.close()


def _check_all_widths(P, what, widths=range(1, MAXW + 1), M=None, cache=True):
    cols, buf = columns(P), buffers(P)
    for sym in P.storages:
        pre = (M or P.M)[sym]
        for nrhs in widths:
            for r_off, z_off in OFFSETS:
                Z = buf.apply(pre, cols[:, :nrhs], r_off, z_off)
                for c in range(nrhs):
                    want = single(P, sym, c, M=pre if M else None, cache=cache)
                    assert np.array_equal(Z[:, c], want), \
                        (what, sym, nrhs, r_off, c, int(np.sum(Z[:, c] != want)))


# ---- 1. column c is amg_apply on column c ----------------------------------------------
@pytest.mark.parametrize("options", ta.OPTS)
@pytest.mark.parametrize("name", ta.SYMMETRIC + ("arrow130",))
def test_every_column_has_the_bits_of_amg_apply(problems, name, options):
    P = problems(name, False, **options)
    _check_all_widths(P, (name, options))
    # ... and of the restatement
    cols = columns(P)
    for sym in P.storages:
        for c in (0, 5):
            assert np.array_equal(single(P, sym, c), P.ref[sym].apply(cols[:, c]))


def test_the_ragged_case_has_a_level_in_the_pairwise_order(problems):
    """what makes ragged3001 the case for the product order: its second level's
    plan takes the sub-wavefront kernel, whose sum the native multi-vector
    kernel would not reproduce"""
    P = problems("ragged3001", False)
    L = P.ref[False].levels[1]
    assert (L["n"], L["nnz"]) == (77, 5507)
    assert ac.vector_lanes(L["csr"]) > 0
    ltr = ac.AmgRef(P.csr, P.N)  # every product left to right
    r = columns(P)[:, 0]
    assert np.any(ltr.apply(r) != P.ref[False].apply(r))
    _check_all_widths(P, "ragged", widths=(2, 4, 8))


@pytest.mark.parametrize("options", [
    {"smooth_degree": 1}, {"smooth_degree": 3}, {"coarse_scale": 1.6},
    {"smooth_degree": 1, "coarse_scale": 1.6, "coarse_degree": 1},
    {"max_levels": 1}, {"min_coarse_rows": 20, "smooth_degree": 3}],
    ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["poisson11", "ragged3001"])
def test_other_options(problems, name, options):
    P = problems(name, True, **options)
    if "max_levels" in options:
        assert P.M[False].levels() == 1
    _check_all_widths(P, (name, options), widths=(2, 3, 4, 8))


POISON = (np.nan, np.inf, -np.inf, 1e308, -0.0, 5e-324)


@pytest.mark.parametrize("name", ["poisson11", "ragged3001", "arrow130"])
def test_a_column_does_not_see_its_neighbours(problems, name):
    P = problems(name, False, min_coarse_rows=20)
    cols, buf = columns(P), buffers(P)
    for sym in P.storages:
        for nrhs in (2, 3, 4, 7, 8):
            for keep in (0, nrhs - 1, nrhs // 2):
                R = np.empty((P.N, nrhs))
                for c in range(nrhs):
                    R[:, c] = POISON[c % len(POISON)]
                    R[::3, c] = cols[::3, (c + 1) % MAXW]
                R[:, keep] = cols[:, keep]
                for r_off, z_off in OFFSETS:
                    Z = buf.apply(P.M[sym], R, r_off, z_off, finite=False)
                    assert np.array_equal(Z[:, keep], single(P, sym, keep)), \
                        (name, sym, nrhs, keep, r_off)


# ---- 2. the tail, refresh, the scratch ---------------------------------------------------
def test_with_a_tail_set_the_bits_and_the_tail_stay(exec_, comm):  # noqa: F811
    P = ta._Problem(exec_, comm, "poisson24", False)
    try:
        before = {sym: [single(P, sym, c) for c in range(MAXW)]
                  for sym in P.storages}
        for sym in P.storages:
            P.M[sym].set_tail_rows(8192)
            assert P.M[sym].tail_levels() == 2
        buf = buffers(P)
        for sym in P.storages:
            for nrhs in (1, 2, 5, 8):
                Z = buf.apply(P.M[sym], columns(P)[:, :nrhs])
                for c in range(nrhs):
                    assert np.array_equal(Z[:, c], before[sym][c]), (sym, nrhs, c)
            assert P.M[sym].tail_levels() == 2
            # (and the single-vector path still runs its tail, same bits)
            z = P.apply(columns(P)[:, 1].copy(), sym)
            assert np.array_equal(z, before[sym][1])
    finally:
        buffers(P).close()
        P.close()


def test_after_refresh(exec_, comm):  # noqa: F811
    name = "ragged3001"
    P = ta._Problem(exec_, comm, name, True, min_coarse_rows=20)
    try:
        buf = buffers(P)
        for sym in P.storages:
            buf.apply(P.M[sym], columns(P)[:, :4])  # scratch exists before
            new = ta._changed(P.csr, 0.05)
            ta._write_values(exec_, P.A[sym], new, sym)
            P.M[sym].refresh(P.A[sym])
            for nrhs in (2, 3, 8):
                Z = buf.apply(P.M[sym], columns(P)[:, :nrhs])
                for c in range(nrhs):
                    want = single(P, sym, c, cache=False)
                    assert np.array_equal(Z[:, c], want), (sym, nrhs, c)
            want = ta.restate(new, P.N, sym, frozen=P.ref[sym],
                              min_coarse_rows=20).apply(columns(P)[:, 0])
            assert np.array_equal(Z[:, 0], want), sym
    finally:
        buffers(P).close()
        P.close()


def test_scratch_regrows_is_reused_released_and_counted(exec_, comm):  # noqa: F811
    P = ta._Problem(exec_, comm, "poisson11", False, min_coarse_rows=20)
    try:
        M, buf, cols = P.M[False], buffers(P), columns(P)
        want = [single(P, False, c) for c in range(MAXW)]
        rows = [M.rows(l) for l in range(M.levels())]
        base = M.plan_bytes()

        def block_bytes(w):  # r, w, dd and z of every level (no ghosts here)
            return sum(rows) * 4 * 8 * w

        def check(nrhs):
            Z = buf.apply(M, cols[:, :nrhs])
            for c in range(nrhs):
                assert np.array_equal(Z[:, c], want[c]), (nrhs, c)
        check(1)                                   # amg_apply itself: no scratch
        assert M.plan_bytes() == base
        check(2)
        assert M.plan_bytes() - base >= block_bytes(2)
        check(8), check(3)                         # regrown
        grown = M.plan_bytes()
        # (beside the vectors: the columns the coarse blocks' plans keep for the
        # per-column product of a width without a native kernel)
        kept = grown - base - block_bytes(8)
        assert 0 <= kept < block_bytes(1)
        check(2), check(3), check(8)               # reused, not shrunk
        assert M.plan_bytes() == grown
        M.release_block_scratch()
        assert M.plan_bytes() == base + kept
        M.release_block_scratch()                  # nothing to free
        check(4)
        assert M.plan_bytes() == base + kept + block_bytes(4)
    finally:
        buffers(P).close()
        P.close()


# ---- 3. errors ------------------------------------------------------------------------------
def test_errors(problems):
    P = problems("poisson11", False)
    e, M, buf, N = P.exec_, P.M[False], buffers(P), P.N
    for nrhs in (0, 9, -1):
        with pytest.raises(host.SpmvHostError, match="nrhs"):
            host.amg_apply_block(e, M, buf.d_r, buf.d_z, nrhs)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.amg_apply_block(e, M, buf.d_z, buf.d_z, 4)
    with pytest.raises(host.SpmvHostError, match="overlaps"):
        host.amg_apply_block(e, M, buf.d_z, buf.d_z + 8 * (4 * N - 1), 4)
    host.amg_apply_block(e, M, buf.d_z, buf.d_z + 8 * 2 * N, 2)  # side by side
    e.synchronize()
    with pytest.raises(host.SpmvHostError, match="NULL"):
        host.amg_apply_block(e, M, None, buf.d_z, 2)
    with pytest.raises(host.SpmvHostError, match="NULL"):
        host.amg_apply_block(e, M, buf.d_r, None, 2)


def test_an_unusable_object_throws(exec_, comm):  # noqa: F811
    csr = tp._scaled(ta._make_csr("poisson11"))
    N = len(csr[0]) - 1
    A = host.Matrix.create_matrix(comm, exec_, *csr, N, N, [], [], False,
                                  host.P2P_NONBLOCKING)
    M = host.AmgPreconditioner(exec_, A)
    d_r, d_z = exec_.alloc(4 * N), exec_.alloc(4 * N)
    try:
        on = np.flatnonzero(csr[1] == tp._row_of(csr[0])[:len(csr[1])])
        bad = (csr[0], csr[1], csr[2].copy())
        bad[2][on[5]] = -1.0
        ta._write_values(exec_, A, bad, False)
        with pytest.raises(host.SpmvHostError, match="diagonal is not positive"):
            M.refresh(A)
        for nrhs in (1, 4):
            with pytest.raises(host.SpmvHostError, match="refresh"):
                host.amg_apply_block(exec_, M, d_r, d_z, nrhs)
        ws = host.PcgBlockWorkspace(exec_)
        with pytest.raises(host.SpmvHostError, match="refresh"):
            host.pcg_block(comm, exec_, A, d_r, d_z, 4, 10, 1e-8, amg=M,
                           workspace=ws)
        ws.close()
    finally:
        exec_.synchronize()
        exec_.free(d_r), exec_.free(d_z)
        M.close()
        A.close()
