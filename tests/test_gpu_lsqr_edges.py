"""Whole solves of host.lsqr on the cases of lsqr_edges.py: every exit on exact
block matrices a few workgroups long (square, tall and wide, with the odd
tail), the floor of scaling, poisoned data and damp and the workspace after
them, systems scaled by powers of two or negated, and two ranks.

No comparison here has a tolerance.  Every one is equality of integers (k,
status, the lengths of the histories) or lsqr_edges.same_bits.  The exact,
floor and poisoned cases are held to lsqr_cases.lsqr_ref, whose bits do not
depend on the order of a sum there (test_lsqr_edges_host.py; the three
poisoned cases where they do are held to k, status and the NaN / Inf pattern);
the scaling relations are between two GPU solves.

X sits between guard words and is filled with a sentinel before every solve;
the `nt` fixture of test_gpu_lsqr.py runs both instantiations of every vector
kernel; poll_every = 16 lets the host enqueue 16 iterations behind a stop."""
import numpy as np
import pytest

import lsqr_edges as le
import oracle
import test_gpu_lsqr as tl
from lsqr_edges import Result, same_bits
from spmv_amd import host
from test_gpu_lsqr import comm, exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = tl.SENTINEL, tl.GUARD
POLLS = (1, 16)
BY_NAME = {c.name: c for c in le.exact_cases()}


class Dev:
    """One matrix on the device with its buffers and workspace; run() is one
    guarded solve."""

    def __init__(self, exec_, comm, csr, ncols):  # noqa: F811
        self.e, self.comm, self.csr = exec_, comm, csr
        self.M, self.N = len(csr[0]) - 1, ncols
        self.A = host.Matrix.create_matrix(comm, exec_, *csr, self.M, ncols, [],
                                           [], False, host.P2P_NONBLOCKING)
        self.d_b = exec_.alloc(self.M)
        self.d_x = exec_.alloc(ncols + 2 * GUARD)
        self.ws = host.LsqrWorkspace(exec_)

    def run(self, b, kmax, rtol, ltol=0.0, damp=0.0, ws=None, what=None, **kw):
        e, N = self.e, self.N
        e.copy_from_host(self.d_b, np.asarray(b, dtype=np.float64))
        e.copy_from_host(self.d_x, np.full(N + 2 * GUARD, SENTINEL))
        k, hist_r, hist_ar, status = host.lsqr(
            self.comm, e, self.A, self.d_b, self.d_x + 8 * GUARD, kmax, rtol,
            ltol, damp, ws=ws or self.ws, **kw)
        buf = e.copy_to_host(self.d_x, N + 2 * GUARD)
        assert np.all(buf[:GUARD] == SENTINEL), (what, "guard in front")
        assert np.all(buf[GUARD + N:] == SENTINEL), (what, "guard behind")
        x = buf[GUARD:GUARD + N].copy()
        assert not np.any(x == SENTINEL), (what, "x not written")
        return Result(x, k, hist_r.copy(), hist_ar.copy(), status)

    def close(self):
        self.ws.close()
        self.A.close()
        for p in (self.d_b, self.d_x):
            self.e.free(p)


@pytest.fixture(scope="module")
def devs(exec_, comm):  # noqa: F811
    """Dev objects by key, created on first use, closed at the end"""
    made = {}

    def get(key, csr, ncols):
        if key not in made:
            made[key] = Dev(exec_, comm, csr, ncols)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _same(got, want, what):
    assert (got.k, got.status) == (want.k, want.status), \
        (what, got.k, got.status, want.k, want.status)
    assert len(got.hist) == len(got.hist_ar) == got.k + 1, (what, len(got.hist))
    assert same_bits(got.hist, want.hist), (what, got.hist[:4], want.hist[:4])
    assert same_bits(got.hist_ar, want.hist_ar), \
        (what, got.hist_ar[:4], want.hist_ar[:4])
    assert same_bits(got.x, want.x), what


def _both_polls(D, want, what, *args, weak=False, **kw):
    """the solve with poll_every = 1 and 16 against `want`, and against each
    other: nothing enqueued behind the stop moves x, the histories or status"""
    runs = []
    for poll in POLLS:
        got = D.run(*args, what=(what, poll), poll_every=poll, **kw)
        if weak:
            assert len(got.hist) == len(got.hist_ar) == got.k + 1, what
            assert le.pattern(got) == le.pattern(want), (what, poll)
        else:
            _same(got, want, (what, poll))
        runs.append(got)
    assert runs[0].same(runs[1]), what
    return runs[0]


# ---- 1. exact cases and the floor ----------------------------------------------------------
@pytest.mark.parametrize("case", le.exact_cases(), ids=lambda c: c.id)
def test_exact_cases(devs, nt, case):  # noqa: F811
    for tail in (False, True):
        csr, ncols, b = case.system(tail)
        D = devs(("exact", case.name, tail), csr, ncols)
        for kmax in case.kmaxes():
            want = le.reference(csr, ncols, b, kmax, 0.0, case.ltol, case.damp)
            assert want.same(case.want(tail)), case.id  # the table
            got = _both_polls(D, want, (case.id, tail, kmax), b, kmax, 0.0,
                              case.ltol, case.damp)
            if case.solved:
                assert same_bits(oracle.csr_spmv(*csr, got.x), b), case.id


@pytest.mark.parametrize("s", le.FLOOR_S)
@pytest.mark.parametrize("name", le.FLOOR_CASES)
def test_floor_cases(exec_, comm, nt, name, s):  # noqa: F811
    case = BY_NAME[name]
    for tail in (False, True):
        csr, ncols, b, damp, want = le.floor_case(case, s, tail)
        ref = le.reference(csr, ncols, b, le.KMAX, 0.0, case.ltol, damp)
        assert ref.same(want), (case.id, s)  # the table
        D = Dev(exec_, comm, csr, ncols)
        try:
            _both_polls(D, want, (case.id, s, tail), b, le.KMAX, 0.0, case.ltol,
                        damp)
        finally:
            D.close()


# ---- 2. poisoned data ----------------------------------------------------------------------
def _poisoned_dev(devs, shape, kind):
    csr, ncols, b, damp = le.poisoned_case(shape, kind)
    return devs((shape, "a_nan" if kind == "a_nan" else "plain"), csr,
                ncols), b, damp


@pytest.mark.parametrize("kind", le.KINDS)
@pytest.mark.parametrize("shape", le.POISON_SHAPES)
def test_poisoned_cases(devs, nt, shape, kind):  # noqa: F811
    D, b, damp = _poisoned_dev(devs, shape, kind)
    k, status, _, x_nan = le.POISON_OUTCOME[kind]
    want = le.poisoned_reference(shape, kind)
    got = _both_polls(D, want, (shape, kind), b, le.POISON_KMAX, le.POISON_RTOL,
                      le.POISON_LTOL, damp, weak=(shape, kind) in le.WEAK)
    assert (got.k, got.status) == (k, status), (shape, kind)
    if x_nan is not None:
        assert np.all(np.isnan(got.x)) if x_nan else \
            same_bits(got.x, np.zeros(D.N)), (shape, kind)
    if kind == "damp_tiny":  # the device's own solve without damp, bit for bit
        plain = D.run(b, le.POISON_KMAX, le.POISON_RTOL, le.POISON_LTOL, 0.0)
        assert np.all(np.isfinite(got.x)) and got.same(plain), shape


def test_the_workspace_after_poison_and_after_every_exit(devs, nt):  # noqa: F811
    """one LsqrWorkspace: a clean solve, then solves that leave ut, vt and w
    full of NaN, or that left through every exit on longer, taller and wider
    vectors, and after each the clean solve again -- with the bits of the
    first, and of a solve on a fresh workspace"""
    shape = "tall"
    csr, ncols = le.csr_of(shape)
    D = devs((shape, "plain"), csr, ncols)
    b = le.scaled_rhs(shape, "rand")
    ws, fresh = host.LsqrWorkspace(D.e), host.LsqrWorkspace(D.e)
    args = (b, 30, 1e-6, 1e-10, 0.5)
    try:
        first = D.run(*args, ws=ws, what="first")
        assert 1 < first.k <= 30
        assert np.all(np.isfinite(first.x)) and np.all(np.isfinite(first.hist))
        assert first.same(D.run(*args, ws=fresh))
        for kind in le.KINDS:
            P, pb, damp = _poisoned_dev(devs, shape, kind)
            bad = P.run(pb, le.POISON_KMAX, le.POISON_RTOL, le.POISON_LTOL,
                        damp, ws=ws)
            assert bad.k == le.POISON_OUTCOME[kind][0], kind
            _same(D.run(*args, ws=ws), first, ("after", kind))
        for case in le.exact_cases():
            csr2, nc2, eb = case.system(True)
            E = devs(("exact", case.name, True), csr2, nc2)
            got = E.run(eb, le.KMAX, 0.0, case.ltol, case.damp, ws=ws)
            _same(got, case.want(True), ("on the shared workspace", case.id))
            _same(D.run(*args, ws=ws), first, ("after", case.id))
    finally:
        ws.close(), fresh.close()


# ---- 3. scaling and negation -------------------------------------------------------------------
def _relation(base, got, s, t, sign, what):
    assert (got.k, got.status) == (base.k, base.status), \
        (what, got.k, got.status, base.k, base.status)
    assert len(got.hist) == len(got.hist_ar) == got.k + 1, what
    assert same_bits(got.hist, np.ldexp(base.hist, t)), what
    assert same_bits(got.hist_ar, np.ldexp(base.hist_ar, s + t)), what
    assert same_bits(got.x, sign * np.ldexp(base.x, t - s)), what
    assert np.all(np.isfinite(got.x)) and np.all(np.isfinite(base.x)), what


@pytest.mark.parametrize("shape", sorted({c[0] for c in le.SCALED}))
def test_scaled_and_negated_systems(devs, nt, shape):  # noqa: F811
    csr, ncols = le.csr_of(shape)
    K, R, L = le.SCALED_KMAX, le.SCALED_RTOL, le.SCALED_LTOL
    D = devs((shape, "plain"), csr, ncols)
    solves = [(kind, damp) for sh, kind, damp in le.SCALED if sh == shape]
    base = {}
    for kind, damp in solves:
        b = le.scaled_rhs(shape, kind)
        base[kind, damp] = D.run(b, K, R, L, damp, what=(shape, kind, damp))
        assert 1 < base[kind, damp].k <= K
        if (shape, kind) == ("tall", "rand"):  # ends by the ltol test
            assert base[kind, damp].status == 1
        _relation(base[kind, damp], D.run(-b, K, R, L, damp), 0, 0, -1.0,
                  (shape, kind, damp, "-b"))
    for s in sorted({s for s, _ in le.PAIRS}):
        S = Dev(D.e, D.comm, le.scale_csr(csr, s), ncols)
        try:
            for kind, damp in solves:
                b = le.scaled_rhs(shape, kind)
                for t in [t for s2, t in le.PAIRS if s2 == s]:
                    what = (shape, kind, damp, s, t)
                    got = S.run(np.ldexp(b, t), K, R, L,
                                float(np.ldexp(damp, s)), what=what)
                    _relation(base[kind, damp], got, s, t, 1.0, what)
        finally:
            S.close()
    S = Dev(D.e, D.comm, le.scale_csr(csr, 0, -1.0), ncols)
    try:
        for kind, damp in solves:
            got = S.run(le.scaled_rhs(shape, kind), K, R, L, damp)
            _relation(base[kind, damp], got, 0, 0, -1.0, (shape, kind, "-A"))
    finally:
        S.close()


# ---- 4. two ranks --------------------------------------------------------------------------------
def test_two_thread_ranks():
    """ltol and two_i in two slabs cut INSIDE a block (ltol's column halo is
    not empty: reverse_update takes part), b_nan with the NaN in rank 1's slab
    only, and one scaled pair on convdiff11_2: every rank returns the same k
    and status (no rank leaves the loop alone), and the gathered x and the
    histories have the bits of the reference, or keep the relation between two
    solves on two ranks."""
    from thread_world import ThreadWorld
    jobs = []  # (key, csr, b, kmax, rtol, ltol, damp, want or None)
    for name in le.TWO_RANKS:
        case = BY_NAME[name]
        csr, ncols, b = case.system(True)
        cut = int(oracle.owner_ranges(2, len(b))[1])
        assert ncols == len(b) and cut % len(case.block) != 0, (name, cut)
        jobs.append((case.id, csr, b, le.KMAX, 0.0, case.ltol, case.damp,
                     case.want(True)))
    shape = "convdiff11_2"
    plain, N = le.csr_of(shape)
    nan_b = le.rank1_nan(N)
    want = le.reference(plain, N, nan_b, le.POISON_KMAX, le.POISON_RTOL,
                        le.POISON_LTOL)
    assert want.k == le.POISON_KMAX and np.all(np.isnan(want.x))
    jobs.append(("b_nan", plain, nan_b, le.POISON_KMAX, le.POISON_RTOL,
                 le.POISON_LTOL, 0.0, want))
    s, t = le.PAIRS[0]
    b = le.scaled_rhs(shape, "ones")
    K, R, L = le.SCALED_KMAX, le.SCALED_RTOL, le.SCALED_LTOL
    jobs.append(("base", plain, b, K, R, L, 0.0, None))
    jobs.append(("scaled", le.scale_csr(plain, s), np.ldexp(b, t), K, R, L, 0.0,
                 None))
    tw = ThreadWorld(2, timeout=45.0)

    def rank_body(rank, comm, exec_):  # noqa: F811
        ws = host.LsqrWorkspace(exec_)
        kept = {}
        for key, csr, b, kmax, rtol, ltol, damp, want in jobs:
            n = len(b)
            ranges = oracle.owner_ranges(2, n)
            r0, r1 = int(ranges[rank]), int(ranges[rank + 1])
            M = r1 - r0
            lrp, lci, lva, gh = oracle.localise_rows(*csr, r0, r1)
            if key == "ltol":
                assert len(gh) > 0, "the halo is empty"
            A = host.Matrix.create_matrix(comm, exec_, lrp, lci, lva, M, M, [],
                                          gh, False, host.P2P_NONBLOCKING)
            d_b = exec_.alloc(M)
            d_x = exec_.alloc(M + 2 * GUARD)
            exec_.copy_from_host(d_b, b[r0:r1])
            exec_.copy_from_host(d_x, np.full(M + 2 * GUARD, SENTINEL))
            k, hist_r, hist_ar, status = host.lsqr(
                comm, exec_, A, d_b, d_x + 8 * GUARD, kmax, rtol, ltol, damp,
                ws=ws)
            buf = exec_.copy_to_host(d_x, M + 2 * GUARD)
            assert np.all(buf[:GUARD] == SENTINEL), key
            assert np.all(buf[GUARD + M:] == SENTINEL), key
            ks = tw.gather(rank, np.array([k, status]))
            assert np.all(ks.reshape(-1, 2) == [k, status]), (key, ks)
            xs = tw.gather(rank, buf[GUARD:GUARD + M])
            got = Result(xs, k, hist_r.copy(), hist_ar.copy(), status)
            if want is not None:
                _same(got, want, (key, rank))
            kept[key] = got
            A.close()
            exec_.free(d_b), exec_.free(d_x)
        assert 1 < kept["base"].k <= K and kept["base"].status == 0
        _relation(kept["base"], kept["scaled"], s, t, 1.0, (s, t, rank))
        ws.close()

    tw.run(rank_body, gpu=True)
