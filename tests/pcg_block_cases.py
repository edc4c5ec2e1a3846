"""spmv::pcg_block restated in numpy, and the cases of test_gpu_pcg_block.py with
their references.  No GPU: the colours come from host.sgs_color, which is the
colouring the device objects use.

block_ref() is cg.h's block recurrence: every column runs the recurrence of
test_gpu_chebyshev._pcg_ref on oracle.csr_spmv, a dot product and a
preconditioner applied per column (test_gpu_sgs.Sweeps.apply, ilu0_cases.
Ilu0Ref.apply or dinv *), the columns in lockstep, each with its own alpha,
beta and stop, frozen once it has stopped.  Column c of its result equals
_pcg_ref on column c alone bit for bit (test_pcg_block_host.py).

Generators are imported, not copied: the matrices of test_gpu_pcg / test_gpu_sgs,
the right-hand sides of test_gpu_cg_block."""
import math

import numpy as np

import ilu0_cases as ic
import oracle
import test_gpu_cg_block as tb
import test_gpu_chebyshev as tc
import test_gpu_pcg as tp
import test_gpu_sgs as ts
from spmv_amd import host
from test_gpu_bicgstab import _dot_chunked

KMAX, RTOL = tp.KMAX, tp.RTOL
SHAPES = tp.SHAPES                  # poisson11, poisson24, banded4097
KINDS = ("dinv", "sgs", "ilu0")
NRHS = (1, 2, 3, 4, 8)


def block_ref(spmv, dot, B, precond, kmax, rtol):
    """-> (iterations[nrhs], history[nrhs, kmax + 1] with -1.0 beyond a
    column's k, X[N, nrhs]); B is [N, nrhs]"""
    N, nrhs = B.shape
    X = [np.zeros(N) for _ in range(nrhs)]
    R = [np.array(B[:, c], dtype=np.float64) for c in range(nrhs)]
    Z = [precond(r) for r in R]
    P = [z.copy() for z in Z]
    rz = [dot(R[c], Z[c]) for c in range(nrhs)]
    rr0 = [dot(R[c], R[c]) for c in range(nrhs)]
    hist = np.full((nrhs, kmax + 1), -1.0)
    hist[:, 0] = [math.sqrt(v) for v in rr0]
    its = np.zeros(nrhs, np.int32)
    done = [v == 0.0 for v in rr0]
    k = 0
    while k < kmax and not all(done):
        k += 1
        AP = [None if done[c] else spmv(P[c]) for c in range(nrhs)]
        for c in range(nrhs):
            if done[c]:
                continue
            alpha = rz[c] / dot(P[c], AP[c])
            R[c] = R[c] - alpha * AP[c]
            Z[c] = precond(R[c])
            rz_new, rr = dot(R[c], Z[c]), dot(R[c], R[c])
            X[c] = X[c] + alpha * P[c]
            hist[c, k] = math.sqrt(rr)
            its[c] = k
            if math.sqrt(rr) / math.sqrt(rr0[c]) < rtol:
                done[c] = True
                continue
            beta = rz_new / rz[c]
            rz[c] = rz_new
            P[c] = beta * P[c] + Z[c]
    return its, hist, np.stack(X, axis=1)


class ColumnRef:
    """One column of two block references (two summation orders of the dot
    product), with the fields test_gpu_chebyshev._vs_ref reads"""

    def __init__(self, first, second, c):
        def column(ref):
            its, hist, X = ref
            k = int(its[c])
            return X[:, c].copy(), k, hist[c, :k + 1].copy()
        self.x, self.k, self.hist = column(first)
        self.second = column(second)

    dev = tc._Ref.dev


def own_deviation(ref, norm_a):
    """The deviation between the two summation orders over EVERY history entry
    _vs_ref compares for a solve that stops where the reference does (its own
    dev_ref leaves out an entry the second order does not have); inf when the
    second order has fewer entries."""
    if ref.k == 0:
        return 0.0
    m = min(ref.k, 50)
    upto = m + 1 if ref.hist[m] >= tp._noise_floor(norm_a, ref.x) else m
    second = ref.second[2]
    if len(second) < upto:
        return math.inf
    return float(np.abs(second[:upto] / ref.hist[:upto] - 1).max())


class Case:
    """One matrix (general CSR), its three preconditioners restated, its
    right-hand sides and the per-column references, computed once."""

    def __init__(self, name):
        self.name = name
        self.csr = ts._make_csr(name)
        self.N = N = len(self.csr[0]) - 1
        self.n_grid = int(name[7:]) if name.startswith("poisson") else 0
        self.dinv = 1.0 / tp._diag_of(self.csr)
        self.norm_a = tp._norm_inf(self.csr)
        self.cols = tb._columns(self.csr, N, self.n_grid)
        self.colours = host.sgs_color(self.csr[0], self.csr[1], N, N, False)[0]
        self._pre, self._refs = {}, {}

    def spmv(self, v):
        return oracle.csr_spmv(*self.csr, np.ascontiguousarray(v))

    def precond(self, kind):
        """r -> M^-1 r"""
        if kind not in self._pre:
            if kind == "dinv":
                self._pre[kind] = lambda r: self.dinv * r
            elif kind == "sgs":
                sweeps = ts.Sweeps(self.csr, self.N, self.colours, False)
                self._pre[kind] = lambda r: sweeps.apply(self.dinv, r)
            else:
                ref = ic.Ilu0Ref(self.csr, self.N, self.colours, False)
                fac = ref.factor()
                self._pre[kind] = lambda r: ref.apply(fac, r)
        return self._pre[kind]

    def pool(self, kind):
        """the columns of a block of nrhs held to the history bar: the first
        nrhs of these.  Two columns are replaced because the restatement
        disagrees with itself on them by more than a tenth of the bar
        (own_deviation).  The eigenvector column: behind SGS its last residual
        is rounding noise just above _vs_ref's noise floor (poisson24: 3.1e-11
        in one summation order, 7.7e-13 in the other); the tests on stops and
        independence use it.  b = A 1 on poisson11 behind ILU(0): 3.7e-7 at
        its last entry; the eigenvector column (13 iterations there) stands in."""
        first = "eig" if (self.name, kind) == ("poisson11", "ilu0") else "ones"
        return [first, "rand0", "rand6", "rand1", "rand2", "rand3", "rand4",
                "rand5"]

    def block(self, names):
        return np.stack([self.cols[c] for c in names], axis=1)

    def block_refs(self, kind, names, kmax=KMAX, rtol=RTOL):
        """the block reference in both summation orders"""
        B, M = self.block(names), self.precond(kind)
        return (block_ref(self.spmv, oracle.ddot, B, M, kmax, rtol),
                block_ref(self.spmv, _dot_chunked, B, M, kmax, rtol))

    def ref(self, kind, col, kmax=KMAX, rtol=RTOL):
        """the reference of one column (a block of one: the bits of a column do
        not depend on its neighbours)"""
        key = (kind, col, kmax, rtol)
        if key not in self._refs:
            first, second = self.block_refs(kind, [col], kmax, rtol)
            self._refs[key] = ColumnRef(first, second, 0)
        return self._refs[key]

    def dev_ref(self, kind, col):
        """what _vs_ref will compute for this column: the deviation between
        the two summation orders over the compared entries"""
        return own_deviation(self.ref(kind, col), self.norm_a)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


class SlabCase:
    """The Poisson matrix of n^3 in slabs over `world` ranks, nrhs = 4, the SGS
    preconditioner block-Jacobi over the ranks: the restatement on
    oracle.dist_spmv with the rank-ordered sum, per storage and halo model."""

    def __init__(self, world, n=8, kmax=200, rtol=1e-10):
        self.world, self.n, self.kmax, self.rtol = world, n, kmax, rtol
        csr = tp._csr(f"poisson{n}")
        rp, ci, va = csr
        self.N = N = n ** 3
        diag = tp._diag_of(csr)
        self.norm_a = tp._norm_inf(csr)
        rng = np.random.default_rng(world)
        self.B = np.stack([oracle.csr_spmv(*csr, np.ones(N)),
                           oracle.csr_spmv(*csr, rng.uniform(-1, 1, N)),
                           tb._sine_mode(n),
                           oracle.csr_spmv(*csr, rng.uniform(-1, 1, N))], axis=1)
        self.ranges = ranges = oracle.owner_ranges(world, N)
        self.blocks = [oracle.localise_rows(rp, ci, va, int(ranges[r]),
                                            int(ranges[r + 1]))
                       for r in range(world)]

        def dist_dot(dot):
            def f(a, b):
                s = 0.0
                for r in range(world):
                    s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
                return s
            return f

        self.refs = {}
        for sym in (False, True):
            sweeps = []
            for r in range(world):
                lrp, lci, lva, _ = self.blocks[r]
                M = int(ranges[r + 1] - ranges[r])
                colours, _ = host.sgs_color(lrp, lci, M, M, sym)
                sweeps.append(ts.Sweeps((np.asarray(lrp), np.asarray(lci),
                                         np.asarray(lva)), M, colours, sym))

            def precond(v, sweeps=sweeps):
                return np.concatenate([
                    sweeps[r].apply(1.0 / diag[ranges[r]:ranges[r + 1]],
                                    v[ranges[r]:ranges[r + 1]])
                    for r in range(world)])

            for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
                def spmv(p, sym=sym, cm=cm):
                    return oracle.dist_spmv(world, rp, ci, va, p, sym, cm)
                first = block_ref(spmv, dist_dot(oracle.ddot), self.B, precond,
                                  kmax, rtol)
                second = block_ref(spmv, dist_dot(_dot_chunked), self.B, precond,
                                   kmax, rtol)
                self.refs[(sym, cm)] = [ColumnRef(first, second, c)
                                        for c in range(4)]

    def dev_refs(self):
        return [own_deviation(r, self.norm_a) for ref in self.refs.values()
                for r in ref]


_SLABS = {}


def slab_case(world):
    if world not in _SLABS:
        _SLABS[world] = SlabCase(world)
    return _SLABS[world]


def gpu_cases():
    """every (shape, kind, column) test_gpu_pcg_block.py holds to the history
    bar: the blocks of test_per_column_against_the_restatement, and
    ragged3001 with sgs"""
    out = [(shape, kind, col) for shape in SHAPES for kind in KINDS
           for col in case(shape).pool(kind)]
    out += [("ragged3001", "sgs", col) for col in case("ragged3001").pool("sgs")[:4]]
    return out
