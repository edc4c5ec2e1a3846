"""The cases of test_gpu_pcg_block_amg.py with their references: pcg_block with an
AmgPreconditioner, restated as pcg_block_cases.block_ref with amg_cases.AmgRef
(through test_gpu_amg.restate, whose products keep the order of the plans) as
the preconditioner of every column.  No GPU.

Matrices, right-hand sides and the two summation orders of the dot products
are pcg_block_cases' (imported, not copied)."""
import numpy as np

import oracle
import pcg_block_cases as pc
import test_gpu_amg as ta
import test_gpu_pcg as tp
from test_gpu_bicgstab import _dot_chunked

KMAX, RTOL = pc.KMAX, pc.RTOL
SHAPES = ("poisson11", "poisson24", "banded4097")
# The columns of a block of nrhs held to the history bar of
# test_gpu_chebyshev._vs_ref: the first nrhs of these.  A column whose
# restatement disagrees with itself between the two summation orders by more
# than a tenth of that bar (1e-7) is not kept (test_amg_block_host.py computes
# it for every one of them).
POOL = {
    "poisson11": ["ones", "rand0", "rand6", "rand1", "rand2", "rand3", "rand4",
                  "rand5"],
    "poisson24": ["ones", "rand0", "rand6", "rand1"],
    "banded4097": ["ones", "rand0", "rand6", "rand1", "rand2", "rand3", "rand4",
                   "rand5"],
}


class Case:
    def __init__(self, name):
        self.name = name
        self.base = B = pc.case(name)
        self.N, self.csr, self.norm_a, self.cols = B.N, B.csr, B.norm_a, B.cols
        self.amg = ta.restate(B.csr, B.N, False)
        self._refs = {}

    def spmv(self, v):
        return self.base.spmv(v)

    def precond(self, r):
        return self.amg.apply(r)

    def block(self, names):
        return self.base.block(names)

    def block_refs(self, names, kmax=KMAX, rtol=RTOL):
        B = self.block(names)
        return (pc.block_ref(self.spmv, oracle.ddot, B, self.precond, kmax, rtol),
                pc.block_ref(self.spmv, _dot_chunked, B, self.precond, kmax, rtol))

    def ref(self, col, kmax=KMAX, rtol=RTOL):
        key = (col, kmax, rtol)
        if key not in self._refs:
            first, second = self.block_refs([col], kmax, rtol)
            self._refs[key] = pc.ColumnRef(first, second, 0)
        return self._refs[key]

    def dev_ref(self, col):
        return pc.own_deviation(self.ref(col), self.norm_a)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


class SlabCase:
    """The Poisson matrix of n^3 in slabs over `world` ranks, nrhs = 4, the AMG
    cycle block-Jacobi over the ranks (each rank's own diagonal block,
    min_coarse_rows = 20 so that the blocks have several levels), general
    storage, both halo models: pcg_block_cases.SlabCase's pattern."""

    OPTIONS = dict(min_coarse_rows=20)

    def __init__(self, world, n=8, kmax=200, rtol=1e-10):
        import gmres_cases as gc
        self.world, self.kmax, self.rtol = world, kmax, rtol
        S = pc.slab_case(world)
        assert (S.n, S.kmax, S.rtol) == (n, kmax, rtol)
        self.B, self.ranges, self.blocks, self.norm_a = (S.B, S.ranges, S.blocks,
                                                         S.norm_a)
        rp, ci, va = tp._csr(f"poisson{n}")
        ranges = self.ranges
        refs = []
        for r in range(world):
            lrp, lci, lva, _ = self.blocks[r]
            lrp, lci, lva = np.asarray(lrp), np.asarray(lci), np.asarray(lva)
            M = int(ranges[r + 1] - ranges[r])
            keep = lci < M  # the diagonal block
            brp = np.concatenate([[0], np.cumsum(np.bincount(
                gc.row_of(lrp)[keep], minlength=M))]).astype(np.int32)
            refs.append(ta.restate((brp, np.ascontiguousarray(lci[keep]),
                                    np.ascontiguousarray(lva[keep])), M, False,
                                   **self.OPTIONS))

        def precond(v):
            return np.concatenate([refs[r].apply(v[ranges[r]:ranges[r + 1]])
                                   for r in range(world)])

        def dist_dot(dot):
            def f(a, b):
                s = 0.0
                for r in range(world):
                    s += dot(a[ranges[r]:ranges[r + 1]], b[ranges[r]:ranges[r + 1]])
                return s
            return f

        self.refs = {}
        from spmv_amd import host
        for cm in (host.P2P_BLOCKING, host.P2P_NONBLOCKING):
            def spmv(p, cm=cm):
                return oracle.dist_spmv(world, rp, ci, va, p, False, cm)
            first = pc.block_ref(spmv, dist_dot(oracle.ddot), self.B, precond,
                                 kmax, rtol)
            second = pc.block_ref(spmv, dist_dot(_dot_chunked), self.B, precond,
                                  kmax, rtol)
            self.refs[cm] = [pc.ColumnRef(first, second, c) for c in range(4)]

    def dev_refs(self):
        return [pc.own_deviation(r, self.norm_a) for ref in self.refs.values()
                for r in ref]


_SLABS = {}


def slab_case(world):
    if world not in _SLABS:
        _SLABS[world] = SlabCase(world)
    return _SLABS[world]
