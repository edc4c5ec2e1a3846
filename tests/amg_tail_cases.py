"""The fused tail of the AMG V-cycle (AmgPreconditioner::set_tail_rows,
spmv_hip_amg_tail_*; hip/spmv_amg.hip: amg_tail_kernel) restated in numpy: which
levels form the tail, the launches it saves, and the walk of the kernel itself
over hand-built levels.  Every numpy operation is one rounding per element; a
level's product is amg_cases.spmv_ltr or, with `lanes`, amg_cases.spmv_vector.
Shared by test_amg_tail_host.py and test_gpu_amg_tail.py.  Nothing here has a
tolerance."""
import numpy as np

import amg_cases as ac
import amg_kernel_cases as kc

BLOCK = 1024  # threads of the one workgroup
LONG = 2500
NZ = np.float64(-0.0)


# ---- the rules --------------------------------------------------------------------------
def first_tail_level(rows, max_rows):
    """The tail is the longest suffix t .. len(rows)-1 with t >= 1 whose levels
    all have at most max_rows rows; -> t, len(rows) when there is none."""
    nl = len(rows)
    if nl < 2 or max_rows <= 0:
        return nl
    t = nl
    while t > 1 and rows[t - 1] <= max_rows:
        t -= 1
    return t


def tail_levels(rows, max_rows):
    return len(rows) - first_tail_level(rows, max_rows)


def launches(nl, s, c, tail=0):
    """kernels and copies of one application (tools/amgbench.py's count): per
    level that is not the coarsest 4 s + 3, on the coarsest 2 c - 1, one copy
    out; a tail of `tail` levels puts one launch in the place of its share"""
    full = (nl - 1) * (4 * s + 3) + (2 * c - 1) + 1
    if tail == 0:
        return full
    t = nl - tail
    return full - ((nl - 1 - t) * (4 * s + 3) + (2 * c - 1)) + 1


# The object cases of test_gpu_amg_tail.py: (matrix of test_gpu_amg, options,
# level sizes, {tail_rows: tail_levels}).  test_amg_tail_host.py holds the sizes
# against AmgRef and the expectations against first_tail_level.
POISSON24 = ("poisson24", {}, (13824, 1685, 150),
             {149: 0, 150: 1, 1685: 2, 10 ** 9: 2})
FURTHER = (
    ("poisson11", {"min_coarse_rows": 20}, (1331, 183, 18),
     {17: 0, 18: 1, 183: 2, 1331: 2}),
    ("banded4097", {}, (4097, 637, 78), {77: 0, 100: 1, 4096: 2}),
    ("convdiff8", {"min_coarse_rows": 20}, (512, 72, 11), {11: 1, 72: 2}),
    ("ragged3001", {}, (3001, 77), {76: 0, 77: 1, 10 ** 6: 1}),
    ("arrow130", {"min_coarse_rows": 20}, (130, 1), {1: 1}),
    ("diag200", {}, (200,), {1: 0, 10 ** 9: 0}),
    ("diag1", {}, (1,), {1: 0, 10 ** 9: 0}),
)
OBJECT_CASES = (POISSON24,) + FURTHER


# ---- the kernel's walk ------------------------------------------------------------------
class Level:
    """One level of a hand-built tail: csr (square), dinv, the step to the next
    level (amg_kernel_cases.make_step; None on the last), the lanes of its
    product (0 = one lane per row) and its coefficients a, b."""

    def __init__(self, csr, dinv, a, b, step=None, lanes=0):
        self.csr, self.dinv, self.step, self.lanes = csr, dinv, step, lanes
        self.a, self.b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        self.n = len(csr[0]) - 1

    def product(self, z):
        if self.lanes:
            return ac.spmv_vector(self.csr, z, self.lanes)
        return ac.spmv_ltr(self.csr, z)


def _chebyshev(L, r, degree):
    d = L.b[0] * (L.dinv * r)
    z = d.copy()
    for j in range(1, degree):
        w = L.product(z)
        d = L.a[j] * d + L.b[j] * (L.dinv * (r - w))
        z = z + d
    return z


def tail_ref(levels, s, c, scale, r0):
    """-> (r per level, z per level) as the kernel leaves them"""
    with np.errstate(all="ignore"):
        rs, zs = [np.asarray(r0, np.float64)], []
        for l, L in enumerate(levels):
            if l == len(levels) - 1:
                zs.append(_chebyshev(L, rs[l], c))
                break
            z = _chebyshev(L, rs[l], s)
            t = rs[l] - L.product(z)
            st = L.step
            rs.append(ac.seq_sum(st["member_ptr"], t[st["member"]]))
            zs.append(z)
        for l in range(len(levels) - 2, -1, -1):
            L, r = levels[l], rs[l]
            z = zs[l] + scale * zs[l + 1][L.step["agg"]]
            d = None
            for j in range(s):
                t = L.b[j] * (L.dinv * (r - L.product(z)))
                d = t if j == 0 else L.a[j] * d + t
                z = z + d
            zs[l] = z
        return rs, zs


def csr_of_lens(lens, n, seed):
    """rows of the given lengths, columns anywhere in [0, n) (repeats allowed:
    a stored entry is a stored entry), values in (-1, 1)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    nnz = int(lens.sum())
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return (rp, rng.integers(0, n, nnz).astype(np.int32),
            rng.uniform(-1.0, 1.0, nnz))


def agg_of_sizes(sizes, seed):
    """aggregates of the given sizes, their members scattered over the rows"""
    agg = np.repeat(np.arange(len(sizes)), sizes)
    np.random.default_rng(seed).shuffle(agg)
    return agg.astype(np.int32)


def _coeffs(degree, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.2, 0.9, 16)[:max(degree, 1)], \
        rng.uniform(0.2, 0.9, 16)[:max(degree, 1)]


class Tail:
    """levels, degrees, scale, the right-hand side and the expected vectors"""

    def __init__(self, name, lens_per_level, aggs, s=2, c=3, scale=1.0, lanes=0,
                 seed=0):
        self.name, self.s, self.c, self.scale = name, s, c, scale
        self.levels = []
        rng = np.random.default_rng(seed + 99)
        for l, lens in enumerate(lens_per_level):
            n = len(lens)
            last = l == len(lens_per_level) - 1
            a, b = _coeffs(c if last else s, seed + 7 * l)
            step = None if last else kc.make_step(aggs[l])
            if step is not None:
                assert step["fine_rows"] == n
                assert step["coarse_rows"] == len(lens_per_level[l + 1])
            lane = lanes[l] if isinstance(lanes, (list, tuple)) else lanes
            self.levels.append(Level(csr_of_lens(lens, n, seed + l),
                                     rng.uniform(0.5, 2.0, n), a, b, step, lane))
        self.r = rng.uniform(-1.0, 1.0, self.levels[0].n)

    def ref(self):
        return tail_ref(self.levels, self.s, self.c, self.scale, self.r)


def _short_lens(n, seed):
    return np.random.default_rng(seed).integers(0, 7, n)


def _split(n, nc, seed):
    """n rows into nc aggregates, none empty"""
    rng = np.random.default_rng(seed)
    extra = rng.multinomial(n - nc, np.full(nc, 1.0 / nc))
    return agg_of_sizes(1 + extra, seed)


SIZES = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)


def size_case(n):
    nc = max(1, n // 3)
    return Tail(f"rows{n}", [_short_lens(n, n), _short_lens(nc, n + 1)],
                [_split(n, nc, n)], seed=n)


def aggregate_case():
    sizes = [1, 2, 3, 700]
    n = sum(sizes)
    return Tail("aggregates", [_short_lens(n, 5), _short_lens(4, 6)],
                [agg_of_sizes(sizes, 3)], seed=11)


def one_coarse_row_case():
    return Tail("one coarse row", [_short_lens(5, 1), [3]],
                [np.zeros(5, np.int32)], seed=12)


def sequential_lens_case():
    lens = [0, 1, LONG, 3, 0, 2]
    return Tail("sequential", [lens, [0, LONG, 1]],
                [np.array([0, 1, 2, 0, 1, 2], np.int32)], seed=13)


def vector_case(lanes):
    edge = [0, 1, lanes - 1, lanes, lanes + 1, LONG]
    rounds = 2 * (BLOCK // lanes) + 1  # a third trip of the rows' loop
    lens = np.array((edge * ((rounds + 5) // 6))[:rounds])
    lens[6:][lens[6:] == LONG] = 9  # one long row is enough
    nc = 6
    return Tail(f"vector{lanes}", [lens, edge], [_split(rounds, nc, lanes)],
                lanes=lanes, seed=20 + lanes)


def degree_case(s, c, scale):
    n = 300
    return Tail(f"s{s}c{c}x{scale}", [_short_lens(n, 1), _short_lens(40, 2)],
                [_split(n, 40, 3)], s=s, c=c, scale=scale, seed=31)


def depth_case(s=2, c=3, lanes=0):
    n0, n1, n2 = 2 * BLOCK + 1, 300, 7
    return Tail(f"depth s{s} c{c}", [_short_lens(n0, 1), _short_lens(n1, 2),
                                    _short_lens(n2, 3)],
                [_split(n0, n1, 4), _split(n1, n2, 5)], s=s, c=c, scale=1.6,
                lanes=lanes, seed=41)


def special_cases():
    """a lone -0.0, Inf - Inf, a NaN in the middle of a row and of an
    aggregate"""
    out = []

    def base(name, seed):
        lens = [3, 1, 5, 4, 2, 5, 3, 3, 4]
        return Tail(name, [lens, [2, 3, 1]],
                    [np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], np.int32)], seed=seed)
    t = base("lone negative zero", 51)
    rp, ci, va = t.levels[0].csr
    va[rp[1]] = NZ  # row 1 has this entry alone: 0.0 + (-0.0 * z) = +0.0
    t.r[4] = NZ
    out.append(t)
    t = base("inf minus inf", 52)
    t.r[0], t.r[3] = np.inf, -np.inf  # both in aggregate 0
    out.append(t)
    t = base("nan in a row", 53)
    rp, ci, va = t.levels[0].csr
    va[rp[2] + 2] = np.nan  # the third of five entries
    out.append(t)
    t = base("nan in an aggregate", 54)
    t.r[4] = np.nan  # aggregate 1 = rows 1, 4, 7
    out.append(t)
    t = base("huge", 55)
    t.r[8] = 1e300
    t.levels[0].csr[2][:] *= 1e200
    out.append(t)
    return out
