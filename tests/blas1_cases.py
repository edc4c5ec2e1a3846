"""Cases and references for the kernel-level tests of the solvers' vector
kernels (blas1.hip, blas1_block.hip, blas1_pcg.hip, blas1_bicgstab.hip,
blas1_cheb.hip).  Nothing here touches a GPU: test_blas1_cases_host.py holds
this module to its targets, test_gpu_blas1_kernels.py runs the kernels on it.

Two data sets:

  set E  small integers (|v| <= 2**10) and scalars that make every coefficient
         a small integer or a power of two: every element, partial sum and
         reduced scalar is an integer below 2**53, so the reference is integer
         numpy and the comparison is equality of bits whatever the order of
         summation.  Used at every length, the wrap edges included.
  set R  irrational values over about 2**+-20 with mixed signs.  Element-wise
         results must equal the unfused numpy restatement below bit for bit
         (every `*`, `+`, `-`, `/` and sqrt of a float64 array or np.float64 is
         one IEEE rounding, as the kernels built with -ffp-contract=off do);
         sums are held to the a-priori bound of `sum_bound`.

The references restate include/spmv_hip.h: one function per kernel, named
after it, taking and returning numpy arrays.  Scalars go through the same
helpers the kernels' prologues spell (cg_alpha, cg_beta, ...).
"""
import math
from fractions import Fraction

import numpy as np

K_BLOCK = 256   # threads of a workgroup (common.h kBlock)
K_U = 4         # 16-byte loads in flight per lane and stream (kU)
UNIT = 2 * K_U * K_BLOCK  # doubles a workgroup takes per trip of its loop
U = 2.0 ** -53  # unit roundoff of float64
WRAP_MAX = 16 << 20  # doubles: beyond this W the wrap edges are skipped
SENTINEL = -777.25   # pre-fill of write-only buffers and guard words


# ---------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------
def wrap_length(dot_blocks):
    """W: doubles the largest grid (dot_blocks workgroups) covers in ONE trip;
    a vector longer than W sends workgroup 0 round its loop a second time."""
    return UNIT * int(dot_blocks)


def small_lengths():
    b2 = 2 * K_BLOCK
    return [0, 1, 2, 3, b2 - 1, b2, b2 + 1, UNIT - 1, UNIT, UNIT + 1,
            2 * UNIT + 1]


def wrap_lengths(dot_blocks):
    w = wrap_length(dot_blocks)
    return [w - 1, w, w + 1, w + UNIT + 3]


def block_shapes(nrhs, dot_blocks, wrap):
    """(M, nrhs) for cg_block: lengths above are those of the interleaved
    array M * nrhs; the nearest M from below and above, so that even and odd M
    both occur for every nrhs (asserted by the host test)."""
    lens = wrap_lengths(dot_blocks) if wrap else small_lengths()
    ms = set()
    for n in lens:
        ms.add(n // nrhs)
        ms.add(-(-n // nrhs))
    if not wrap:
        ms |= {0, 1, 2, 3}
    return sorted(ms)


def stream_grid(n2, dot_blocks):
    """spmv_grid_for(ctx, n2, kUnit): workgroups of a streaming kernel"""
    need = max(1, -(-n2 // (K_U * K_BLOCK)))
    return min(need, dot_blocks)


def rows_grid(n, dot_blocks):
    """one element (row) per thread, capped at dot_blocks workgroups"""
    return min(max(1, -(-n // K_BLOCK)), dot_blocks)


def onehot_indices(n, dot_blocks):
    """0, 1, n-2, n-1, every unit boundary +-1, the first element after a wrap"""
    idx = {0, 1, n - 2, n - 1}
    for b in range(UNIT, n + 1, UNIT):
        idx |= {b - 1, b, b + 1}
    idx |= {wrap_length(dot_blocks)}
    return sorted(i for i in idx if 0 <= i < n)


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def exact_vec(n, seed):
    """set E: integers in [-2**10, 2**10] \\ {0}, as float64"""
    rng = np.random.default_rng(1000 + seed)
    v = rng.integers(1, 2 ** 10 + 1, size=n).astype(np.float64)
    return v * rng.choice([-1.0, 1.0], size=n)


def exact_dinv(n, seed):
    """set E preconditioner: 1, 2 or 4"""
    rng = np.random.default_rng(2000 + seed)
    return rng.choice([1.0, 2.0, 4.0], size=n)


def round_vec(n, seed):
    """set R: sqrt(prime-ish) mantissas times 2**e, e in [-20, 20], mixed signs"""
    rng = np.random.default_rng(3000 + seed)
    m = np.sqrt(rng.integers(2, 10 ** 6, size=n).astype(np.float64) + 0.5)
    e = rng.integers(-20, 21, size=n)
    return np.ldexp(m / 1000.0, e) * rng.choice([-1.0, 1.0], size=n)


def round_dinv(n, seed):
    """set R preconditioner: positive, spread over 2**+-4"""
    return np.abs(round_vec(n, 77 + seed)) ** 0.2


def bits26(x):
    """x rounded to 26 significant bits: its square is exact in float64 and
    the square root of that square is x again"""
    m, e = math.frexp(x)
    return math.ldexp(round(m * 2 ** 26), e - 26)


# ---------------------------------------------------------------------------
# scalars, as the kernels' prologues form them (each operation one rounding)
# ---------------------------------------------------------------------------
def f(x):
    return np.float64(x)


def cg_alpha(rr_prev, pap):
    s = np.sqrt(f(rr_prev))
    return (s * s) / f(pap)                                       # cg.cpp:66


def cg_beta(rr_new, rr_prev):
    sn, so = np.sqrt(f(rr_new)), np.sqrt(f(rr_prev))
    return (sn * sn) / (so * so)                                  # cg.cpp:77


def converged(rr_new, rr0, rtol):
    return bool(np.sqrt(f(rr_new)) / np.sqrt(f(rr0)) < f(rtol))   # cg.cpp:80


def pcg_alpha(rz_prev, pap):
    return f(rz_prev) / f(pap)


def pcg_beta(rz_new, rz_prev):
    return f(rz_new) / f(rz_prev)


def bicg_omega(ts, tt):
    return f(0.0) if tt == 0.0 else f(ts) / f(tt)


def bicg_beta(rho_k, rho_prev, alpha, omega):
    return (f(rho_k) / f(rho_prev)) * (f(alpha) / f(omega))


# ---------------------------------------------------------------------------
# element-wise references (unfused: a product rounded, then a sum rounded)
# ---------------------------------------------------------------------------
def axpy(a, x, y):
    """y + a x, the multiply rounded first"""
    return y + f(a) * x


def cg_update_xr(alpha, p, Ap, x, r):
    return axpy(alpha, p, x), r + (-f(alpha)) * Ap


def cg_update_r(alpha, Ap, r):
    return r + (-f(alpha)) * Ap


def cg_update_p(beta, r, p):
    return f(beta) * p + r


def cg_update_xp(alpha, beta, conv, r, x, p):
    """converged: x takes the update, p stays (cg.cpp:80-81)"""
    xn = axpy(alpha, p, x)
    return xn, (p.copy() if conv else f(beta) * p + r)


def cg_update_x2p(alpha_prev, alpha, beta, conv, r, x, p_prev, p_cur):
    xn = axpy(alpha, p_cur, axpy(alpha_prev, p_prev, x))
    return xn, (p_prev.copy() if conv else f(beta) * p_cur + r)


def cg_residual(b, Ax):
    return b - Ax


def pcg_update_r(alpha, Ap, dinv, r):
    """-> r, z = dinv*r (the second factor of the r.z terms)"""
    rn = r + (-f(alpha)) * Ap
    return rn, dinv * rn


def pcg_update_xp(alpha, beta, conv, r, dinv, x, p):
    xn = axpy(alpha, p, x)
    return xn, (p.copy() if conv else f(beta) * p + dinv * r)


def scaled(dinv, v):
    return v if dinv is None else dinv * v


def bicg_update_s(alpha, r, v, dinv):
    s = r - f(alpha) * v
    return s, (None if dinv is None else dinv * s)


def bicg_update_xr(alpha, omega, ph, sh, s, t, x):
    """sh None: the unpreconditioned kernel, whose sh is s"""
    h = s if sh is None else sh
    xn = (x + f(alpha) * ph) + f(omega) * h
    return xn, s - f(omega) * t


def bicg_update_p(beta, omega, r, v, dinv, p):
    w = r + f(beta) * (p - f(omega) * v)
    return w, (None if dinv is None else dinv * w)


def cheb_scale(s, dinv, vin):
    return scaled(dinv, vin / f(s))


def cheb_apply0(b0, r, dinv):
    return f(b0) * scaled(dinv, r)


def cheb_step(a, b, w, r, dinv, d, z):
    """-> d, z"""
    dn = f(a) * d + f(b) * scaled(dinv, r - w)
    return dn, z + dn


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def exact_dot_int(a, b):
    """set E: the dot product as a Python int (a, b hold integers)"""
    ai, bi = a.astype(np.int64), b.astype(np.int64)
    assert np.array_equal(ai, a) and np.array_equal(bi, b)
    return int(np.dot(ai, bi))


def exact_dot(a, b):
    """set R: (sum a_i b_i, sum |a_i b_i|) as Fractions, no rounding at all"""
    s = sa = Fraction(0)
    for x, y in zip(a.tolist(), b.tolist()):
        t = Fraction(x) * Fraction(y)
        s += t
        sa += abs(t)
    return s, sa


def depth(n, dot_blocks, streaming=True, arrays=1):
    """d: the longest chain of additions between a product and the scalar the
    reducer installs, read off the kernels.

    producer, streaming (stream_dot, stream_update_r, ...: SPMV_FOR_UNITS):
      a thread adds 2 * kU products per trip of its loop (kU double2 elements,
      .x then .y, into one accumulator), over ceil(n2 / (grid * kU * kBlock))
      trips with n2 = n // 2 and grid = spmv_grid_for(n2, kUnit);
    producer, one element per thread (cg_init, cg_residual, pcg_init, ...):
      one product per trip, ceil(n / (grid * kBlock)) trips;
    both: + 1 for the odd tail element (thread 0 of workgroup 0), + 6 shuffle
      steps (offsets 32 .. 1), + 4 wave slots added by thread 0 (the first to
      a zero, counted all the same).
    reducer (reduce_partials, sum_partials, consume_partials, reduce_column):
      ceil(len / kBlock) partials per thread and array (`arrays` = 2 for the
      *_pAp2 forms), + 6 shuffle steps, + 4 wave slots.
    The pair kernels of cg_block stop their shuffles at offset K/2 and add
    kU products per accumulator and trip: fewer additions, the same bound."""
    if streaming:
        n2 = n // 2
        g = stream_grid(n2, dot_blocks)
        adds = 2 * K_U * max(1, -(-n2 // (g * K_U * K_BLOCK)))
    else:
        g = rows_grid(n, dot_blocks)
        adds = max(1, -(-n // (g * K_BLOCK)))
    producer = adds + 1 + 6 + 4
    reducer = arrays * -(-dot_blocks // K_BLOCK) + 6 + 4
    return producer + reducer


def sum_bound(d, sum_abs, roundings=1):
    """|computed - exact| <= gamma * sum|terms| with gamma = m u / (1 - m u),
    m = d + roundings: every term carries `roundings` roundings of its own
    (1: the product; 2: a product of a product, as r * (dinv * r)) and at most
    d additions, each a factor (1 + delta), |delta| <= u (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2: any order of summation)."""
    m = Fraction(d + roundings) * Fraction(U)
    return m * Fraction(sum_abs) / (1 - m)


def sum_within(computed, exact, sum_abs, d, roundings=1):
    return abs(Fraction(float(computed)) - exact) <= sum_bound(d, sum_abs,
                                                                roundings)


def same_bits(a, b):
    """equality of bits (distinguishes -0.0 from 0.0, equal NaNs are equal)"""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64),
                                                 b.view(np.uint64))


# ---------------------------------------------------------------------------
# installed scalars
# ---------------------------------------------------------------------------
RTOL_GO = 2.0 ** -20    # sqrt(rr_new / rr0) is of order 1: not converged, by 2**20
RTOL_STOP = 2.0 ** 20   # ... converged, by 2**20


def cg_scalars(kind):
    """rr[0], rr[k-2] (= rr[0] at k = 2), pAp[k-1], rr[k-1], pAp[k], rr[k].
    E: alpha_prev = 1 / 0.25 = 4, alpha = 4 / 2 = 2, beta = 16 / 4 = 4 (rr[k] a
    perfect square times rr[k-1]), all exact.  R: every rr the exact square of
    a 26-bit number, so sqrt and the squaring back are exact and alpha, beta
    are one correctly rounded division each."""
    if kind == "E":
        return dict(rr0=1.0, pAp_prev=0.25, rr_prev=4.0, pAp=2.0, rr_new=16.0)
    s0, s1, s2 = bits26(1.7320508), bits26(1.2345678), bits26(0.7771234)
    return dict(rr0=s0 * s0, pAp_prev=0.5772156649, rr_prev=s1 * s1,
                pAp=0.7310585786, rr_new=s2 * s2)


def pcg_scalars(kind):
    """rr[0], rz[k-1], pAp[k], rz[k], rr[k].  E: alpha = 2, beta = 4."""
    if kind == "E":
        return dict(rr0=1.0, rz_prev=4.0, pAp=2.0, rz_new=16.0, rr_new=16.0)
    return dict(rr0=3.0000001, rz_prev=1.5241577, pAp=0.7310585786,
                rz_new=0.6039207, rr_new=0.9182736)


def bicg_scalars(kind):
    """rr[0], rho[k-1], rv[k], ts[k], tt[k], rr[k], rho[k].
    E: alpha = 4 / 2 = 2, omega = 8 / 2 = 4, beta = (16 / 4) * (2 / 4) = 2."""
    if kind == "E":
        return dict(rr0=1.0, rho_prev=4.0, rv=2.0, ts=8.0, tt=2.0, rr_new=16.0,
                    rho_new=16.0)
    return dict(rr0=3.0000001, rho_prev=1.5241577, rv=-0.7310585786,
                ts=0.6039207, tt=0.8414709848, rr_new=0.9182736,
                rho_new=-1.1447298858)


def cheb_scalars(kind):
    """b0 of step 0; a, b of a later step; s of cheb_scale"""
    if kind == "E":
        return dict(b0=2.0, a=4.0, b=2.0, s=0.5)
    return dict(b0=0.6180339887, a=0.4142135623, b=1.3247179572, s=2.7182818284)
