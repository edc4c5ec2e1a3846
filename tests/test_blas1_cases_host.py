"""blas1_cases.py held to its targets, without a GPU: the lengths, the data
sets, every reference against Fraction arithmetic, and numpy mutants of the
kernels that the cases must reject (the GPU tests are only as sharp as this)."""
from fractions import Fraction

import numpy as np
import pytest

import blas1_cases as bc

DOT_BLOCKS = 2048  # MI355X: 256 CUs x 8
F = Fraction


def frac_round(q):
    """a Fraction rounded to the nearest float64 (ties to even): int / int"""
    return np.float64(q.numerator / q.denominator)


def frac_vec(op, *vs):
    return np.array([frac_round(op(*[F(float(x)) for x in xs]))
                     for xs in zip(*vs)])


# ---------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------
def test_lengths_for_mi355x():
    assert bc.UNIT == 2048
    assert bc.small_lengths() == [0, 1, 2, 3, 511, 512, 513, 2047, 2048, 2049,
                                  4097]
    w = bc.wrap_length(DOT_BLOCKS)
    assert w == 4_194_304 and w <= bc.WRAP_MAX
    assert bc.wrap_lengths(DOT_BLOCKS) == [w - 1, w, w + 1, w + 2051]


@pytest.mark.parametrize("dot_blocks", [8, 304 * 8, 2048])
def test_lengths_follow_dot_blocks(dot_blocks):
    w = bc.wrap_length(dot_blocks)
    # W is the first length whose double2 count no longer fits one trip
    assert bc.stream_grid(w // 2, dot_blocks) == dot_blocks
    assert -(-(w // 2) // (dot_blocks * bc.K_U * bc.K_BLOCK)) == 1
    assert -(-((w + 2) // 2) // (dot_blocks * bc.K_U * bc.K_BLOCK)) == 2
    for n in bc.wrap_lengths(dot_blocks):
        assert abs(n - w) <= bc.UNIT + 3
    # the deepest chain grows by one trip's additions behind the wrap
    assert (bc.depth(w + 2, dot_blocks) - bc.depth(w, dot_blocks)
            == 2 * bc.K_U)


@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("wrap", [False, True])
def test_block_shapes_have_even_and_odd_rows(nrhs, wrap):
    ms = bc.block_shapes(nrhs, DOT_BLOCKS, wrap)
    assert any(m % 2 == 0 for m in ms) and any(m % 2 == 1 for m in ms)
    if wrap:  # on both sides of the wrap of the interleaved array
        w = bc.wrap_length(DOT_BLOCKS)
        assert min(ms) * nrhs < w < max(ms) * nrhs


def test_onehot_indices():
    idx = bc.onehot_indices(4097, 2)  # W = 4096 for two workgroups
    assert idx == [0, 1, 2047, 2048, 2049, 4095, 4096]
    assert bc.onehot_indices(3, 2) == [0, 1, 2]
    assert bc.onehot_indices(0, 2) == []


def test_depth_at_the_small_edges():
    # one trip: 8 products, the tail, 6 shuffles, 4 wave slots; the reducer:
    # 2048 / 256 partials per thread, 6 shuffles, 4 wave slots
    assert bc.depth(4097, DOT_BLOCKS) == (8 + 1 + 6 + 4) + (8 + 6 + 4)
    assert bc.depth(4097, DOT_BLOCKS, arrays=2) == 19 + 26
    assert bc.depth(4097, DOT_BLOCKS, streaming=False) == (1 + 11) + 18
    w = bc.wrap_length(DOT_BLOCKS)
    assert bc.depth(w + 1, DOT_BLOCKS, streaming=False) == (9 + 11) + 18


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def test_data_sets():
    e = bc.exact_vec(5000, 1)
    assert np.all(e == np.rint(e)) and np.all(e != 0)
    assert np.abs(e).max() <= 2 ** 10 and (e < 0).any() and (e > 0).any()
    assert set(bc.exact_dinv(500, 0)) == {1.0, 2.0, 4.0}
    r = bc.round_vec(5000, 1)
    ex = np.frexp(r)[1]
    assert ex.min() <= -14 and ex.max() >= 14 and (r < 0).any() and (r > 0).any()
    # irrational in the sense that matters: the mantissas use all 53 bits
    assert np.mean(np.frexp(r)[0] * 2.0 ** 53 % 2 == 1) > 0.3
    assert not np.array_equal(bc.exact_vec(9, 1), bc.exact_vec(9, 2))
    d = bc.round_dinv(100, 0)
    assert np.all(d > 0) and np.all(np.isfinite(d))


def test_scalar_sets_are_exact_where_promised():
    s = bc.cg_scalars("E")
    assert bc.cg_alpha(s["rr_prev"], s["pAp"]) == 2.0
    assert bc.cg_alpha(s["rr0"], s["pAp_prev"]) == 4.0
    assert bc.cg_beta(s["rr_new"], s["rr_prev"]) == 4.0
    assert not bc.converged(s["rr_new"], s["rr0"], bc.RTOL_GO)
    assert bc.converged(s["rr_new"], s["rr0"], bc.RTOL_STOP)
    s = bc.cg_scalars("R")
    for key in ("rr0", "rr_prev", "rr_new"):
        root = np.sqrt(np.float64(s[key]))
        assert F(float(root)) ** 2 == F(s[key])  # exact square of a 26-bit number
    # so alpha and beta are one correctly rounded division each
    assert bc.cg_alpha(s["rr_prev"], s["pAp"]) == frac_round(
        F(s["rr_prev"]) / F(s["pAp"]))
    assert bc.cg_beta(s["rr_new"], s["rr_prev"]) == frac_round(
        F(s["rr_new"]) / F(s["rr_prev"]))
    for kind in ("E", "R"):  # the branch is decided by a margin of 2**17 or more
        for sc in (bc.cg_scalars(kind), bc.pcg_scalars(kind),
                   bc.bicg_scalars(kind)):
            ratio = np.sqrt(sc["rr_new"] / sc["rr0"])
            assert bc.RTOL_GO * 2 ** 17 < ratio < bc.RTOL_STOP / 2 ** 17
    s = bc.pcg_scalars("E")
    assert bc.pcg_alpha(s["rz_prev"], s["pAp"]) == 2.0
    assert bc.pcg_beta(s["rz_new"], s["rz_prev"]) == 4.0
    s = bc.bicg_scalars("E")
    a, o = bc.pcg_alpha(s["rho_prev"], s["rv"]), bc.bicg_omega(s["ts"], s["tt"])
    assert (a, o) == (2.0, 4.0)
    assert bc.bicg_beta(s["rho_new"], s["rho_prev"], a, o) == 2.0
    assert bc.bicg_omega(1.0, 0.0) == 0.0


# ---------------------------------------------------------------------------
# references against Fraction arithmetic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 37])
def test_elementwise_references_round_twice(n):
    x, y, z, w = (bc.round_vec(n, s) for s in (1, 2, 3, 4))
    dinv = bc.round_dinv(n, 0)
    a, b = np.float64(0.7310585786), np.float64(-1.3247179572)

    def mul(p, q):
        return frac_vec(lambda s, t: s * t, p, q)

    def add(p, q):
        return frac_vec(lambda s, t: s + t, p, q)

    av, bv = np.full(n, a), np.full(n, b)
    assert bc.same_bits(bc.axpy(a, x, y), add(y, mul(av, x)))
    xr = bc.cg_update_xr(a, x, y, z, w)
    assert bc.same_bits(xr[0], add(z, mul(av, x)))
    assert bc.same_bits(xr[1], add(w, mul(-av, y)))
    assert bc.same_bits(bc.cg_update_r(a, y, w), xr[1])
    assert bc.same_bits(bc.cg_update_p(b, x, y), add(mul(bv, y), x))
    xn, pn = bc.cg_update_xp(a, b, False, x, y, z)
    assert bc.same_bits(xn, add(y, mul(av, z)))
    assert bc.same_bits(pn, add(mul(bv, z), x))
    xn, pn = bc.cg_update_xp(a, b, True, x, y, z)
    assert bc.same_bits(pn, z) and bc.same_bits(xn, add(y, mul(av, z)))
    xn, pn = bc.cg_update_x2p(b, a, b, False, x, y, z, w)
    assert bc.same_bits(xn, add(add(y, mul(bv, z)), mul(av, w)))
    assert bc.same_bits(pn, add(mul(bv, w), x))
    rn, zn = bc.pcg_update_r(a, x, dinv, y)
    assert bc.same_bits(rn, add(y, mul(-av, x)))
    assert bc.same_bits(zn, mul(dinv, rn))
    xn, pn = bc.pcg_update_xp(a, b, False, x, dinv, y, z)
    assert bc.same_bits(pn, add(mul(bv, z), mul(dinv, x)))
    s, sh = bc.bicg_update_s(a, x, y, dinv)
    assert bc.same_bits(s, add(x, -mul(av, y))) and bc.same_bits(sh, mul(dinv, s))
    assert bc.bicg_update_s(a, x, y, None)[1] is None
    xn, rn = bc.bicg_update_xr(a, b, x, y, z, w, s)
    assert bc.same_bits(xn, add(add(s, mul(av, x)), mul(bv, y)))
    assert bc.same_bits(rn, add(z, -mul(bv, w)))
    xn2, _ = bc.bicg_update_xr(a, b, x, None, z, w, s)
    assert bc.same_bits(xn2, add(add(s, mul(av, x)), mul(bv, z)))
    pn, ph = bc.bicg_update_p(a, b, x, y, dinv, z)
    assert bc.same_bits(pn, add(x, mul(av, add(z, -mul(bv, y)))))
    assert bc.same_bits(ph, mul(dinv, pn))
    assert bc.same_bits(bc.cheb_scale(a, dinv, x),
                        mul(dinv, frac_vec(lambda s, t: s / t, x, av)))
    assert bc.same_bits(bc.cheb_apply0(a, x, dinv), mul(av, mul(dinv, x)))
    assert bc.same_bits(bc.cheb_apply0(a, x, None), mul(av, x))
    dn, zn = bc.cheb_step(a, b, w, x, dinv, y, z)
    assert bc.same_bits(dn, add(mul(av, y), mul(bv, mul(dinv, add(x, -w)))))
    assert bc.same_bits(zn, add(z, dn))
    assert bc.same_bits(bc.cg_residual(x, y), add(x, -y))


@pytest.mark.parametrize("n", [0, 1, 2, 513])
def test_sum_references(n):
    a, b = bc.exact_vec(n, 1), bc.exact_vec(n, 2)
    assert bc.exact_dot_int(a, b) == sum(int(s) * int(t) for s, t in zip(a, b))
    x, y = bc.round_vec(n, 1), bc.round_vec(n, 2)
    s, sa = bc.exact_dot(x, y)
    assert s == sum((F(float(p)) * F(float(q)) for p, q in zip(x, y)), F(0))
    assert sa == sum((abs(F(float(p)) * F(float(q))) for p, q in zip(x, y)), F(0))
    # a plain float64 loop, whatever its order, lies inside the bound of its
    # own depth (n additions): the bound is a bound
    acc = np.float64(0)
    for p, q in zip(x, y):
        acc = acc + p * q
    assert bc.sum_within(acc, s, sa, max(n, 1))


def test_sum_bound_formula():
    assert bc.sum_bound(36, 1) == F(37, 2 ** 53) / (1 - F(37, 2 ** 53))
    assert bc.sum_bound(36, 3, roundings=2) == 3 * F(38, 2 ** 53) / (
        1 - F(38, 2 ** 53))


def test_same_bits_sees_signed_zero():
    assert not bc.same_bits(np.array([0.0]), np.array([-0.0]))
    assert bc.same_bits(np.array([np.nan]), np.array([np.nan]))


# ---------------------------------------------------------------------------
# mutants: each must be rejected by the check the GPU tests apply
# ---------------------------------------------------------------------------
N_MUT = 4097


def tree_dot(x, y, dot_blocks, *, acc_dtype=np.float64, skip=()):
    """numpy model of dot_partial + reduce_partials: this thread's products in
    trip order, shuffle tree, wave slots, then the reducer's tree"""
    n = len(x)
    n2 = n // 2
    g = bc.stream_grid(n2, dot_blocks)
    acc = np.zeros((g, bc.K_BLOCK), acc_dtype)
    xs, ys = x.astype(acc_dtype), y.astype(acc_dtype)
    step = bc.K_U * bc.K_BLOCK
    for base in range(0, max(n2, 1), g * step):
        for blk in range(g):
            for u in range(bc.K_U):
                i = base + blk * step + u * bc.K_BLOCK + np.arange(bc.K_BLOCK)
                ok = i < n2
                for h in (0, 1):
                    j = np.where(ok, 2 * i + h, 0)
                    t = np.where(ok & ~np.isin(2 * i + h, skip),
                                 xs[j] * ys[j] if n else 0, 0).astype(acc_dtype)
                    acc[blk] += t
    if n & 1 and (n - 1) not in skip:
        acc[0, 0] += xs[n - 1] * ys[n - 1]

    def block_sum(v):
        v = v.copy()
        for off in (32, 16, 8, 4, 2, 1):
            w = v.reshape(-1, 64)
            w[:, :off] += w[:, off:2 * off]
        r = acc_dtype(0)
        for wv in range(bc.K_BLOCK // 64):
            r = r + v[64 * wv]
        return r

    partials = np.zeros(dot_blocks, acc_dtype)
    for blk in range(g):
        partials[blk] = block_sum(acc[blk])
    racc = np.zeros(bc.K_BLOCK, acc_dtype)
    for i0 in range(0, dot_blocks, bc.K_BLOCK):
        chunk = partials[i0:i0 + bc.K_BLOCK]
        racc[:len(chunk)] += chunk
    return np.float64(block_sum(racc)), partials


def test_the_model_itself_passes():
    x, y = bc.exact_vec(N_MUT, 1), bc.exact_vec(N_MUT, 2)
    s, _ = tree_dot(x, y, 8)
    assert s == bc.exact_dot_int(x, y)
    xr, yr = bc.round_vec(N_MUT, 1), bc.round_vec(N_MUT, 2)
    s, partials = tree_dot(xr, yr, 8)
    ex, sa = bc.exact_dot(xr, yr)
    assert bc.sum_within(s, ex, sa, bc.depth(N_MUT, 8))
    assert np.all(partials[bc.stream_grid(N_MUT // 2, 8):] == 0)


def test_mutant_fused_multiply_add():
    s = bc.cg_scalars("R")
    alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
    n = 513
    p, x = bc.round_vec(n, 1), bc.round_vec(n, 2)
    fused = frac_vec(lambda a, b, c: a * b + c, np.full(n, alpha), p, x)
    good = bc.axpy(alpha, p, x)
    assert not bc.same_bits(fused, good)
    # not by one lucky element: a tenth of them move, in every lane position
    moved = fused != good
    assert moved.mean() > 0.1 and moved[0::2].any() and moved[1::2].any()
    # ... and in set E the two agree: it is set R that holds the rounding
    pe, xe = bc.exact_vec(n, 1), bc.exact_vec(n, 2)
    assert bc.same_bits(frac_vec(lambda a, b, c: a * b + c,
                                 np.full(n, 2.0), pe, xe),
                        bc.axpy(2.0, pe, xe))


def test_mutant_fp32_accumulation():
    x, y = bc.exact_vec(N_MUT, 1), bc.exact_vec(N_MUT, 2)
    s, _ = tree_dot(x, y, 8, acc_dtype=np.float32)
    assert s != bc.exact_dot_int(x, y)
    xr, yr = bc.round_vec(N_MUT, 1), bc.round_vec(N_MUT, 2)
    s, _ = tree_dot(xr, yr, 8, acc_dtype=np.float32)
    ex, sa = bc.exact_dot(xr, yr)
    assert not bc.sum_within(s, ex, sa, bc.depth(N_MUT, 8))


def test_mutant_skips_odd_tail():
    x, y = bc.exact_vec(N_MUT, 1), bc.exact_vec(N_MUT, 2)
    s, _ = tree_dot(x, y, 8, skip=(N_MUT - 1,))
    assert s != bc.exact_dot_int(x, y)
    # the one-hot probe at n - 1 sees it too
    e = np.zeros(N_MUT)
    e[-1] = 1.0
    assert tree_dot(e, y, 8, skip=(N_MUT - 1,))[0] != y[-1]
    assert tree_dot(e, y, 8)[0] == y[-1]


def test_mutant_skips_first_element_of_second_trip():
    db = 2
    w = bc.wrap_length(db)
    for n in bc.wrap_lengths(db)[2:]:  # W + 1, W + unit + 3: a second trip
        x, y = bc.exact_vec(n, 1), bc.exact_vec(n, 2)
        assert tree_dot(x, y, db)[0] == bc.exact_dot_int(x, y)
        assert tree_dot(x, y, db, skip=(w,))[0] != bc.exact_dot_int(x, y)
    assert w in bc.onehot_indices(w + 1, db)


@pytest.mark.parametrize("kind", ["E", "R"])
def test_mutant_alpha_from_the_wrong_slot(kind):
    s = bc.cg_scalars(kind)
    vec = bc.exact_vec if kind == "E" else bc.round_vec
    p, x = vec(513, 1), vec(513, 2)
    good = bc.axpy(bc.cg_alpha(s["rr_prev"], s["pAp"]), p, x)
    assert not bc.same_bits(bc.axpy(bc.cg_alpha(s["rr_new"], s["pAp"]), p, x),
                            good)
    assert not bc.same_bits(bc.axpy(bc.cg_alpha(s["rr0"], s["pAp"]), p, x), good)
    for sc, a, b in ((bc.pcg_scalars(kind), "rz_prev", "rz_new"),
                     (bc.bicg_scalars(kind), "rho_prev", "rho_new")):
        den = sc["pAp"] if "pAp" in sc else sc["rv"]
        assert not bc.same_bits(bc.axpy(bc.pcg_alpha(sc[a], den), p, x),
                                bc.axpy(bc.pcg_alpha(sc[b], den), p, x))


@pytest.mark.parametrize("kind", ["E", "R"])
def test_mutant_converged_branch_updates_p(kind):
    s = bc.cg_scalars(kind)
    vec = bc.exact_vec if kind == "E" else bc.round_vec
    r, x, p = vec(513, 1), vec(513, 2), vec(513, 3)
    alpha = bc.cg_alpha(s["rr_prev"], s["pAp"])
    beta = bc.cg_beta(s["rr_new"], s["rr_prev"])
    xn, pn = bc.cg_update_xp(alpha, beta, True, r, x, p)
    xm, pm = bc.cg_update_xp(alpha, beta, False, r, x, p)  # the mutant
    assert bc.same_bits(xn, xm) and bc.same_bits(pn, p)
    assert not bc.same_bits(pm, pn)
    # every element moves, so a partial write cannot hide either
    assert np.all(pm != pn)
