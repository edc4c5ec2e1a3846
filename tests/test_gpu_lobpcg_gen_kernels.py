"""The kernels of the pencil form of spmv::lobpcg (hip/blas1_lobpcg.hip: gram_gen,
update_gen, residual_gen) alone through the C ABI, bit for bit against
lobpcg_gen_cases.py: nev in {1, 2, 3, 4, 5, 8} (the native widths and two
run-time ones), blocks 1 and 3, the edge lengths of test_gpu_lobpcg_kernels.py
(M = 0, 1, the chunk edges 63 / 64 / 65, the workgroup edges) with 127 / 128 /
129 added, the wrap lengths of blas1_cases.py, the Gram kernel's own wrap,
aligned and 8-byte-offset blocks, cached and non-temporal accesses, the masks
all / one column / all but one / a compacted one (0b111010), P absent, and
`done`."""
import numpy as np
import pytest

import lobpcg_cases as lc
import lobpcg_gen_cases as lg
from spmv_amd import _lib
from test_gpu_lobpcg_kernels import (GPART, GRAM, RPART, THETA, Blocks, Ws,
                                     _data, _partials_len, _run_rr, _spd_pencil,
                                     lc_sentinel, lengths, same_bits,
                                     same_values, wrap_lengths)
from test_gpu_pcg import exec_, nt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NEV = (1, 2, 3, 4, 5, 8)


def gen_lengths(nev, L):
    return sorted(set(lengths(nev, L)) | {127, 128, 129})


def masks_of(nev):
    full = (1 << nev) - 1
    return sorted({full, 1, full & ~1, 0b111010 & full} - {0})


# ---- gram ---------------------------------------------------------------------
def _gram_gen(ws, M, nb, B):
    _lib.call("spmv_hip_lobpcg_gram_gen_f64", ws.ctx, ws.h, M, nb, *B.ptr, None)
    _lib.call("spmv_hip_lobpcg_gram_reduce", ws.ctx, ws.h, M, nb, None)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", NEV)
def test_gram_gen(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    for M in gen_lengths(nev, _partials_len(exec_)):
        for nb, cancel in ((3, False), (1, False), (3, True)):
            d = _data(M, nev, 9, M + nev, cancel)
            B = Blocks(exec_, d, off)
            _gram_gen(ws, M, nb, B)
            grid, m = ws.gram_grid(M), nb * nev
            S, AS, BS = (np.concatenate(d[i:i + nb], axis=1) for i in (0, 3, 6))
            want = lg.gram_partials_gen(S, AS, BS, grid)
            got = ws.get(GPART, grid * 2 * m * m).reshape(grid, 2, m, m)
            assert same_values(got, want), (M, nb, cancel)
            slot = ws.get(GRAM, 2 * m * m).reshape(2, m, m)
            assert same_values(slot, lc.gram_sum(want)), (M, nb, cancel)
            if cancel and M >= 255 and nev > 1:  # B's operand and the order show
                assert not np.array_equal(slot[0], np.triu(S.T @ BS))
                assert not np.array_equal(slot[0], lc.gram_sum(
                    lc.gram_partials(S, AS, grid))[0])
            B.close()
    ws.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", NEV)
def test_gram_gen_with_bs_at_s_is_the_six_block_kernel(exec_, nt, nev, off):  # noqa: F811
    """BS pointing at S: spmv_hip_lobpcg_gram_f64's partials exactly"""
    ws = Ws(exec_, nev)
    cap = ws.gram_grid(1 << 40)
    for M in (0, 1, 63, 64, 65, 127, 128, 129, 1331, 64 * cap + 65):
        for nb in (3, 1):
            d = _data(M, nev, 6, M + 3 * nev, cancel=M < 5000)
            B = Blocks(exec_, d, off)
            grid, m = ws.gram_grid(M), nb * nev
            ws.put(GPART, np.full(grid * 2 * m * m, lc_sentinel()))
            _lib.call("spmv_hip_lobpcg_gram_f64", ws.ctx, ws.h, M, nb, *B.ptr, None)
            six = ws.get(GPART, grid * 2 * m * m)
            ws.put(GPART, np.full(grid * 2 * m * m, lc_sentinel()))
            _lib.call("spmv_hip_lobpcg_gram_gen_f64", ws.ctx, ws.h, M, nb, *B.ptr,
                      *B.ptr[:3], None)
            nine = ws.get(GPART, grid * 2 * m * m)
            assert same_bits(six, nine), (M, nb)
            assert not np.any(nine == lc_sentinel())
            B.close()
    ws.close()


@pytest.mark.parametrize("nev", NEV)
def test_gram_gen_wraps_the_grid(exec_, nt, nev):  # noqa: F811
    """more chunks than workgroups: workgroup 0 takes a second chunk, the last
    chunk is a partial one"""
    ws = Ws(exec_, nev)
    cap = ws.gram_grid(1 << 40)
    M, m = 64 * cap + 65, 3 * nev
    d = _data(M, nev, 9, 7 + nev)
    B = Blocks(exec_, d, nev % 2)
    _lib.call("spmv_hip_lobpcg_gram_gen_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    assert ws.gram_grid(M) == cap
    want = lg.gram_partials_gen(*(np.concatenate(d[i:i + 3], axis=1)
                                  for i in (0, 3, 6)), cap)
    got = ws.get(GPART, cap * 2 * m * m).reshape(cap, 2, m, m)
    assert same_values(got, want)
    B.close()
    ws.close()


def test_gram_gen_after_done(exec_):  # noqa: F811
    nev, M = 4, 300
    ws = Ws(exec_, nev)
    B = Blocks(exec_, _data(M, nev, 9, 1), 0)
    n = ws.gram_grid(M) * 2 * 144
    ws.put(GPART, np.full(n, lc_sentinel()))
    ws.set_state(15, 1, done=1)
    _lib.call("spmv_hip_lobpcg_gram_gen_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    assert np.all(ws.get(GPART, n) == lc_sentinel())
    B.close()
    ws.close()


# ---- update ---------------------------------------------------------------------
def _check_update_gen(ws, exec_, nev, M, off, active, has_p):  # noqa: F811
    gram = np.stack(_spd_pencil(3 * nev, M % 97 + active))
    want = lc.rr_ref(gram, nev, 3, active, has_p)
    _run_rr(ws, gram, 3, active, has_p)
    d = _data(M, nev, 9, M)
    B = Blocks(exec_, d, off)
    _lib.call("spmv_hip_lobpcg_update_gen_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    outs = lg.update_gen([d[0:3], d[3:6], d[6:9]], want["coef"], want["basis"],
                         active, nev)
    what = (M, active, has_p)
    for t, (xo, po) in enumerate(outs):
        assert same_values(B.get(3 * t, (M, nev)), xo), (what, t, "x")
        assert same_bits(B.get(3 * t + 1, (M, nev)), d[3 * t + 1]), (what, t, "w")
        got_p = B.get(3 * t + 2, (M, nev))
        assert same_values(got_p, po), (what, t, "p")
        for c in range(nev):  # an inactive column's P is left alone
            if not (active >> c) & 1:
                assert same_bits(got_p[:, c], d[3 * t + 2][:, c])
    B.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", NEV)
def test_update_gen(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    full = (1 << nev) - 1
    for M in gen_lengths(nev, _partials_len(exec_)):
        for active in (masks_of(nev) if M in (129, 1331) else [full]):
            for has_p in ((1, 0) if M in (65, 1331) else (1,)):
                _check_update_gen(ws, exec_, nev, M, off, active, has_p)
    # one block: the prologue's X R^-1 and BX R^-1, without and with AX
    M = 257
    gram = np.stack(_spd_pencil(nev, 4))
    want = lc.rr_ref(gram, nev, 1, full, 0, mode=1)
    _run_rr(ws, gram, 1, full, 0, mode=1, advance=0)
    for with_ax in (False, True):
        d = _data(M, nev, 3, 11)
        B = Blocks(exec_, d, off)
        _lib.call("spmv_hip_lobpcg_update_gen_f64", ws.ctx, ws.h, M, 1, B.ptr[0],
                  None, None, B.ptr[1] if with_ax else None, None, None, B.ptr[2],
                  None, None, None)
        ref = [lc.combine([a], want["coef"], want["basis"], full, nev)[0]
               for a in d]
        assert same_values(B.get(0, (M, nev)), ref[0])
        assert same_values(B.get(1, (M, nev)), ref[1] if with_ax else d[1])
        assert same_values(B.get(2, (M, nev)), ref[2])
        B.close()
    # after done every output is untouched
    d = _data(M, nev, 9, 12)
    B = Blocks(exec_, d, off)
    ws.set_state(full, 0, done=1)
    _lib.call("spmv_hip_lobpcg_update_gen_f64", ws.ctx, ws.h, M, 3, *B.ptr, None)
    for i in range(9):
        assert same_bits(B.get(i, (M, nev)), d[i]), i
    B.close()
    ws.close()


@pytest.mark.parametrize("nev", NEV)
def test_update_gen_has_the_bits_of_update(exec_, nt, nev):  # noqa: F811
    """the triples [X, W, P] and [AX, AW, AP] through update_gen and through
    spmv_hip_lobpcg_update_f64: the same bits"""
    ws = Ws(exec_, nev)
    M = 1331
    for active in masks_of(nev):
        gram = np.stack(_spd_pencil(3 * nev, active))
        _run_rr(ws, gram, 3, active, 1)
        d = _data(M, nev, 9, active)
        B6, B9 = Blocks(exec_, d[:6], 0), Blocks(exec_, d, 0)
        _lib.call("spmv_hip_lobpcg_update_f64", ws.ctx, ws.h, M, 3, *B6.ptr, None)
        _lib.call("spmv_hip_lobpcg_update_gen_f64", ws.ctx, ws.h, M, 3, *B9.ptr,
                  None)
        for i in range(6):
            assert same_bits(B6.get(i, (M, nev)), B9.get(i, (M, nev))), (active, i)
        B6.close()
        B9.close()
    ws.close()


@pytest.mark.parametrize("slot", range(4))
@pytest.mark.parametrize("nev", NEV)
def test_update_gen_wraps_the_grid(exec_, nt, nev, slot):  # noqa: F811
    """a thread takes a second row: every width"""
    ws = Ws(exec_, nev)
    full = (1 << nev) - 1
    L = _partials_len(exec_)
    for M in wrap_lengths(nev, L, slot):
        assert M > 256 * L - 2
        _check_update_gen(ws, exec_, nev, M, slot % 2,
                          full if slot else full & ~1 or full, 1)
    ws.close()


# ---- residual ---------------------------------------------------------------------
def _check_residual_gen(ws, exec_, nev, M, off, with_dinv, L, done=0):  # noqa: F811
    full = (1 << nev) - 1
    rng = np.random.default_rng(M)
    theta = rng.uniform(0.5, 2.0, nev)
    AX, BX = _data(M, nev, 2, M + 1)
    dinv = rng.uniform(0.5, 2.0, M + 1)
    ws.reset(rtol=2.0 ** -20, atol=0.0)
    ws.set_state(full, 0, it=2, done=done)
    ws.put(THETA, theta)
    ws.put(RPART, np.full(L * nev, lc_sentinel()))
    fill = np.full((M, nev), lc_sentinel())
    B = Blocks(exec_, [AX, BX, fill, fill], off)
    d_dinv = exec_.alloc(M + 1)
    exec_.copy_from_host(d_dinv, dinv)
    _lib.call("spmv_hip_lobpcg_residual_gen_f64", ws.ctx, ws.h, M, B.ptr[0],
              B.ptr[1], d_dinv if with_dinv else None, B.ptr[2], B.ptr[3], 0,
              None)
    got_r, got_w = B.get(2, (M, nev)), B.get(3, (M, nev))
    got_p = ws.get(RPART).reshape(L, nev)
    if done:
        assert np.all(got_r == lc_sentinel()) and np.all(got_w == lc_sentinel())
        assert np.all(got_p == lc_sentinel())
    else:
        R, W, r2 = lg.residual_gen(AX, BX, theta, dinv[:M] if with_dinv else None)
        assert same_values(got_r, R), (M, with_dinv)
        assert same_values(got_w, W), (M, with_dinv)
        grid = lc.rows_grid(M, L)
        assert same_values(got_p[:grid], lc.rows_partials(r2, grid)), M
        assert np.all(got_p[grid:] == 0.0), M
    exec_.free(d_dinv)
    B.close()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("nev", NEV)
def test_residual_gen(exec_, nt, nev, off):  # noqa: F811
    ws = Ws(exec_, nev)
    L = _partials_len(exec_)
    for M in gen_lengths(nev, L):
        for with_dinv in (False, True):
            _check_residual_gen(ws, exec_, nev, M, off, with_dinv, L)
    _check_residual_gen(ws, exec_, nev, 300, off, True, L, done=1)
    ws.close()


@pytest.mark.parametrize("slot", range(4))
@pytest.mark.parametrize("nev", NEV)
def test_residual_gen_wraps_the_grid(exec_, nt, nev, slot):  # noqa: F811
    ws = Ws(exec_, nev)
    L = _partials_len(exec_)
    for M in wrap_lengths(nev, L, slot):
        _check_residual_gen(ws, exec_, nev, M, 0, bool(slot % 2), L)
    ws.close()
