"""The life cycle of the eleven solver workspaces through the C ABI alone:
create, capacity, reset, read_async, the test hooks, destroy, create again.

Nothing here launches a solver kernel; what is pinned is the plumbing every
workspace shares (spmv_amd/csrc/hip/ws_core.h, solver_ws.h) as include/spmv_hip.h
documents it per solver:

  state words after reset (read_async copies them from `done` on)
    cg, pcg            {done, kstop}                    = 0, -1
    bicgstab, minres,
    lsqr               {done, kstop, status}            = 0, -1, 0
    gmres, idrs        {done, kstop, status, k}         = 0, -1, 0, 0
    cg_shifted         {done, kstop, status, its[8]}    = 0, -1, 0, 0 x 8
    cg_block,
    pcg_block          {all_done, done[8], kstop[8]}    = 0, 0 x 8, -1 x 8
    lobpcg             {done, kstop, status, it, active, has_p, restarts, basis}
                                                         = 0, 0, 0, 0, 2^nev - 1, 0, 0, 0
  history the read copies, in doubles, zero after reset (lobpcg: -1.0)
    cg, gmres, minres, idrs   kmax + 1
    pcg, bicgstab, lsqr       2 (kmax + 1)   (pairs: rz/rr, rr/rho, hist_r/hist_ar)
    cg_shifted                8 (kmax + 1)
    cg_block                  (kmax + 1) nrhs
    pcg_block                 2 (kmax + 1) nrhs
    lobpcg                    (kmax + 1) nev

A history buffer one double short gets SPMV_HIP_EINVAL and nothing is enqueued:
both destinations keep their sentinel.  No workspace is used after destroy."""
import ctypes as C

import numpy as np
import pytest

from spmv_amd import _lib, host

pytestmark = pytest.mark.gpu

EINVAL = -1
WORD_SENTINEL, HIST_SENTINEL = 99, -7.0
MAX_BLOCK = 8  # SPMV_HIP_CGB_MAX_NRHS, and the widest lobpcg block
RTOL = 1e-8


@pytest.fixture(scope="module")
def exec_():
    e = host.HipExecutor(0)
    yield e
    e.synchronize()
    e.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Spec:
    """What differs between the workspaces: the arguments of create and reset,
    the state words and the history after reset, and the optional hooks."""
    block = False        # create and capacity take a block width
    state_len_arg = False  # read_async takes the length of the state buffer
    scalars_arg = False  # read_async takes a third destination
    hist_fill = 0.0
    array = False        # has _ws_array
    unknown_which = ()

    def __init__(self, prefix):
        self.prefix = prefix

    def fn(self, name):
        return getattr(_lib.hip, f"spmv_hip_{self.prefix}_ws_{name}")

    def reset_args(self, kmax, width):
        return (RTOL,)

    def round_trip(self, ws, kmax, width, sync):
        pass


class Pairs(Spec):
    def __init__(self, prefix, state, per_step):
        super().__init__(prefix)
        self._state, self.per_step = state, per_step

    def state(self, kmax, width):
        return list(self._state)

    def hist_len(self, kmax, width):
        return self.per_step * (kmax + 1)


class Block(Pairs):
    block = state_len_arg = True

    def state(self, kmax, width):
        return [0] + [0] * MAX_BLOCK + [-1] * MAX_BLOCK

    def hist_len(self, kmax, width):
        return self.per_step * (kmax + 1) * width


class StateHooks(Pairs):
    """gmres, minres, lsqr: set_state installs k and done (kstop = k), get_state
    reads the words back."""
    array = True

    def __init__(self, prefix, state, per_step, reset_tail, unknown_which, gmres):
        super().__init__(prefix, state, per_step)
        self._reset_tail, self.unknown_which, self._gmres = (reset_tail,
                                                             unknown_which, gmres)

    def reset_args(self, kmax, width):
        return (RTOL,) + self._reset_tail(kmax)

    def round_trip(self, ws, kmax, width, sync):
        k = kmax
        if self._gmres:  # {done, kstop, status, k, jn, finished}
            _lib.check(self.fn("set_state")(ws, k, 1, 1, 0, None), "set_state")
            want = [1, k, 0, k, 1, 0]
        else:            # {done, kstop, status, k, kmax}
            _lib.check(self.fn("set_state")(ws, k, 1, None), "set_state")
            want = [1, k, 0, k, kmax]
        got = np.full(len(want), WORD_SENTINEL, np.int32)
        _lib.check(self.fn("get_state")(ws, _vp(got), None), "get_state")
        sync()
        assert list(got) == want
        # a running state again: kstop = -1
        args = (0, 0, 0, 0) if self._gmres else (0, 0)
        _lib.check(self.fn("set_state")(ws, *args, None), "set_state")
        _lib.check(self.fn("get_state")(ws, _vp(got), None), "get_state")
        sync()
        assert list(got[:4]) == [0, -1, 0, 0]


class WordHooks(Pairs):
    """cg_shifted, idrs: set_words installs every word, get_words reads them."""
    array = True

    def __init__(self, prefix, state, per_step, unknown_which):
        super().__init__(prefix, state, per_step)
        self.unknown_which = unknown_which

    def round_trip(self, ws, kmax, width, sync):
        reset = self.words_after_reset(kmax)
        got = np.full(len(reset), WORD_SENTINEL, np.int32)
        _lib.check(self.fn("get_words")(ws, _vp(got), None), "get_words")
        sync()
        assert list(got) == reset
        put = np.array(self.words_to_set(kmax), np.int32)
        _lib.check(self.fn("set_words")(ws, _vp(put), None), "set_words")
        got[:] = WORD_SENTINEL
        _lib.check(self.fn("get_words")(ws, _vp(got), None), "get_words")
        sync()
        assert list(got) == list(put)


class Cgs(WordHooks):
    NS = 3
    shifts = np.array([0.0, 0.5, 2.0])

    def reset_args(self, kmax, width):
        return (RTOL, kmax, self.NS, _vp(self.shifts))

    def words_after_reset(self, kmax):
        # done, kstop, status, its[8], k, kmax, ns, n_act, n_upd, act[8], upd[8]
        act = list(range(self.NS)) + [0] * (8 - self.NS)
        return [0, -1, 0] + [0] * 8 + [0, kmax, self.NS, self.NS, 0] + act + [0] * 8

    def words_to_set(self, kmax):
        its = [kmax, 0, kmax] + [0] * 5
        return ([1, kmax, 0] + its + [kmax, kmax, self.NS, 2, 1]
                + [0, 2] + [0] * 6 + [1 | 8] + [0] * 7)


class Idrs(WordHooks):
    S = 4

    def reset_args(self, kmax, width):
        return (RTOL, 0.7, kmax, self.S, 12345)

    def words_after_reset(self, kmax):  # done, kstop, status, k, kmax, s
        return [0, -1, 0, 0, kmax, self.S]

    def words_to_set(self, kmax):
        return [1, kmax, 2, kmax, kmax, self.S]


class Lobpcg(Spec):
    block = scalars_arg = array = True
    hist_fill = -1.0
    unknown_which = (-1, 7)

    def reset_args(self, kmax, width):
        return (RTOL, 0.0, kmax, 0)

    def state(self, kmax, width):
        return [0, 0, 0, 0, (1 << width) - 1, 0, 0, 0]

    def hist_len(self, kmax, width):
        return (kmax + 1) * width

    def round_trip(self, ws, kmax, width, sync):
        # set_state installs active, has_p, it and done; read_async shows them
        _lib.check(self.fn("set_state")(ws, 1, 1, kmax, 1, None), "set_state")
        got = np.full(8, WORD_SENTINEL, np.int32)
        _lib.check(self.fn("read_async")(ws, _vp(got), None, 0, None, None),
                   "read_async")
        sync()
        assert list(got) == [1, 0, 0, kmax, 1, 1, 0, 0]


SPECS = {
    "cg": Pairs("cg", (0, -1), 1),
    "pcg": Pairs("pcg", (0, -1), 2),
    "bicgstab": Pairs("bicg", (0, -1, 0), 2),
    "gmres": StateHooks("gmres", (0, -1, 0, 0), 1, lambda kmax: (kmax, 30),
                        (-1, 12), True),
    "minres": StateHooks("minres", (0, -1, 0), 1, lambda kmax: (kmax,), (-1, 6),
                         False),
    "lsqr": StateHooks("lsqr", (0, -1, 0), 2, lambda kmax: (1e-9, 0.25, kmax),
                       (-1, 7), False),
    "cg_shifted": Cgs("cgs", (0, -1, 0) + (0,) * 8, 8, (-1, 6)),
    "idrs": Idrs("idrs", (0, -1, 0, 0), 1, (-1, 4)),
    "cg_block": Block("cgb", None, 1),
    "pcg_block": Block("pcgb", None, 2),
    "lobpcg": Lobpcg("lobpcg"),
}
CASES = [(name, kmax, width) for name, spec in SPECS.items()
         for kmax in (0, 1, 5)
         for width in ((1, MAX_BLOCK) if spec.block else (0,))]


def _read(spec, ws, words, hist, hist_len, scalars=None):
    args = [ws, _vp(words)]
    if spec.state_len_arg:
        args.append(len(words))
    args += [_vp(hist), hist_len]
    if spec.scalars_arg:
        args.append(None if scalars is None else _vp(scalars))
    return spec.fn("read_async")(*args, None)


def _create(spec, ctx, kmax, width):
    ws = C.c_void_p()
    args = (ctx, kmax, width) if spec.block else (ctx, kmax)
    _lib.check(spec.fn("create")(*args, C.byref(ws)), spec.prefix + "_ws_create")
    assert ws.value
    return ws


def _check_capacity(spec, ws, kmax, width):
    cap, cap_width = C.c_int(-1), C.c_int(-1)
    if spec.block:
        _lib.check(spec.fn("capacity")(ws, C.byref(cap), C.byref(cap_width)),
                   "capacity")
        assert (cap.value, cap_width.value) == (kmax, width)
    else:
        _lib.check(spec.fn("capacity")(ws, C.byref(cap)), "capacity")
        assert cap.value == kmax


def _check_reset_and_read(spec, ws, kmax, width, sync):
    _lib.check(spec.fn("reset")(ws, *spec.reset_args(kmax, width), None), "reset")
    want = spec.state(kmax, width)
    n = spec.hist_len(kmax, width)
    words = np.full(len(want), WORD_SENTINEL, np.int32)
    hist = np.full(n, HIST_SENTINEL)
    # one double short: refused before anything is enqueued
    assert _read(spec, ws, words, hist, n - 1) == EINVAL
    sync()
    assert np.all(words == WORD_SENTINEL) and np.all(hist == HIST_SENTINEL)
    scalars = np.full(3 * width, HIST_SENTINEL) if spec.scalars_arg else None
    _lib.check(_read(spec, ws, words, hist, n, scalars), "read_async")
    sync()
    assert list(words) == want
    assert np.all(hist == spec.hist_fill)
    if scalars is not None:  # theta, then the two halves of RN
        assert np.all(scalars == 0.0)


@pytest.mark.parametrize("name,kmax,width", CASES)
def test_workspace_life_cycle(exec_, name, kmax, width):
    spec, ctx, sync = SPECS[name], exec_.context, exec_.synchronize
    ws = _create(spec, ctx, kmax, width)
    try:
        _check_capacity(spec, ws, kmax, width)
        _check_reset_and_read(spec, ws, kmax, width, sync)
        spec.round_trip(ws, kmax, width, sync)
        if spec.array:
            p, n = C.c_void_p(), C.c_int64()
            for which in spec.unknown_which:
                assert spec.fn("array")(ws, which, C.byref(p),
                                        C.byref(n)) == EINVAL
            _lib.check(spec.fn("array")(ws, spec.unknown_which[1] - 1,
                                        C.byref(p), C.byref(n)), "array")
            assert p.value and n.value >= 1
    finally:
        sync()
        _lib.check(spec.fn("destroy")(ws), "destroy")
    # a second, larger workspace after the first is gone
    ws = _create(spec, ctx, kmax + 3, width)
    try:
        _check_capacity(spec, ws, kmax + 3, width)
        _check_reset_and_read(spec, ws, kmax + 3, width, sync)
    finally:
        sync()
        _lib.check(spec.fn("destroy")(ws), "destroy")
    assert spec.fn("destroy")(None) == 0
