"""The device setup of AmgPreconditioner (hip/spmv_amg_build.hip) restated in
numpy.  Shared by test_amg_device_host.py and test_gpu_amg_device.py.

aggregate_by_priority is the DEFINITION: the three passes of host/amg_build.h
as sequential loops, with "i ascending" read as "i in descending priority".
aggregate_in_rounds simulates the device's scheme launch by launch (bid / take,
push / take) and also counts the rounds.  Both take the expanded rows of
amg_cases.expand; everything else of a step and of the hierarchy is
amg_cases.coarsen / AmgRef with the aggregate function swapped (swapped())."""
import contextlib

import numpy as np

import amg_cases as ac
import gmres_cases as gc
import ilu0_cases as ic
import test_amg_host as tah

ORDERS = ("natural", "hashed")
MASK = (1 << 64) - 1


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def priorities(n, order):
    """-> list of n Python ints, no two equal, none 0"""
    if order == "natural":
        return [n - i for i in range(n)]
    assert order == "hashed", order
    return [_mix64(((i + 1) * 0x9E3779B97F4A7C15) & MASK) for i in range(n)]


def strong_lists(ptr, col, val, n, theta):
    """strong(i) in expanded order, a column once (amg_build.cpp:103-119)"""
    out = []
    for i in range(n):
        c, a = col[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
        m = 0.0
        for j, v in zip(c.tolist(), a.tolist()):
            if j != i and abs(v) > m:  # (a NaN never replaces a number)
                m = abs(v)
        bar = theta * m
        seen, s = set(), []
        for j, v in zip(c.tolist(), a.tolist()):
            if j != i and v != 0.0 and abs(v) >= bar and j not in seen:
                seen.add(j)
                s.append(j)
        out.append(s)
    return out


def _number(n, owner, roots1, roots3):
    """pass-1 roots ascending by row, then pass-3 roots ascending by row"""
    number = {r: k for k, r in enumerate(sorted(roots1))}
    number.update({r: len(roots1) + k for k, r in enumerate(sorted(roots3))})
    return np.array([number[owner[i]] for i in range(n)], np.int32), len(number)


def aggregate_by_priority(ptr, col, val, n, theta, order):
    """-> (agg, n_agg): the definition"""
    strong = strong_lists(ptr, col, val, n, theta)
    prio = priorities(n, order)
    by_prio = sorted(range(n), key=lambda i: -prio[i])
    owner = [-1] * n
    roots1, roots3 = [], []
    for i in by_prio:  # pass 1
        if owner[i] < 0 and all(owner[j] < 0 for j in strong[i]):
            for j in [i] + strong[i]:
                owner[j] = i
            roots1.append(i)
    snapshot = list(owner)
    for i in range(n):  # pass 2: order-free
        if snapshot[i] < 0:
            for j in strong[i]:
                if snapshot[j] >= 0:
                    owner[i] = snapshot[j]
                    break
    for i in by_prio:  # pass 3
        if owner[i] < 0:
            owner[i] = i
            roots3.append(i)
            for j in strong[i]:
                if owner[j] < 0:
                    owner[j] = i
    return _number(n, owner, roots1, roots3)


def aggregate_in_rounds(ptr, col, val, n, theta, order):
    """-> (agg, n_agg, (rounds of pass 1, rounds of pass 3)): the launches of
    spmv_hip_amg_aggregate, each reading only what earlier launches wrote"""
    strong = strong_lists(ptr, col, val, n, theta)
    prio = priorities(n, order)
    own = [-1] * n
    state = [0] * n  # 0 open, 1 root, 2 non-root
    rounds1 = 0
    while True:
        rounds1 += 1
        assert rounds1 <= n + 1
        bid = [0] * n
        for i in range(n):  # bid
            if state[i] != 0:
                continue
            if own[i] >= 0 or any(own[j] >= 0 for j in strong[i]):
                state[i] = 2
                continue
            for v in [i] + strong[i]:
                bid[v] = max(bid[v], prio[i])
        left, marks = 0, []
        for i in range(n):  # take
            if state[i] != 0:
                continue
            if all(bid[v] == prio[i] for v in [i] + strong[i]):
                state[i] = 1
                marks += [(v, i) for v in [i] + strong[i]]
            else:
                left += 1
        for v, i in marks:
            own[v] = i
        if left == 0:
            break
    roots1 = [i for i in range(n) if own[i] == i]
    own2 = [-1] * n
    for i in range(n):  # pass 2
        if own[i] < 0:
            for j in strong[i]:
                if own[j] >= 0:
                    own2[i] = own[j]
                    break
    # pass 3: 0 taken, 1 free, 2 new root, 3 root, 4 member
    state = [1 if own[i] < 0 and own2[i] < 0 else 0 for i in range(n)]
    claim = [0] * n

    def push(bid):
        for k in range(n):
            if state[k] in (1, 2):
                to = bid if state[k] == 1 else claim
                for c in strong[k]:
                    if state[c] != 0:
                        to[c] = max(to[c], prio[k])
                if state[k] == 2:
                    state[k] = 3
    rounds3 = 0
    while True:
        rounds3 += 1
        assert rounds3 <= n + 1
        bid = [0] * n
        push(bid)
        left = 0
        for i in range(n):  # take
            if state[i] != 1:
                continue
            if claim[i] > prio[i]:
                state[i] = 4
            elif bid[i] < prio[i]:
                state[i] = 2
            else:
                left += 1
        if left == 0:
            break
    push([0] * n)
    roots3 = [k for k in range(n) if state[k] == 3]
    for k in roots3:  # the owners
        own2[k] = k
        for c in strong[k]:
            if state[c] == 4 and claim[c] == prio[k]:
                own2[c] = k
    owner = [own[i] if own[i] >= 0 else own2[i] for i in range(n)]
    agg, n_agg = _number(n, owner, roots1, roots3)
    return agg, n_agg, (rounds1, rounds3)


@contextlib.contextmanager
def swapped(order, how=aggregate_by_priority):
    """amg_cases.coarsen / AmgRef with the aggregates of `order`"""
    keep = ac.aggregate
    ac.aggregate = lambda ptr, col, val, n, theta: \
        how(ptr, col, val, n, theta, order)[:2]
    try:
        yield
    finally:
        ac.aggregate = keep


def coarsen(csr, n, symmetric, diagonal, theta, order, agg=None):
    """One step of the restatement -> amg_cases.coarsen's dict plus xrow_ptr /
    xrow_src (the expanded rows).  agg: the caller's aggregates instead."""
    ptr, col, src = ac.expand(csr[0], csr[1], n, symmetric)
    val = ac.values_of(src, csr[2], diagonal)
    if agg is None:
        how = aggregate_by_priority
    else:
        def how(*_):
            return np.asarray(agg, np.int32), int(np.max(agg, initial=-1)) + 1
    with swapped(order, how):
        out = ac.coarsen(ptr, col, src, val, n, theta)
    out.update(xrow_ptr=ptr, xrow_src=src)
    return out


def restate(order, *args, **kw):
    """test_gpu_amg.restate's hierarchy with the aggregates of `order`;
    args: an AmgRef constructor (e.g. test_gpu_amg.restate) and its arguments"""
    make, rest = args[0], args[1:]
    with swapped(order):
        return make(*rest, **kw)


# ---- matrices ------------------------------------------------------------------
def duplicates():
    """a row with a column twice (and the pair's mirror), unsorted rows"""
    n = 12
    rows, cols, vals = [], [], []
    for i in range(n):
        ent = [(i, 4.0)]
        if i > 0:
            ent += [(i - 1, -1.0)]
        if i + 1 < n:
            ent = [(i + 1, -1.0)] + ent
        if i == 5:
            ent += [(4, -0.5), (6, -0.25)]
        if i in (4, 6):
            ent = [(5, -0.5 if i == 4 else -0.25)] + ent
        for c, v in ent:
            rows.append(i), cols.append(c), vals.append(v)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (rp.astype(np.int32), np.array(cols, np.int32), np.array(vals))


def weak_row():
    """row 3's only off-diagonal entries are 0.0 and NaN: strong(3) is empty"""
    rp, ci, va = (a.copy() for a in tah._csr("poisson5"))
    va = va.astype(np.float64)
    off = [e for e in range(rp[3], rp[4]) if ci[e] != 3]
    for k, e in enumerate(off):
        va[e] = 0.0 if k % 2 == 0 else np.nan
    return rp, ci, va


def empty_block(n=7):
    return (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))


def matrix(name):
    if name == "duplicates":
        return duplicates()
    if name == "weak_row":
        return weak_row()
    if name == "empty7":
        return empty_block()
    return tah._csr(name)  # poissonN, bandedN, convdiffN, arrow130, ragged3001, diagN


def storages(csr, n, symmetric):
    """-> (csr of the storage, diagonal or None)"""
    if not symmetric:
        return csr, None
    return ac.lower_split(csr)
