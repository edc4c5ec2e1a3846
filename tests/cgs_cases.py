"""Cases and references for spmv::cg_shifted (multi-shift CG: (A + sigma_s I)
x_s = b for ns shifts on the Krylov space of A).  Nothing here touches a GPU:
test_cgs_host.py holds this module to its targets, test_gpu_cgs_kernels.py and
test_gpu_cgs.py run the device on it.

  cgs_ref        the recurrence of host/cg.h restated, word for word, on `spmv`
                 and `dot` callables (every operation one float64 rounding)
  cgs_start, cgs_update_r, cgs_step, cgs_update_xp
                 one reference per kernel of blas1_cgshift.hip, named after it;
                 the scalar ones on Python floats and a state dict; data sets E
                 and R, the lengths, depth and sum_bound are blas1_cases.py's
  cgs_compose    the same solve, made of the kernel references alone
  device_dot     stream_dot's summation order followed by sum_partials': what
                 update_r + step (and the dot-partials kernel) compute

Depth of the dot product of update_r, read off the kernel: a thread adds 2 * kU
products per trip (.x then .y, element order), trips as stream_dot's; the odd
tail element last; the shuffle tree and the wave slots of spmv_block_sum; reduce,
start and step are sum_partials.  That is blas1_cases.depth(n, dot_blocks)
unchanged; a term t * t carries one rounding.

Matrices (CSR triples of int32, int32, float64): poisson11 (minres_cases), tri(N)
(2 on the diagonal, -1 beside it), diag(d).  Right-hand side of poisson11: A u
with u = uniform(-1, 1), seeded."""
import numpy as np

import blas1_cases as bc
import gmres_cases as gc
import minres_cases as mc
from blas1_cases import f

MAX_NS = 8
KMAX, RTOL = 200, 1e-10
SHIFTS1 = (0.0,)
SHIFTS4 = (0.0, 0.1, 1.0, 10.0)
SHIFTS8 = (0.5, 0.01, 3.0, 100.0, 1000.0, 0.2, 7.0, 40.0)
SHIFT_SETS = {"one": SHIFTS1, "four": SHIFTS4, "eight": SHIFTS8}

# iterations_s of cgs_ref on poisson11 with b = A uniform(-1, 1), np.dot, RTOL,
# KMAX: the restatement's own counts (test_cgs_host.py asserts them)
COUNTS = {"one": (50,),
          "four": (50, 47, 32, 14),
          "eight": (38, 50, 22, 7, 4, 44, 15, 9)}


def _sqrt(s):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(s)))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---------------------------------------------------------------------------
# the scalar kernels: a state dict with the fields of CgsScalars
# ---------------------------------------------------------------------------
def new_state(shifts, rtol, kmax):
    """the state spmv_hip_cgs_ws_reset leaves"""
    ns = len(shifts)
    pad = [0.0] * (MAX_NS - ns)
    return dict(rtol=float(rtol), pq=0.0, rrn=0.0, rr=0.0, a_old=1.0, b_old=0.0,
                bn=0.0, hist0=0.0, sigma=[float(s) for s in shifts] + pad,
                zeta=[1.0] * ns + pad, rho=[1.0] * ns + pad, cx=[0.0] * MAX_NS,
                cp=[0.0] * MAX_NS, done=0, kstop=-1, status=0, its=[0] * MAX_NS,
                k=0, kmax=int(kmax), ns=ns, n_act=ns, n_upd=0,
                act=list(range(ns)) + [0] * (MAX_NS - ns), upd=[0] * MAX_NS)


def _raise(st, kstop, status):
    st.update(done=1, kstop=kstop, status=status)


def cgs_start(st, rr, hist):
    """hist: [MAX_NS, kmax + 1], written in place"""
    if st["done"]:
        return
    st["rrn"] = st["rr"] = rr
    st["hist0"] = _sqrt(rr)
    for s in range(st["ns"]):
        hist[s, 0] = st["hist0"]
    if rr == 0.0:
        _raise(st, 0, 0)


def cgs_alpha(st):
    """a = rr / pq as update_r and step form it; None where pq is not > 0"""
    return _div(st["rr"], st["pq"]) if st["pq"] > 0.0 else None


def cgs_step(st, rrn, hist):
    """the scalar part of an iteration; st["pq"] is in place"""
    if st["done"]:
        return
    k = st["k"]
    if not st["pq"] > 0.0:
        return _raise(st, k, 1)
    if k >= st["kmax"]:
        return _raise(st, k, 0)
    st["rrn"] = rrn
    rr, a_old, b_old = st["rr"], st["a_old"], st["b_old"]
    with np.errstate(all="ignore"):
        a = _div(rr, st["pq"])
        bn = _div(rrn, rr)
        rnorm = _sqrt(rrn)
        ab = float(f(a) * f(b_old))
        na = 0
        for j in range(st["n_act"]):
            s = st["act"][j]
            rho = f(st["rho"][s])
            den = f(ab) * (f(1.0) - rho) \
                + f(a_old) * (f(1.0) + f(st["sigma"][s]) * f(a))
            rn = _div(a_old, den)
            z = float(f(st["zeta"][s]) * f(rn))
            st["cx"][s] = float(f(a) * f(rn))
            st["zeta"][s] = z
            st["rho"][s] = rn
            h = float(f(abs(z)) * f(rnorm))
            hist[s, k + 1] = h
            st["its"][s] = k + 1
            if _div(h, st["hist0"]) < st["rtol"]:
                st["upd"][j] = s
            else:
                st["cp"][s] = float(f(bn) * (f(rn) * f(rn)))
                st["upd"][j] = s | 8
                st["act"][na] = s
                na += 1
    st["n_upd"] = st["n_act"]
    st["n_act"] = na
    st.update(bn=bn, a_old=a, b_old=bn, rr=rrn, k=k + 1)
    if na == 0 or rrn == 0.0 or k + 1 == st["kmax"]:
        _raise(st, k + 1, 0)


# ---------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------
def cgs_update_r(st, q, r):
    """-> r - a * q, or None where the kernel writes nothing"""
    if st["done"] or cgs_alpha(st) is None:
        return None
    with np.errstate(all="ignore"):
        return r - f(cgs_alpha(st)) * q


def cgs_update_xp(st, k, r, p, X, PS):
    """-> (p, X, PS) after update_xp(k): new arrays; columns outside upd[] are
    the inputs' own bits"""
    p, X, PS = np.array(p), np.array(X), np.array(PS)
    if st["k"] != k:
        return p, X, PS
    go_on = not st["done"]
    with np.errstate(all="ignore"):
        for j in range(st["n_upd"]):
            w = st["upd"][j]
            s = w & 7
            ps = PS[s].copy()
            X[s] = X[s] + f(st["cx"][s]) * ps
            if go_on and w & 8:
                PS[s] = f(st["zeta"][s]) * r + f(st["cp"][s]) * ps
        if go_on:
            p = r + f(st["bn"]) * p
    return p, X, PS


# ---------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------
def cgs_ref(spmv, dot, b, shifts, kmax, rtol):
    """-> (X [ns, n], k, iterations [ns], hist [ns, kmax + 1] with -1.0 beyond
    iterations_s, status).  The recurrence of host/cg.h, word for word."""
    with np.errstate(all="ignore"):
        return _cgs_ref(spmv, dot, b, shifts, kmax, rtol)


def _cgs_ref(spmv, dot, b, shifts, kmax, rtol):
    ns, n = len(shifts), len(b)
    sig = [f(s) for s in shifts]
    r = np.array(b, np.float64)
    p = r.copy()
    rr = f(dot(r, r))
    hist = np.full((ns, kmax + 1), -1.0)
    hist[:, 0] = np.sqrt(rr)
    X = np.zeros((ns, n))
    PS = np.tile(r, (ns, 1))
    zeta = [f(1.0)] * ns
    rho = [f(1.0)] * ns
    its = [0] * ns
    active = list(range(ns))
    a_old, b_old = f(1.0), f(0.0)
    k = status = 0
    if rr == 0.0:
        return X, 0, its, hist, 0
    while k < kmax and active:
        q = spmv(p)
        pq = f(dot(p, q))
        if not pq > 0.0:
            status = 1
            break
        a = rr / pq
        rhon = {s: a_old / ((a * b_old) * (f(1.0) - rho[s])
                            + a_old * (f(1.0) + sig[s] * a)) for s in active}
        r = r - a * q
        rrn = f(dot(r, r))
        bn = rrn / rr
        k += 1
        still = []
        for s in active:
            X[s] = X[s] + (a * rhon[s]) * PS[s]
            zeta[s] = zeta[s] * rhon[s]
            rho[s] = rhon[s]
            hist[s, k] = np.abs(zeta[s]) * np.sqrt(rrn)
            its[s] = k
            if hist[s, k] / hist[s, 0] < rtol:
                continue
            PS[s] = zeta[s] * r + (bn * (rhon[s] * rhon[s])) * PS[s]
            still.append(s)
        active = still
        p = r + bn * p
        rr, a_old, b_old = rrn, a, bn
        if rrn == 0.0:
            break
    return X, max(its), its, hist, status


def cgs_compose(spmv, dot, b, shifts, kmax, rtol):
    """cgs_ref made of the kernel references: the launch sequence of
    cg_shifted() on one rank -> (X, k, iterations, hist, status)"""
    ns, n = len(shifts), len(b)
    st = new_state(shifts, rtol, kmax)
    hist = np.zeros((MAX_NS, kmax + 1))
    r = np.array(b, np.float64)
    p = r.copy()
    X = np.zeros((ns, n))
    PS = np.tile(r, (ns, 1))
    with np.errstate(all="ignore"):
        cgs_start(st, float(dot(r, r)), hist)
        k = 0
        while k < kmax and not st["done"]:
            k += 1
            q = spmv(p)
            st["pq"] = float(dot(p, q))
            rn = cgs_update_r(st, q, r)
            rrn = 0.0
            if rn is not None:
                r = rn
                rrn = float(dot(r, r))
            cgs_step(st, rrn, hist)
            p, X, PS = cgs_update_xp(st, k, r, p, X, PS)
    its = st["its"][:ns]
    out = np.full((ns, kmax + 1), -1.0)
    for s in range(ns):
        out[s, :its[s] + 1] = hist[s, :its[s] + 1]
    return X, max(its), its, out, st["status"]


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def _block_sum(v):
    v = np.array(v, np.float64).reshape(-1, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
    r = np.float64(0.0)
    for w in range(v.shape[0]):
        r = r + v[w, 0]
    return r


def sum_partials(partials):
    """sum_partials of blas1_stream.h: thread t adds partials[t], [t + 256], ...
    to 0.0, then spmv_block_sum"""
    acc = np.zeros(bc.K_BLOCK)
    for i0 in range(0, len(partials), bc.K_BLOCK):
        chunk = np.asarray(partials[i0:i0 + bc.K_BLOCK], np.float64)
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return _block_sum(acc)


def stream_partials(x, y, dot_blocks):
    """the partial array of a streaming dot product (stream_dot's shape:
    spmv_hip_dot_partial_f64, update_r)"""
    with np.errstate(all="ignore"):
        n = len(x)
        n2 = n // 2
        g = bc.stream_grid(n2, dot_blocks)
        prod = np.asarray(x, np.float64) * np.asarray(y, np.float64)
        acc = np.zeros((g, bc.K_BLOCK))
        step = bc.K_U * bc.K_BLOCK
        lane = np.arange(bc.K_BLOCK)
        for base in range(0, n2, g * step):
            for blk in range(g):
                for u in range(bc.K_U):
                    i = base + blk * step + u * bc.K_BLOCK + lane
                    ok = i < n2
                    if not ok.any():
                        continue
                    for h in (0, 1):
                        t = np.where(ok, prod[np.where(ok, 2 * i + h, 0)], 0.0)
                        acc[blk] = np.where(ok, acc[blk] + t, acc[blk])
        if n & 1:
            acc[0, 0] = acc[0, 0] + prod[n - 1]
        partials = np.zeros(dot_blocks)
        for blk in range(g):
            partials[blk] = _block_sum(acc[blk])
        return partials


def device_dot(dot_blocks):
    def dot(x, y):
        with np.errstate(all="ignore"):
            return sum_partials(stream_partials(x, y, dot_blocks))
    return dot


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def tri(N):
    i = np.arange(N)
    return gc.to_csr(N, [i, i[:-1], i[1:]], [i, i[1:], i[:-1]],
                     [np.full(N, 2.0), np.full(N - 1, -1.0), np.full(N - 1, -1.0)])


def diag(d):
    d = np.asarray(d, np.float64)
    i = np.arange(len(d))
    return gc.to_csr(len(d), [i], [i], [d])


def shifted(csr, sigma):
    """A + sigma I"""
    rp, ci, va = csr
    va = va.copy()
    va[ci == gc.row_of(rp)] += sigma
    return rp, ci, va


def dense(csr):
    rp, ci, va = csr
    N = len(rp) - 1
    A = np.zeros((N, N))
    np.add.at(A, (gc.row_of(rp), ci), va)
    return A


def poisson11():
    return mc.csr_by_name("poisson11")


def poisson11_rhs(spmv=None):
    csr = poisson11()
    spmv = spmv or (lambda q: gc.csr_spmv(csr, q))
    N = len(csr[0]) - 1
    return spmv(np.random.default_rng(N + 7).uniform(-1, 1, N))


# ---------------------------------------------------------------------------
# the exits
# ---------------------------------------------------------------------------
def exit_case(name):
    """-> (csr, b, shifts, kmax, rtol, k_want, status_want)"""
    if name == "zero":  # b = 0: every shift stops at k = 0
        return tri(40), np.zeros(40), SHIFTS4, 20, RTOL, 0, 0
    if name == "indefinite":  # poisson11 - 3 I: p.q < 0 after a few steps
        return shifted(poisson11(), -3.0), poisson11_rhs(), (0.0, 1.0, 10.0), \
            40, RTOL, None, 1
    if name == "negative":  # -A: status 1 at k = 0
        rp, ci, va = tri(40)
        b = np.random.default_rng(41).uniform(-1, 1, 40)
        return (rp, ci, -va), b, (0.0, 1.0), 40, RTOL, 0, 1
    if name == "underflow":  # rtol = 0: zeta of the large shifts underflows
        return poisson11(), poisson11_rhs(), (0.0, 1e3, 1e6), 400, 0.0, 400, 0
    if name == "identity":  # one step solves every shift exactly: rrn == 0
        b = np.arange(1.0, 9.0)
        return diag(np.ones(8)), b, (0.0, 1.0, 3.0), 10, RTOL, 1, 0
    if name == "nan":  # a NaN in b: p.q is NaN at once
        b = np.random.default_rng(43).uniform(-1, 1, 40)
        b[17] = np.nan
        return tri(40), b, SHIFTS4, 12, RTOL, 0, 1
    raise KeyError(name)


EXITS = ("zero", "indefinite", "negative", "underflow", "identity", "nan")
