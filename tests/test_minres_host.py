"""spmv::minres without a GPU: minres_cases.py is held to the CPU prototype's
table, the per-kernel references are shown to compose into minres_ref bit for
bit, every exit is reached on a hand-built case, and the argument rules are
checked through the host library."""
import math

import numpy as np
import pytest

import minres_cases as mc
import oracle
from spmv_amd import host


def _spmv(csr):
    return lambda q: oracle.csr_spmv(*csr, q)


def _dense_spmv(A):
    A = np.asarray(A, np.float64)

    def mult(q):  # row sums left to right, the product rounded first
        out = np.zeros(len(q))
        for i in range(len(q)):
            s = 0.0
            for j in range(len(q)):
                s += float(A[i, j] * q[j])
            out[i] = s
        return out
    return mult


_CACHE = {}


def _case(name, kind, pre):
    key = (name, kind, pre)
    if key not in _CACHE:
        csr = mc.csr_by_name(name)
        sp = _spmv(csr)
        b = mc.rhs(csr, kind, sp)
        d = mc.dinv_by_name(name)
        minv = None if pre == "none" else (lambda q: d * q)
        first = mc.minres_ref(sp, np.dot, minv, b, mc.KMAX, mc.RTOL)
        second = mc.minres_ref(sp, mc.dot_chunks64, minv, b, mc.KMAX, mc.RTOL)
        _CACHE[key] = (sp, b, first, second)
    return _CACHE[key]


@pytest.mark.parametrize("case", sorted(mc.TABLE))
def test_the_restatement_reproduces_the_prototype(case):
    sp, b, (x, k, hist, status), second = _case(*case)
    res = np.linalg.norm(b - sp(x)) / np.linalg.norm(b)
    xdev = np.linalg.norm(second[0] - x) / np.linalg.norm(x)
    print(case, "k", k, second[1], "x of the two orders", xdev, "residual", res)
    assert k == second[1] == mc.TABLE[case]
    assert status == second[3] == 0
    assert len(hist) == k + 1 and np.all(np.diff(hist) <= 0.0)
    assert hist[k] / hist[0] < mc.RTOL <= hist[k - 1] / hist[0]
    assert res < 10 * mc.RTOL
    assert xdev <= 1e-9


def test_sas_needs_its_preconditioner_and_k_is_not_determined():
    """the table's last row: Jacobi converges in 96..99 steps, the count moves
    between the summation orders; without it 600 steps do not suffice"""
    ks = []
    for kind in ("ones", "rand"):
        sp, b, first, second = _case("sas", kind, "dinv")
        assert first[3] == second[3] == 0
        ks += [first[1], second[1]]
        for x in (first[0], second[0]):
            assert np.linalg.norm(b - sp(x)) / np.linalg.norm(b) < 10 * mc.RTOL
    assert ks == [99, 96, 99, 99]
    sp, b, first, _ = _case("sas", "ones", "none")
    assert first[1] == mc.KMAX and not first[2][-1] / first[2][0] < mc.RTOL


@pytest.mark.parametrize("kind", ["ones", "rand"])
def test_minres_never_exceeds_cg_on_a_definite_matrix(kind):
    """M = I on poisson11: MINRES minimises ||r_k|| over the Krylov space CG
    picks its iterate from, so hist[k] <= ||r_k|| of CG, up to what the
    summation order moves either history by"""
    sp, b, (_, k, hist, _), second = _case("poisson11", kind, "none")
    cg = mc.cg_norms(sp, b, k)
    dev = np.abs(second[2][:k + 1] - hist).max() / hist[0]
    slack = max(dev, 2.0 ** -50) * hist[0]
    print(kind, "two-order deviation", dev, "largest hist - cg",
          (hist - cg).max())
    assert hist[0] == cg[0]
    assert np.all(hist <= cg + slack)


def _by_kernels(sp, b, dinv, kmax, rtol, dot=np.dot):
    """the solve as the device runs it: init, start, update_xwv(0), then
    update_r, step, update_xwv per iteration, all from the kernel references"""
    r2 = np.array(b, np.float64)
    r1 = np.zeros(len(b))
    y = mc.minres_init(r2, dinv)
    st = mc.minres_start(dot(r2, y))
    x, w1, w2 = (np.zeros(len(b)) for _ in range(3))
    if st["done"]:
        return x, 0, np.array([st["hist0"] or 0.0]), st["status"]
    hist, k = [st["hist0"]], 0
    v = mc.minres_scale(y, st["inv_beta"])
    bob = 0.0
    while k < kmax:
        Av = sp(v)
        alfa = dot(v, Av)
        t, y = mc.minres_update_r(Av, r1, r2, dinv, alfa, st["beta"], bob, k == 0)
        r1, r2 = r2, t
        out = mc.minres_step(st, alfa, dot(r2, y), hist[0], k, kmax, rtol)
        if out["k"] == k:  # stopped without a new iterate
            return x, k, np.array(hist), out["status"]
        k = out["k"]
        hist.append(out["res"])
        w, x, v = mc.minres_update_xwv(
            v, w1, w2, x, y, out["oldeps"], out["delta"], out["inv_gamma"],
            out["phi"], out.get("inv_beta", 0.0), go_on=not out["done"])
        w1, w2 = w2, w
        if out["done"]:
            return x, k, np.array(hist), out["status"]
        st = {key: out[key] for key in mc.STATE}
        bob = out["bob"]
    return x, k, np.array(hist), 0


@pytest.mark.parametrize("name,pre", [("shift11", "none"), ("saddle500", "dinv")])
def test_the_kernel_references_compose_into_the_recurrence(name, pre):
    sp, b, first, _ = _case(name, "rand", pre)
    dinv = None if pre == "none" else mc.dinv_by_name(name)
    for kmax, rtol in ((mc.KMAX, mc.RTOL), (7, 0.0)):
        minv = None if dinv is None else (lambda q: dinv * q)
        ref = first if kmax == mc.KMAX else mc.minres_ref(sp, np.dot, minv, b,
                                                          kmax, rtol)
        x, k, hist, status = _by_kernels(sp, b, dinv, kmax, rtol)
        assert (k, status) == (ref[1], ref[3])
        assert np.array_equal(hist, ref[2]) and np.array_equal(x, ref[0])


# ---- the exits, on hand-built cases ------------------------------------------
EXITS = {
    # two distinct eigenvalues: the Lanczos process ends after 2 steps
    "lanczos": (np.diag([2.0, 2.0, 5.0, 5.0]), [1.0, 1.0, 1.0, 1.0], None, 2, 1),
    # r.M^-1 r < 0 at once
    "negative": (np.diag([2.0, 3.0]), [1.0, 1.0], [1.0, -2.0], 0, 2),
    # A b = 0: alfa = 0 and beta = 0 on the first step, so gamma = 0
    "singular": (np.array([[1.0, -1.0], [-1.0, 1.0]]), [1.0, 1.0], None, 0, 3),
    # diag(1, -1) with b = (1, 1): alfa = 0 and beta = 1 on the first step.
    # gbar = -cs * alfa = 0, but gamma = sqrt(gbar^2 + beta^2) = 1: NOT a
    # singular direction -- the second step solves the system (x = (1, -1))
    "zero_alfa": (np.diag([1.0, -1.0]), [1.0, 1.0], None, 2, 0),
}


def exit_case(name):
    A, b, dinv, k, status = EXITS[name]
    dinv = None if dinv is None else np.array(dinv)
    minv = None if dinv is None else (lambda q: dinv * q)
    ref = mc.minres_ref(_dense_spmv(A), mc.dot_plain, minv, np.array(b), 50,
                        1e-12)
    return A, np.array(b), dinv, ref, k, status


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_exit_is_reached(name):
    A, b, dinv, (x, k, hist, status), k_want, status_want = exit_case(name)
    print(name, "k", k, "status", status, "x", x, "hist", hist)
    assert status == status_want
    assert k_want is None or k == k_want
    assert np.all(np.isfinite(x)) and len(hist) == k + 1
    if name == "lanczos":
        assert np.allclose(A @ x, b, rtol=0, atol=1e-14)
    if name == "singular":
        assert np.all(x == 0.0) and np.all(A @ b == 0.0)
    if name == "zero_alfa":
        # confirmed in the restatement: v = b / sqrt(2), alfa = v.Av = 0, r2 =
        # Av, beta = 1; gamma = 1, and x = (1, -1) after the second step
        v = b * (1.0 / math.sqrt(2.0))
        Av = A @ v
        assert mc.dot_plain(v, Av) == 0.0
        assert abs(math.sqrt(mc.dot_plain(Av, Av)) - 1.0) <= 2.0 ** -52
        # the first step cannot reduce the residual
        assert abs(hist[1] - hist[0]) <= 2.0 ** -51
        assert np.allclose(x, [1.0, -1.0], rtol=0, atol=1e-15)


def test_a_zero_right_hand_side_returns_at_once():
    x, k, hist, status = mc.minres_ref(_dense_spmv(np.eye(3)), np.dot, None,
                                       np.zeros(3), 10, 1e-10)
    assert (k, status) == (0, 0) and np.all(x == 0.0) and list(hist) == [0.0]


# ---- the argument rules, through the host library ----------------------------
def test_check_rules_error_strings():
    buf = np.zeros(64)
    p = buf.ctypes.data
    ok = dict(kmax=5, rows=8, b_ptr=p, x_ptr=p + 8 * 8)
    host.minres_check_rules(**ok)
    host.minres_check_rules(**ok, has_dinv=True, dinv_ptr=p + 16 * 8)
    host.minres_check_rules(**ok, has_sgs=True, sgs_rows=8)
    host.minres_check_rules(**ok, has_amg=True, amg_rows=8)
    host.minres_check_rules(kmax=0, rows=0)  # empty ranges never overlap
    bad = [
        (dict(ok, kmax=-1), "kmax"),
        (dict(ok, has_dinv=True, has_sgs=True, sgs_rows=8, dinv_ptr=p + 128),
         "one preconditioner"),
        (dict(ok, has_sgs=True, has_amg=True, sgs_rows=8, amg_rows=8),
         "one preconditioner"),
        (dict(ok, has_sgs=True, sgs_rows=7), "7 rows, the matrix has 8"),
        (dict(ok, has_amg=True, amg_rows=9), "9 rows, the matrix has 8"),
        (dict(ok, has_sgs=True, sgs_rows=8, sgs_negative_pivots=3),
         "3 negative pivot"),
        (dict(ok, x_ptr=p + 7 * 8), "x overlaps b"),
        (dict(ok, has_dinv=True, dinv_ptr=p + 15 * 8), "x overlaps dinv"),
    ]
    for kw, text in bad:
        with pytest.raises(host.SpmvHostError, match=text):
            host.minres_check_rules(**kw)
    # the order: kmax before the preconditioner before the rows
    with pytest.raises(host.SpmvHostError, match="kmax"):
        host.minres_check_rules(kmax=-1, has_dinv=True, has_sgs=True)
    with pytest.raises(host.SpmvHostError, match="one preconditioner"):
        host.minres_check_rules(kmax=1, has_amg=True, has_sgs=True, sgs_rows=3,
                                rows=8)


def test_the_python_surface():
    assert callable(host.minres) and issubclass(host.MinresWorkspace, object)
