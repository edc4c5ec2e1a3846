"""lobpcg_edges.py held to its claims on the restatement alone: the recorded
(k, status, restarts) of every entry, the classes of group a, the theorem and
orthonormality where a solve converged, X after a collapse, whether the
decisions survive another summation order, the scaling and negation relations
with the edges of their range, and mutants of the restatement that the table
must tell from it.  No GPU."""
import inspect
import types

import numpy as np
import pytest

import lobpcg_cases as lc
import lobpcg_edges as le
from lobpcg_edges import BY_ID, TABLE, decisions, same

_REF = {}


def ref(e):
    """the reference of a table entry, made once and never changed"""
    if e.id not in _REF:
        with le.Probe() as p:
            r = le.reference(e)
        r["restart_masks"] = p.restart_masks
        _REF[e.id] = r
    return _REF[e.id]


# ---- 1. the table --------------------------------------------------------------------
@pytest.mark.parametrize("e", [e for e in TABLE if e.want], ids=repr)
def test_recorded_decisions(e):
    r = ref(e)
    print(e.id, decisions(r), "active", bin(r["active"]), "restarts on",
          [bin(m) for m in r["restart_masks"]])
    assert decisions(r) == e.want
    assert bool(np.all(np.isfinite(r["X"]))) == e.finite
    assert len(r["restart_masks"]) == r["restarts"]
    if e.group in "abce":
        assert le.is_wild(e, r) == e.wild, r["theta"]


def test_classes_of_group_a():
    """every class twice or more, on different matrices; nev = 8 with all 24
    columns; a restart on a compacted index list"""
    got = {c: [] for c in le.CLASSES}
    for e in TABLE:
        if e.cls is None:
            continue
        k, status, restarts = e.want
        r = ref(e)
        assert {"recovered": status == 0 and restarts >= 1 and r["active"] == 0
                and k < e.kmax,
                "kmax": status == 0 and restarts >= 1 and k == e.kmax,
                "collapsed": status == 1 and restarts >= 1 and k > 0,
                "no_p": status == 1 and restarts == 0 and k >= 1}[e.cls], e.id
        got[e.cls].append(e.matrix)
    for c, mats in got.items():
        assert len(set(mats)) >= 2, (c, mats)
    full8 = [e.id for e in TABLE if e.cls and e.nev == 8
             and 0xff in ref(e)["restart_masks"]]
    assert full8, "no restart with m = 24"
    part = [e.id for e in TABLE if e.cls and any(
        m != (1 << e.nev) - 1 for m in ref(e)["restart_masks"])]
    assert len(part) >= 2, part


@pytest.mark.parametrize("e", [e for e in TABLE if e.group in "abc"], ids=repr)
def test_converged_pairs_and_collapsed_blocks(e):
    r = ref(e)
    M = e.mat()
    if r["status"] == 0 and r["active"] == 0:
        lc.theorem_check(M.csr, M.norm_a, M.eigvals(), r["theta"], r["X"],
                         e.largest, e.id)
        assert np.abs(r["X"].T @ r["X"] - np.eye(e.nev)).max() <= 1e-12
    if r["status"] == 1:
        assert np.all(np.isfinite(r["X"]))
        assert any(same(r["X"], B) for B in le.before_failure(e, r)), e.id


@pytest.mark.parametrize("e", [e for e in TABLE if e.group == "d"], ids=repr)
def test_poisoned_blocks(e):
    r = ref(e)
    if r["status"] == 1:
        assert any(same(r["X"], B) for B in le.before_failure(e, r)), e.id
    if e.poison and e.poison[0] == "dinv" and r["status"] == 1:
        # the prologue's rotated block: not X0, and the iterate of k = 0
        assert not same(r["X"], e.X0())
        assert same(r["X"], le.reference(e, kmax=0)["X"])
        assert np.all(r["hist"][:, 0] > 0.0) and np.all(r["hist"][:, 1:] == -1.0)
    if e.id in ("d_a_1e308", "d_a_1e200"):
        assert np.all(np.isfinite(r["theta"]))
        assert np.all(np.isinf(r["true_resnorm"]))


def test_exact_cases():
    r = ref(BY_ID["c_exact"])
    assert same(r["theta"], [1.0, 2.0, 3.0]) and same(r["hist"][:, 0], 0.0)
    assert same(r["true_resnorm"], 0.0) and same(r["X"], BY_ID["c_exact"].X0())
    r = ref(BY_ID["c_theta0"])
    assert same(r["theta"], [0.0, 1.0]) and same(r["true_resnorm"], 0.0)
    assert r["active"] == 0b01  # 0 < 0 is false: column 0 stays active
    r = ref(BY_ID["c_theta0_random"])
    assert r["active"] & 1 and abs(r["theta"][0]) < 1e-20
    r = ref(BY_ID["c_ties"])
    assert same(r["theta"], [1.0, 1.0, 2.0])
    assert same(r["X"], le.units((1, 0, 2))(9, 3))  # ties by the smaller index
    r = ref(BY_ID["b_zero1"])
    assert same(r["theta"], 0.0) and same(r["hist"][:, 0], 0.0)


# ---- 2. other summation orders ---------------------------------------------------------
@pytest.mark.parametrize("e", [e for e in TABLE if e.group in "abc"], ids=repr)
def test_decisions_under_other_summation_orders(e):
    got = le.other_orders(e)
    print(e.id, decisions(ref(e)), got)
    stable = all(d == decisions(ref(e)) for d in got.values())
    assert e.order == ("stable" if stable else "one")
    if e.id == le.TWO_RANKS:
        assert all(d[1] == 1 for d in got.values())  # collapses under each


# ---- 3. scaled and negated systems -------------------------------------------------------
@pytest.mark.parametrize("kind,id,edge,outside", le.EDGES,
                         ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_edges_of_the_working_range(kind, id, edge, outside):
    e, base = BY_ID[id], ref(BY_ID[id])
    step = 1 if edge > 0 else -1
    assert le.holds(kind, e, base, edge)
    assert not le.holds(kind, e, base, edge + step)
    point, want = outside
    r, _ = (le.a_scaled if kind == "a" else le.x_scaled)(e, point)
    assert decisions(r) == want and abs(point) > abs(edge)


@pytest.mark.parametrize("id", ["e_none", "e_dinv"])
def test_relations_inside_the_range(id):
    e, base = BY_ID[id], ref(BY_ID[id])
    for kind, points in le.INSIDE.items():
        for v in points:
            assert le.holds(kind, e, base, v), (kind, v)


@pytest.mark.parametrize("id", le.NEGATED)
def test_negated_matrix(id):
    e = BY_ID[id]
    base = ref(e)
    assert base["k"] == e.kmax and base["status"] == 0
    assert le.negation_relation(base, le.negated(e))


# ---- 4. mutants ----------------------------------------------------------------------------
# name -> (the line of lobpcg_cases.py, its replacement, the entry that tells,
# what of the result tells)
MUTANTS = {
    "the retry also keeps P": (
        "use_p = nb == 3 and has_p and attempt == 0",
        "use_p = nb == 3 and has_p", "a_diag7", "decisions"),
    "the retry is skipped when has_p": (
        "if attempt == 1 and not (nb == 3 and has_p):",
        "if attempt == 1:", "a_diag15_l", "decisions"),
    "piv >= 0": ("if not piv > 0.0:", "if not piv >= 0.0:", "c_dup", "X"),
    "ties go to the larger index": (
        "(th[b] == th[a] and b < a)", "(th[b] == th[a] and b > a)", "c_ties",
        "X"),
    "P' of an inactive column is overwritten": (
        "po[:, c] = ap if (active >> c) & 1 else blocks[-1][:, c]",
        "po[:, c] = ap", "a_diag12", "P"),
    "r <= tol": ("if r < tol:", "if r <= tol:", "c_theta0", "decisions"),
    "has_p is cleared by a restart": (
        "            has_p = 1\n",
        "            has_p = 0 if rr[\"restart\"] else 1\n", "a_tri16_8", "X"),
    "largest is ignored": (
        "before = th[b] > th[a] if largest else th[b] < th[a]",
        "before = th[b] < th[a]", "a_diag6_l", "theta"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_table_tells_a_mutant(name):
    """a one-line change of the restatement, a bug the kernels could have: the
    named entry's result differs, in the field named (P, which no solve
    returns, shows only here and in test_gpu_lobpcg_kernels.py)"""
    old, new, id, field = MUTANTS[name]
    src = inspect.getsource(lc)
    assert src.count(old) == 1, (name, src.count(old))
    mod = types.ModuleType("lobpcg_mutant")
    exec(compile(src.replace(old, new), "lobpcg_mutant", "exec"), mod.__dict__)
    e = BY_ID[id]
    M = e.mat()
    got = mod.lobpcg_ref(M.spmv, None, e.X0(), e.kmax, e.rtol, e.atol,
                         e.largest, e.dinv())
    want = ref(e)
    print(name, id, decisions(got), decisions(want))
    if field == "decisions":
        assert decisions(got) != e.want
    else:
        assert not same(got[field], want[field])
    # and the unchanged source gives the reference again
    exec(compile(src, "lobpcg_same", "exec"), mod.__dict__)
    again = mod.lobpcg_ref(M.spmv, None, e.X0(), e.kmax, e.rtol, e.atol,
                           e.largest, e.dinv())
    assert decisions(again) == e.want and same(again["X"], want["X"])


# ---- 5. non-finite values never raise ------------------------------------------------------
def test_no_path_raises_where_ieee_gives_nan_or_inf():
    inf, nan = np.inf, np.nan
    with np.errstate(all="ignore"):  # lobpcg_ref's guard
        assert same(lc.reduce_column(np.array([[inf, 1.0], [-inf, nan]])),
                    [nan, nan])
        assert same(lc.reduce_column(np.array([[inf, 1e308], [1.0, 1e308]])),
                    [inf, inf])
        assert same(lc.rows_partials(np.array([[inf], [-1.0]]), 1), [[inf]])
    hist = np.full((5, 1), -1.0)
    rn2 = np.array([0.0, inf, nan, -1.0, -0.0])
    active, done = lc.norms_ref(rn2, np.array([inf, 1.0, 1.0, nan, 0.0]),
                                0b11111, 0, 3, 1e-3, 0.0, hist)
    assert same(hist[:, 0], [0.0, inf, nan, nan, 0.0])
    assert active == 0b11110 and not done  # 0 < 1e-3 * inf alone is met
    eye = np.eye(3)
    for bad in (0.0, inf, nan, -1.0):  # 1 / sqrt of each on the diagonal of Gb
        gb = eye.copy()
        gb[1, 1] = bad
        assert not lc.rr_ref(np.stack([gb, eye]), 3, 1, 7, 0)["ok"]
    ga = eye.copy()
    ga[0, 1] = inf
    assert not lc.rr_ref(np.stack([eye, ga]), 3, 1, 7, 0)["ok"]
    ga[0, 1] = 1e308  # finite Ritz values from huge entries
    ga[1, 1] = -1e308
    out = lc.rr_ref(np.stack([eye, ga]), 3, 1, 7, 0)
    assert not out["ok"] or np.all(np.isfinite(out["theta"]))
