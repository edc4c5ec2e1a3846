"""CPU checks of the multicolour symmetric Gauss-Seidel preconditioner
(spmv::SgsPreconditioner, sgs_apply, pcg_sgs): the new symbols are declared in
both headers, exported and prototyped with the declared number of arguments,
the change is additive (ABI 5), NULL handles are refused before anything touches
a device, and the two pure-host entries -- the colouring and the builder of the
colour-major copy -- equal their restatements.

Matrices: test_gpu_pcg's shapes (its generators are imported, not copied), their
lower triangles in the symmetric input form, and the small cases a colouring or
a split can get wrong."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_pcg as tp
from spmv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NEW = ("spmv_hip_mcgs_plan_create", "spmv_hip_mcgs_plan_destroy",
           "spmv_hip_mcgs_plan_bytes", "spmv_hip_mcgs_apply_f64",
           "spmv_hip_sgs_init_f64", "spmv_hip_sgs_update_r_f64",
           "spmv_hip_sgs_dot_rz_f64")
HOST_NEW = ("spmvh_sgs_color", "spmvh_sgs_build_create", "spmvh_sgs_build_get",
            "spmvh_sgs_build_destroy", "spmvh_sgs_create", "spmvh_sgs_destroy",
            "spmvh_sgs_info", "spmvh_sgs_colors", "spmvh_sgs_apply",
            "spmvh_sgs_workspace_create", "spmvh_sgs_workspace_destroy",
            "spmvh_sgs_workspace_reserve_timing", "spmvh_pcg_sgs")
EINVAL = -1


# ---- 1. the interface -------------------------------------------------------------
def _declared_arity(header):
    """function name -> number of parameters of its declaration"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_sgs_symbols_declared_exported_prototyped():
    hip_decl = _declared_arity("spmv_hip.h")
    host_decl = _declared_arity("spmv_host_c.h")
    for n in HIP_NEW:
        assert n in hip_decl and hasattr(_lib.hip, n) and n in _lib.HIP_SYMBOLS, n
        assert len(getattr(_lib.hip, n).argtypes) == hip_decl[n], n
    for n in HOST_NEW:
        assert n in host_decl and hasattr(host.lib, n) and n in host.HOST_SYMBOLS, n
        assert len(getattr(host.lib, n).argtypes) == host_decl[n], n


def test_abi_version_is_still_5():
    assert _lib.hip.spmv_hip_abi_version() == 5
    txt = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"#define\s+SPMV_HIP_ABI_VERSION\s+5\b", txt)


def test_rules_are_stated_and_the_kernels_are_built():
    cg_h = open(os.path.join(ROOT, "spmv_amd", "csrc", "host", "cg.h")).read()
    for name in ("class SgsPreconditioner", "void sgs_apply(", "int pcg_sgs(",
                 "class SgsWorkspace", "int num_colors() const",
                 "void colors(int32_t* out) const", "int64_t plan_bytes() const"):
        assert name in cg_h, name
    part = cg_h[cg_h.index("CG with the preconditioner M from x0 = 0"):
                cg_h.index("int pcg_sgs(")]
    assert "poll_every and time_spmv apply" in part
    assert "consumer_reductions, defer_x and mixed are IGNORED" in part
    mk = open(os.path.join(ROOT, "spmv_amd", "csrc", "Makefile")).read()
    assert "hip/spmv_mcgs.hip" in mk
    assert os.path.exists(os.path.join(ROOT, "spmv_amd", "csrc", "hip",
                                       "spmv_mcgs.hip"))


def test_null_handles_refused_without_a_device():
    h = _lib.hip
    plan = C.c_void_p()
    nbytes = C.c_int64()
    assert h.spmv_hip_mcgs_plan_create(None, None, C.byref(plan)) == EINVAL
    assert h.spmv_hip_mcgs_plan_destroy(None) == 0
    assert h.spmv_hip_mcgs_plan_bytes(None, C.byref(nbytes)) == EINVAL
    assert h.spmv_hip_mcgs_apply_f64(None, None, None, None, None, None) == EINVAL
    assert h.spmv_hip_sgs_init_f64(None, None, 4, None, None, None, None) == EINVAL
    assert h.spmv_hip_sgs_update_r_f64(None, None, 1, 4, None, None,
                                       None) == EINVAL
    assert h.spmv_hip_sgs_dot_rz_f64(None, None, 4, None, None, None) == EINVAL
    # a context but no plan / no input / no workspace: refused before the
    # context is looked at -- the block of memory standing in for it is never read
    ctx = C.create_string_buffer(4096)
    v = C.addressof(ctx) + 1024
    v -= v % 16
    assert h.spmv_hip_mcgs_plan_create(ctx, None, C.byref(plan)) == EINVAL
    assert h.spmv_hip_mcgs_plan_create(ctx, v, None) == EINVAL
    assert h.spmv_hip_mcgs_apply_f64(ctx, None, None, v, v, None) == EINVAL
    assert h.spmv_hip_sgs_init_f64(ctx, None, 4, v, v, v, None) == EINVAL
    assert h.spmv_hip_sgs_update_r_f64(ctx, None, 1, 4, v, v, None) == EINVAL
    assert h.spmv_hip_sgs_dot_rz_f64(ctx, None, 4, v, v, None) == EINVAL


def test_host_facade_refuses_null_handles():
    lib = host.lib
    k = C.c_int()
    assert lib.spmvh_pcg_sgs(None, None, None, None, None, None, 10, 1e-8,
                             C.byref(k), None, None, 0, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_create(None, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_apply(None, None, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_info(None, None, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_colors(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_workspace_create(None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_workspace_reserve_timing(None, 4) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_build_create(None, None, None, 0, 0, 0, None, None) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_build_get(None, *([None] * 10)) != 0
    assert b"NULL" in lib.spmvh_last_error()
    assert lib.spmvh_sgs_destroy(None) == 0
    assert lib.spmvh_sgs_workspace_destroy(None) == 0
    assert lib.spmvh_sgs_build_destroy(None) == 0


def test_python_layer_has_the_entry_points():
    for name in ("SgsPreconditioner", "sgs_apply", "pcg_sgs", "SgsWorkspace",
                 "sgs_color", "sgs_build"):
        assert callable(getattr(host, name)), name
    for name in ("num_colors", "colors", "plan_bytes", "close"):
        assert callable(getattr(host.SgsPreconditioner, name)), name
    assert callable(host.SgsWorkspace.reserve_timing)


# ---- 2. the colouring ---------------------------------------------------------------
def _is_entry(i, c, n, symmetric):
    """an off-diagonal entry of the local diagonal block, as stored"""
    return c < n and c != i and (not symmetric or c < i)


def greedy_ref(rp, ci, n, symmetric):
    """greedy in natural order over the pattern of B + B^T"""
    nb = [set() for _ in range(n)]
    for i in range(n):
        for c in ci[rp[i]:rp[i + 1]].tolist():
            if _is_entry(i, c, n, symmetric):
                nb[i].add(c)
                nb[c].add(i)
    colour = np.full(n, -1, np.int32)
    for i in range(n):
        worn = {colour[j] for j in nb[i] if j < i}
        c = 0
        while c in worn:
            c += 1
        colour[i] = c
    return colour, nb


def _lower(csr):
    """the lower triangle with the diagonal: the symmetric input form"""
    rp, ci, va = csr
    keep = ci <= tp._row_of(rp)
    rows = tp._row_of(rp)[keep]
    n = len(rp) - 1
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return rp2.astype(np.int32), ci[keep], va[keep]


def _from_rows(rows):
    """[[(col, val), ...], ...] -> CSR"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float64)
    return rp, ci, va


def _small_cases():
    diag = _from_rows([[(i, 2.0 + i)] for i in range(70)])
    one = _from_rows([[(0, 3.0)]])
    # row 2 has no off-diagonal entry (and no mirror either)
    lonely = _from_rows([[(0, 4.0), (1, -1.0)], [(0, -1.0), (1, 4.0), (3, -1.0)],
                         [(2, 4.0)], [(1, -1.0), (3, 4.0)]])
    # (0, 2) is present and (2, 0) is not; (1, 3) and (3, 1) likewise: a
    # colouring over the rows' own entries alone lets 0 and 2 share a colour
    oneway = _from_rows([[(0, 4.0), (2, -1.0)], [(1, 4.0), (3, -0.5)],
                         [(2, 4.0)], [(3, 4.0)], [(4, 4.0), (0, -1.0)]])
    return {"diagonal": diag, "n1": one, "lonely_row": lonely,
            "one_way": oneway}


CASES = {}
for _name in tp.SHAPES:
    CASES[_name] = (tp._csr(_name), False)
    CASES[_name + "_lower"] = (_lower(tp._csr(_name)), True)
    CASES[_name + "_full_as_symmetric"] = (tp._csr(_name), True)
for _name, _csr in _small_cases().items():
    CASES[_name] = (_csr, False)
CASES["lonely_row_lower"] = (_lower(_small_cases()["lonely_row"]), True)
CASES["diagonal_symmetric"] = (_small_cases()["diagonal"], True)


@pytest.fixture(scope="module")
def refs():
    return {name: greedy_ref(csr[0], csr[1], len(csr[0]) - 1, sym)
            for name, (csr, sym) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_colouring_equals_the_greedy_restatement(refs, name):
    (rp, ci, _), sym = CASES[name]
    n = len(rp) - 1
    want, nb = refs[name]
    got, nc = host.sgs_color(rp, ci, n, n, sym)
    assert np.array_equal(got, want), name
    # proper, and every colour 0 .. C-1 is worn
    assert nc == int(want.max()) + 1
    assert np.array_equal(np.unique(got), np.arange(nc)), name
    for i in range(n):
        assert all(got[j] != got[i] for j in nb[i]), (name, i)


def test_small_cases_have_the_colours_one_expects(refs):
    assert host.sgs_color(*CASES["diagonal"][0][:2], 70)[1] == 1
    got, nc = host.sgs_color(*CASES["n1"][0][:2], 1)
    assert nc == 1 and got.tolist() == [0]
    got, nc = host.sgs_color(*CASES["one_way"][0][:2], 5)
    assert got[0] != got[2] and got[1] != got[3] and got[0] != got[4]
    # ... which the rows' own entries alone would not give: rows 2 and 3 store
    # no off-diagonal entry
    assert nc == 2 and got[2] == 1 and got[3] == 1
    got, nc = host.sgs_color(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)
    assert nc == 0 and len(got) == 0


@pytest.mark.parametrize("symmetric", [False, True])
def test_poisson_gets_the_parity_colouring(symmetric):
    n = 11
    rp, ci, _ = tp._csr("poisson11") if not symmetric \
        else _lower(tp._csr("poisson11"))
    got, nc = host.sgs_color(rp, ci, n ** 3, n ** 3, symmetric)
    i = np.arange(n ** 3)
    parity = (i % n + (i // n) % n + i // (n * n)) % 2
    assert nc == 2 and np.array_equal(got, parity)


def test_ghost_columns_are_ignored_and_sizes_checked():
    # the rows of a rank that owns 3 columns; columns 3, 4 are ghosts
    rp, ci, va = _from_rows([[(0, 4.0), (1, -1.0), (3, -1.0)],
                             [(0, -1.0), (1, 4.0), (4, -1.0)],
                             [(2, 4.0), (4, -1.0), (3, -1.0)]])
    got, nc = host.sgs_color(rp, ci, 3, 3, False)
    assert nc == 2 and got.tolist() == [0, 1, 0]
    b = host.sgs_build(rp, ci, va, 3, 3, False)
    assert b["before"][1].tolist() == [0] and b["after"][1].tolist() == [1]
    with pytest.raises(host.SpmvHostError, match="same index range"):
        host.sgs_color(rp, ci, 3, 5, False)
    with pytest.raises(host.SpmvHostError, match="same index range"):
        host.sgs_build(rp, ci, va, 3, 2, False)


# ---- 3. the builder -------------------------------------------------------------------
def _row_entries_ref(csr, n, symmetric):
    """row -> its off-diagonal local entries [(col, val)], ascending by column,
    duplicates in storage order (symmetric: the stored lower entries and the
    entries of the row's column in the stored block, a stable transpose)"""
    rp, ci, va = csr
    rows = [[] for _ in range(n)]
    mirror = [[] for _ in range(n)]
    for i in range(n):
        for e in range(rp[i], rp[i + 1]):
            c = int(ci[e])
            if _is_entry(i, c, n, symmetric):
                rows[i].append((c, va[e]))
                if symmetric:
                    mirror[c].append((i, va[e]))
    out = []
    for i in range(n):
        both = rows[i] + mirror[i]
        order = np.argsort([c for c, _ in both], kind="stable")
        out.append([both[j] for j in order])
    return out


def _check_build(name, csr, symmetric, colours_want):
    rp, ci, va = csr
    n = len(rp) - 1
    b = host.sgs_build(rp, ci, va, n, n, symmetric)
    colours, perm, start = b["colors"], b["perm"], b["color_start"]
    assert np.array_equal(colours, colours_want), name
    nc = b["num_colors"]
    # a permutation, colour-major, ascending within a colour
    assert np.array_equal(np.sort(perm), np.arange(n)), name
    assert start[0] == 0 and start[nc] == n, name
    for c in range(nc):
        seg = perm[start[c]:start[c + 1]]
        assert len(seg) > 0 and np.all(colours[seg] == c), (name, c)
        assert np.all(np.diff(seg) > 0), (name, c)
    # the diagonal: the sum of the entries (i, i) in storage order
    d = np.zeros(n)
    rows = tp._row_of(rp)
    for e in np.flatnonzero(ci == rows):
        d[rows[e]] += va[e]
    assert np.array_equal(b["d"], d), name
    # before + after of a row are exactly its entries, split by the colour of
    # the column, each part in the order of the reference
    want = _row_entries_ref(csr, n, symmetric)
    for pos in range(n):
        i = perm[pos]
        for part, keep in (("before", lambda c: colours[c] < colours[i]),
                           ("after", lambda c: colours[c] > colours[i])):
            ptr, col, val = b[part]
            got = list(zip(col[ptr[pos]:ptr[pos + 1]].tolist(),
                           val[ptr[pos]:ptr[pos + 1]].tolist()))
            ref = [(c, float(v)) for c, v in want[i] if keep(c)]
            assert got == ref, (name, part, i)
        assert all(colours[c] != colours[i] for c, _ in want[i]), (name, i)
    return b


@pytest.mark.parametrize("name", list(CASES))
def test_builder_output(refs, name):
    csr, sym = CASES[name]
    csr = tp._scaled(csr) if len(csr[0]) > 100 else csr
    _check_build(name, csr, sym, refs[name][0])


def test_duplicates_keep_their_storage_order():
    # row 1 stores column 0 twice and column 2 twice, out of column order;
    # row 3 stores its diagonal twice
    rows = [[(0, 4.0), (1, -1.0)],
            [(2, -0.25), (0, -1.0), (1, 4.0), (2, -0.5), (0, -2.0)],
            [(1, -0.75), (2, 4.0)],
            [(3, 1.5), (3, 2.5), (2, -1.0)]]
    csr = _from_rows(rows)
    want, _ = greedy_ref(csr[0], csr[1], 4, False)
    b = _check_build("duplicates", csr, False, want)
    pos = int(np.flatnonzero(b["perm"] == 1)[0])
    ptr, col, val = b["before"]
    # colours 0, 1, 0, 1: both neighbours of row 1 come before it
    assert col[ptr[pos]:ptr[pos + 1]].tolist() == [0, 0, 2, 2]
    assert val[ptr[pos]:ptr[pos + 1]].tolist() == [-1.0, -2.0, -0.25, -0.5]
    ptr, col, val = b["after"]
    assert ptr[pos] == ptr[pos + 1]
    assert b["d"][3] == 4.0
    # the symmetric input form of a lower triangle with duplicates
    rows = [[(0, 4.0)], [(0, -1.0), (1, 4.0), (0, -2.0)],
            [(1, -0.5), (0, -0.25), (2, 4.0), (1, -0.75)]]
    csr = _from_rows(rows)
    want, _ = greedy_ref(csr[0], csr[1], 3, True)
    b = _check_build("duplicates_lower", csr, True, want)
    # row 0 = column 0 of the stored block: (1, -1), (1, -2), (2, -0.25)
    pos = int(np.flatnonzero(b["perm"] == 0)[0])
    ptr, col, val = b["after"]
    assert col[ptr[pos]:ptr[pos + 1]].tolist() == [1, 1, 2]
    assert val[ptr[pos]:ptr[pos + 1]].tolist() == [-1.0, -2.0, -0.25]


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_both_storages_of_a_symmetric_matrix_give_identical_arrays(shape):
    csr = tp._scaled(tp._csr(shape))  # S A S: exactly symmetric
    n = len(csr[0]) - 1
    general = host.sgs_build(*csr, n, n, False)
    for form in (_lower(csr), csr):
        sym = host.sgs_build(*form, n, n, True)
        assert sym["num_colors"] == general["num_colors"]
        for key in ("colors", "perm", "color_start", "d"):
            assert np.array_equal(sym[key], general[key]), (shape, key)
        for part in ("before", "after"):
            for a, b in zip(sym[part], general[part]):
                assert np.array_equal(a, b), (shape, part)
