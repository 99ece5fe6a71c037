"""Subassignment x[i, j, ...] <- value without a GPU: the numpy expectation of tests/subassign_cases.py against a
per-leaf statement of the rule; Session.subassign over a recording dispatcher -- one call per case, every check and
message of .subassign_SVT_by_Nindex (R/SparseArray-subassignment.R:114-170) in its order, the no-op paths without a
call; what the library answers without a device (the tile, the workspace sizes, the refusals decided on the host); and
the ``__host__`` side of the element rule (svt_rule_assign, sparsearray_amd/csrc/svt_arith_rules.h) through
tests/assign_rules_main.cpp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import subassign_cases as sa
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.api import Session
from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP
from subset_cases import SPECIALS_F64, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR, SVT = "C_subassign_SVT_with_short_Rvector", "C_subassign_SVT_with_SVT"
NA = int(NA_integer)


class Recorder:
    """offers every entry point, records the calls and answers the two subassignments by the per-leaf restatement"""

    def __init__(self):
        self.calls = []

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        assert name in (VECTOR, SVT)
        x, index, value = args
        if name == SVT:
            return sa.restate(x, index, value, value.type)
        v_type = "logical" if value.dtype == np.bool_ else "double" if value.dtype == np.float64 else "integer"
        return sa.restate(x, index, value.astype(np.int32) if v_type == "logical" else value, v_type)


@pytest.fixture()
def rec():
    r = Recorder()
    return Session(r), r


def _value_for_session(value, v_type):
    """the Python value a caller would write for a vector of R type ``v_type``: a logical vector without NA is bool"""
    if v_type == "logical" and not (np.asarray(value) == NA_integer).any():
        return np.asarray(value) != 0
    return value


# ---------------------------------------------------------------------------
# the expectation itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sa.NAMES)
def test_numpy_expectation_agrees_with_the_per_leaf_restatement(name):
    x, index, value, v_type = sa.case(name)[:4]
    sa.check(sa.restate(x, index, value, v_type), name)


def test_the_cases_reach_what_they_are_named_for():
    def merged(name):
        x, index, value, v_type, _, _, want_stored = sa.case(name)
        sub = sa.index0(x.dim, index)
        covered = len(set(sub[1].tolist())) if x.ndim == 2 else None
        last = {}
        for p, r in enumerate(sub[0]):
            last[int(r)] = value[p % len(value)]
        return x.nzcount() + covered * sum(1 for v in last.values() if v != 0 or v != v)
    assert [merged(f"merged_length_{s}") for s in ("T_minus_1", "T", "T_plus_1")] == [sa.T - 1, sa.T, sa.T + 1]
    assert 2 * sa.T < merged("covered_column_of_5000_rows") <= 3 * sa.T
    assert merged("patch_leaf_over_400_leaves") - sa.case("patch_leaf_over_400_leaves")[0].nzcount() == 400 * 30 > 2 * sa.P
    assert merged("filter_value_zero") == sa.case("filter_value_zero")[0].nzcount() > sa.T
    # the pair on the tile edge: x's entry of row 1024 is merged place T - 1, the y entry of that row place T
    x, index, value = sa.case("pair_split_across_a_tile_edge")[:3]
    merged_places = sorted([(int(r), "x") for r in x.leaves[0][0]] + [(int(r), "y") for r in np.flatnonzero(value)])
    assert merged_places.index((1024, "x")) == sa.T - 1 and merged_places.index((1024, "y")) == sa.T
    # stored zeros of x inside and outside the selected leaves, and values that are 0, -0.0, NA and a payload NaN
    x = sa.case("stored_zeros_of_x_inside_and_outside")[0]
    assert all((x.leaves[c][1] == 0).any() for c in (1, 2, 12, 20))
    v = sa.case("values_zero_minus_zero_NA_NaN")[2]
    assert {0x0, 0x8000000000000000, 0x7FF00000000007A2, 0x7FF8000000000001} <= set(bits(v).tolist())
    assert any((lf is not None and (lf[1] == 0).any()) for lf in sa.case("svt_v_with_stored_zeros")[2].leaves)
    assert {(sa.case(n)[0].type, sa.case(n)[3]) for n in sa.NAMES if n.startswith("types_") and "_vector_" in n} == \
           {(a, b) for a in sa.TYPE_ORDER for b in sa.TYPE_ORDER}
    assert sa.case("three_d")[0].ndim == 3 and sa.case("four_d")[0].ndim == 4 and sa.case("svt_three_d")[0].ndim == 3


def test_leaf_list_is_outermost_slowest():
    assert sa.leaf_list((7, 3, 4), [None, None, None]) is None
    assert sa.leaf_list((7, 3, 4), [None, [3, 1], [2, 4]]).tolist() == [2 + 3 * 1, 0 + 3 * 1, 2 + 3 * 3, 0 + 3 * 3]
    assert sa.leaf_list((7, 3, 4), [[1], None, [4]]).tolist() == [9, 10, 11]
    assert sa.leaf_list((7, 3), [None, []]).tolist() == []


# ---------------------------------------------------------------------------
# Session.subassign
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sa.NAMES)
def test_session_passes_the_case_through_one_call(rec, name):
    s, r = rec
    x, index, value, v_type, new_type = sa.case(name)[:5]
    is_svt = isinstance(value, SVT_SparseArray)
    res = s.subassign(x, value if is_svt else _value_for_session(value, v_type), *index)
    sa.check(res, name, "Session.subassign: ")
    if any(sub is not None and len(sub) == 0 for sub in index):
        assert r.calls == []                            # the empty selection: x coerced, without a call
        return
    (call,) = r.calls
    assert call[0] == (SVT if is_svt else VECTOR) and call[1] is x
    assert [None if a is None else a.tolist() for a in call[2]] == [None if a is None else list(a) for a in index]
    if is_svt:
        assert call[3] is value
    else:                                               # storage.mode(value) <- the result's type
        want_dtype = np.float64 if new_type == "double" else np.bool_ if call[3].dtype == np.bool_ else np.int32
        assert call[3].dtype == want_dtype and np.array_equal(bits(sa.widen(value, v_type, new_type)),
                                                             bits(call[3].astype(np.int32) if call[3].dtype == np.bool_ else call[3]))


def _x(dim=(5, 4), type_="double", seed=1):
    return sa.make(dim, type_, sa._mask((dim[0], sa.nleaves_of(dim)), 0.5, seed))


def test_every_check_and_message_in_the_reference_s_order():
    from test_arith_cpu import NoCall
    s = Session(NoCall())
    x = _x()
    with pytest.raises(SparseArrayError, match="incorrect number of subscripts"):
        s.subassign(x, 1.0, [1], [1], [1])
    with pytest.raises(SparseArrayError, match="incorrect number of subscripts"):      # before the value's class
        s.subassign(_x((5, 4, 3)), {"a": 1}, [1], [1])
    with pytest.raises(SparseArrayError, match="must be an ordinary vector or array, or an SVT_SparseArray object"):
        s.subassign(x, {"a": 1}, [1], [1])
    with pytest.raises(SparseArrayError, match="must be an ordinary vector or array"):       # before the subscripts
        s.subassign(x, object(), [99], [1])
    with pytest.raises(SparseArrayUnsupported, match="type \"complex\""):
        s.subassign(x, 1j, [1], [1])
    with pytest.raises(SparseArrayUnsupported, match="type \"character\""):
        s.subassign(x, "a", [1], [1])
    with pytest.raises(SparseArrayError, match="subscript out of bounds"):
        s.subassign(x, 1.0, [6], None)
    with pytest.raises(SparseArrayError, match="subscript contains NAs"):
        s.subassign(x, 1.0, None, [float("nan")])
    # the empty selection comes before the vector-length errors: a value of length zero passes
    assert s.subassign(x, np.zeros(0), [], None) is x
    with pytest.raises(SparseArrayError, match="replacement has length zero"):
        s.subassign(x, np.zeros(0), [1], None)
    with pytest.raises(SparseArrayError, match="the supplied value is longer than the selection"):
        s.subassign(x, np.ones(5), [1, 2], [1, 2])
    with pytest.raises(SparseArrayUnsupported, match="recycled across the columns"):       # 4 values over 2 rows x 2 columns
        s.subassign(x, np.ones(4), [1, 2], [1, 2])
    with pytest.raises(SparseArrayUnsupported, match="recycled across the columns"):       # 2 does not divide 3
        s.subassign(x, np.ones(2), [1, 2, 3], None)
    with pytest.raises(SparseArrayError, match="the selection and supplied value must have the same dimensions"):
        s.subassign(x, _x((2, 3)), [1, 2], [1, 2])
    with pytest.raises(SparseArrayError, match="the selection and supplied value must have the same dimensions"):
        s.subassign(x, np.ones((2, 3)), [1, 2], [1, 2])
    with pytest.raises(SparseArrayUnsupported, match="dense array value"):
        s.subassign(x, np.ones((2, 2)), [1, 2], [1, 2])
    na = SVT_SparseArray(x.dim, x.type, x.leaves, na_background=True)
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        s.subassign(na, 1.0, [1], None)
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        s.subassign(x, SVT_SparseArray((1, 4), "double", [None] * 4, na_background=True), [1], None)


def test_no_op_paths_coerce_without_a_call(rec):
    s, r = rec
    xi = sa.make((5, 4), "integer", sa._mask((5, 4), 0.6, 3), "specials")
    assert s.subassign(xi, 7, [], None) is xi
    res = s.subassign(xi, 2.5, None, [])
    assert res.type == "double" and r.calls == []
    want = xi.to_dense().astype(np.float64)
    want[xi.to_dense() == NA_integer] = NA_real
    assert np.array_equal(bits(res.to_dense()), bits(want))
    xl = sa.make((5, 4), "logical", sa._mask((5, 4), 0.6, 4), "specials")
    res = s.subassign(xl, 3, [], [])
    assert res.type == "integer" and r.calls == [] and np.array_equal(res.to_dense(), xl.to_dense())
    assert s.subassign(xl, True, [], None) is xl


@pytest.mark.parametrize("tx", sa.TYPE_ORDER)
@pytest.mark.parametrize("tv", sa.TYPE_ORDER)
def test_type_rule_and_dimnames(rec, tx, tv):
    s, r = rec
    x = _x((5, 4), tx)
    x = SVT_SparseArray(x.dim, x.type, x.leaves, dimnames=[list("abcde"), None])
    value = {"logical": True, "integer": 3, "double": 2.5}[tv]
    res = s.subassign(x, value, [2], None)
    assert res.type == sa.wider(tx, tv) and res.dimnames == [list("abcde"), None]
    # storage.mode(value) <- the result's type
    assert r.calls[0][3].dtype == {"logical": np.bool_, "integer": np.int32, "double": np.float64}[sa.wider(tx, tv)]


def test_a_library_without_the_entries_is_unsupported():
    class Lacking:
        def has_entry(self, name):
            return False

        def __call__(self, name, *args):
            raise AssertionError(f"{name} was called")

    s, x = Session(Lacking()), _x()
    with pytest.raises(SparseArrayUnsupported, match=f"{VECTOR} is not offered"):
        s.subassign(x, 1.0, [1], None)
    with pytest.raises(SparseArrayUnsupported, match=f"{SVT} is not offered"):
        s.subassign(x, _x((1, 4)), [1], None)
    assert s.subassign(x, 1.0, [], None) is x            # no call: no entry needed


# ---------------------------------------------------------------------------
# the library without a device: the tile, the sizes and the refusals decided on the host
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


def test_tile_and_ws_bytes(lib):
    from sparsearray_amd.device import arith_tile, subassign_tile
    assert subassign_tile() == sa.P and arith_tile() == sa.T
    f = lib.svt_dev_subassign_place_ws_bytes
    assert f(0, 0) % 256 == 0 and f(0, 0) >= 256 and f(-3, -9) == f(0, 0)
    for nrow, ncol in ((1, 1), (1000, 3), (3, 1000), (100000, 7000)):
        # carved at multiples of 256: the head; per row 4 (last) + 8 (scan) + 4 + 8 (patch leaf); per leaf 4 + 8
        assert f(nrow, ncol) % 256 == 0 and f(nrow, ncol) >= 256 + 24 * nrow + 8 + 12 * ncol + 8
    assert all(f(n + 1, 5) >= f(n, 5) and f(5, n + 1) >= f(5, n) for n in range(0, 9000, 61))


def _outputs():
    return (np.full(8, -7, dtype=np.int64), np.full(8, 0xA5, dtype=np.uint8), np.full(8, 0xA5, dtype=np.uint8),
            ctypes.c_int64(-7), np.full(1 << 16, 0xA5, dtype=np.uint8))


def _untouched(cp, cr, cl, nnz, ws):
    return (cp == -7).all() and (cr == 0xA5).all() and (cl == 0xA5).all() and nnz.value == -7 and (ws == 0xA5).all()


VECTOR_REFUSALS = [
    # (what, nrow, ncol, rows given, nrows_sel, leaves given, nleaves_sel, nvals, v_Rtype, message)
    ("nvals_0", 5, 4, True, 2, True, 2, 0, REALSXP, "replacement has length zero"),
    ("type_character", 5, 4, True, 2, True, 2, 1, 16, "logical.*integer.*double"),
    ("negative_extent", -1, 4, True, 2, True, 2, 1, REALSXP, "extents"),
    ("too_many_leaves", 5, 2 ** 31 - 1, True, 2, True, 2, 1, REALSXP, "extents"),
    ("rows_missing", 5, 4, False, 2, True, 2, 1, REALSXP, "a subscript is needed"),
    ("leaves_missing", 5, 4, True, 2, False, 2, 1, REALSXP, "a subscript is needed"),
    ("too_many_row_subscripts", 5, 4, True, 2 ** 31, True, 2, 1, REALSXP, "at most"),
]


@pytest.mark.parametrize("what,nrow,ncol,rows,nr,leaves,nl,nvals,rt,msg", VECTOR_REFUSALS, ids=[r[0] for r in VECTOR_REFUSALS])
def test_vector_placement_refusals_need_no_gpu(lib, what, nrow, ncol, rows, nr, leaves, nl, nvals, rt, msg):
    import re
    idx = np.zeros(8, dtype=np.int32)
    vals = np.ones(8)
    cp, cr, cl, nnz, ws = _outputs()
    args = (nrow, ncol, idx.ctypes.data if rows else None, nr, idx.ctypes.data if leaves else None, nl, vals.ctypes.data, nvals, rt)
    assert lib.svt_dev_subassign_place_vector_count(*args, cp.ctypes.data, cr.ctypes.data, cl.ctypes.data, ctypes.byref(nnz),
                                                    ws.ctypes.data, ws.size, None) < 0
    assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
    assert lib.svt_dev_subassign_place_vector_fill(*args, cp.ctypes.data, 0, None, None, ws.ctypes.data, ws.size, None) < 0
    assert _untouched(cp, cr, cl, nnz, ws)


def test_small_workspace_missing_tables_and_compositions_need_no_gpu(lib):
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN
    idx = np.zeros(8, dtype=np.int32)
    vals = np.ones(8)
    cp, cr, cl, nnz, ws = _outputs()
    need = lib.svt_dev_subassign_place_ws_bytes(5, 4)
    args = (5, 4, idx.ctypes.data, 2, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP)
    assert lib.svt_dev_subassign_place_vector_count(*args, cp.ctypes.data, cr.ctypes.data, cl.ctypes.data, ctypes.byref(nnz),
                                                    ws.ctypes.data, need - 1, None) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_subassign_place_vector_fill(*args, cp.ctypes.data, 0, None, None, ws.ctypes.data, need - 1, None) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_subassign_place_vector_count(*args, cp.ctypes.data, None, cl.ctypes.data, ctypes.byref(nnz),
                                                    ws.ctypes.data, ws.size, None) < 0
    assert "cover table" in lib.svt_last_error().decode()
    # the SVT form and the merge, on handles whose arrays are never read
    x, v, vbad, y = [lib.svt_wrap_device_csc(rt, nr, nc, 0, None, None, None)
                     for rt, nr, nc in ((REALSXP, 5, 4), (INTSXP, 2, 2), (INTSXP, 2, 3), (REALSXP, 5, 3))]
    try:
        svt_args = (5, 4, idx.ctypes.data, 2, idx.ctypes.data, 2)
        outs = (cp.ctypes.data, cr.ctypes.data, cl.ctypes.data, ctypes.byref(nnz), ws.ctypes.data)
        assert lib.svt_dev_subassign_place_svt_count(*svt_args, vbad, *outs, ws.size, None) < 0
        assert "the selection and supplied value must have the same dimensions" in lib.svt_last_error().decode()
        assert lib.svt_dev_subassign_place_svt_count(*svt_args, None, *outs, ws.size, None) < 0
        assert lib.svt_dev_subassign_place_svt_count(*svt_args, v, *outs, need - 1, None) < 0
        assert "workspace too small" in lib.svt_last_error().decode()
        ctypes.c_int32.from_address(v + 56).value = 1   # struct svt_dev_csc: na_background follows the three pointers
        assert lib.svt_dev_subassign_place_svt_count(*svt_args, v, *outs, ws.size, None) > 0
        assert "NaArray" in lib.svt_last_error().decode()
        ctypes.c_int32.from_address(v + 56).value = 0
        # the merge: extents of y that differ, a short workspace, an NaArray operand
        m_out = (cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data)
        assert lib.svt_dev_assign_merge_count(x, y, None, None, *m_out, ws.size, None) < 0
        assert "extents of x" in lib.svt_last_error().decode()
        assert lib.svt_dev_assign_merge_count(x, None, None, None, *m_out, ws.size, None) < 0
        assert lib.svt_dev_assign_merge_count(x, x, None, None, *m_out, lib.svt_dev_arith_merge_ws_bytes(4, 0, 0) - 1, None) < 0
        assert "workspace too small" in lib.svt_last_error().decode()
        assert lib.svt_dev_assign_merge_fill(x, x, None, None, cp.ctypes.data, None, None, ws.ctypes.data,
                                             lib.svt_dev_arith_merge_ws_bytes(4, 0, 0) - 1, None) < 0
        ctypes.c_int32.from_address(x + 56).value = 1
        assert lib.svt_dev_assign_merge_count(x, x, None, None, *m_out, ws.size, None) > 0
        # the compositions: the allocator is never asked
        asked = []
        alloc, release = ALLOC_FN(lambda nbytes, ctx: asked.append(nbytes)), FREE_FN(lambda p, ctx: None)
        res = [ctypes.c_int(-7), ctypes.c_int64(-7)] + [ctypes.c_void_p(0) for _ in range(3)]
        tail = (alloc, release, None, *[ctypes.byref(o) for o in res], None)
        assert lib.svt_dev_subassign_vector(x, idx.ctypes.data, 2, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, *tail) > 0
        ctypes.c_int32.from_address(x + 56).value = 0
        assert lib.svt_dev_subassign_vector(x, idx.ctypes.data, 2, idx.ctypes.data, 2, vals.ctypes.data, 0, REALSXP, *tail) < 0
        assert "replacement has length zero" in lib.svt_last_error().decode()
        assert lib.svt_dev_subassign_svt(x, idx.ctypes.data, 2, idx.ctypes.data, 2, vbad, *tail) < 0
        assert "same dimensions" in lib.svt_last_error().decode()
        assert lib.svt_dev_subassign_vector(None, idx.ctypes.data, 2, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, *tail) < 0
        assert lib.svt_dev_subassign_vector(x, idx.ctypes.data, 2, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP,
                                            ALLOC_FN(), FREE_FN(), None, *[ctypes.byref(o) for o in res], None) < 0
        assert "an allocator is needed" in lib.svt_last_error().decode()
        assert asked == [] and [o.value for o in res[:2]] == [-7, -7] and not any(o.value for o in res[2:])
        assert _untouched(cp, cr, cl, nnz, ws)
    finally:
        for h in (x, v, vbad, y):
            lib.svt_release(h)


# ---------------------------------------------------------------------------
# the host side of the element rule
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/assign_rules_main.cpp, built with the host compiler like tests/arith_rules_main.cpp"""
    exe = tmp_path_factory.mktemp("assign_rules") / "assign_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", str(exe),
                    os.path.join(ROOT, "tests", "assign_rules_main.cpp"), "-lm"], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:-1]
    return ask


def _hexbits(v, t):
    return f"{int(bits(np.array([v], dtype=np.float64 if t == 'd' else np.int32))[0]):x}"


def test_rule_program_states_the_table_of_the_issue(rules):
    """stored in Y: Y's value in the result type; stored in x only, row and leaf covered: dropped; else x's value; kept
    unless the leaf is covered and the value == 0; in an uncovered leaf every x entry is kept whatever its value"""
    ints = [0, 1, -1, 7, 2 ** 31 - 1, NA]
    dbls = list(SPECIALS_F64) + [2.5]
    lines, want = [], []
    for tx, xs in (("i", ints), ("d", dbls)):
        for ty, ys in (("i", ints), ("d", dbls)):
            out_t = "d" if "d" in (tx, ty) else "i"
            for in_y in (0, 1):
                for rc in (0, 1):
                    for lc in (0, 1):
                        if in_y and not lc:
                            continue                    # Y has entries in covered leaves only
                        for xv in xs:
                            for yv in ys:
                                lines.append(f"A {tx} {ty} {in_y} {rc} {lc} {_hexbits(xv, tx)} {_hexbits(yv, ty)}")
                                src, st = (yv, ty) if in_y else (xv, tx)
                                if not in_y and rc and lc:
                                    want.append((0, 0))
                                    continue
                                val = sa.widen(np.array([src], dtype=np.float64 if st == "d" else np.int32),
                                               "double" if st == "d" else "integer", "double" if out_t == "d" else "integer")[0]
                                kept = not (lc and val == 0)
                                want.append((int(kept), int(bits(np.array([val]))[0]) if kept else 0))
    got = [(int(a), int(b, 16)) for a, b in (s.split() for s in rules(lines))]
    assert len(got) == len(want) > 1000
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:5]


def test_rule_program_result_types(rules):
    types = {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}
    lines = [f"T {types[a]} {types[b]}" for a in sa.TYPE_ORDER for b in sa.TYPE_ORDER] + [f"T 16 {REALSXP}", f"T {INTSXP} 15"]
    want = [types[sa.wider(a, b)] for a in sa.TYPE_ORDER for b in sa.TYPE_ORDER] + [0, 0]
    assert [int(s) for s in rules(lines)] == want
