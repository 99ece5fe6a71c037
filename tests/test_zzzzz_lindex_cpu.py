"""Subsetting and subassignment by an L-index or M-index without a GPU: the numpy expectation of tests/lindex_cases.py
on the dense array against its statement on the cells and against a per-leaf restatement of subassign_leaf_by_OPBuf
(src/SparseArray_subassignment.c:453-681); the four Session methods over a recording dispatcher -- every check and
message in the reference's order, the paths without a call; what the library answers without a device (workspace sizes,
sort passes, the refusals decided on the host); the ``__host__`` side of the element rule (svt_rule_assign_cells,
sparsearray_amd/csrc/svt_arith_rules.h) through tests/lindex_rules_main.cpp; and that the named cases reach what they
are named for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lindex_cases as lc
from sparsearray_amd import NA_integer, SVT_SparseArray, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.api import Session
from sparsearray_amd.svt import REALSXP
from subset_cases import NP_DTYPE, SPECIALS_F64, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSET_L, SUBSET_M = "C_subset_SVT_by_Lindex", "C_subset_SVT_by_Mindex"
ASSIGN_L, ASSIGN_M = "C_subassign_SVT_by_Lindex", "C_subassign_SVT_by_Mindex"
NA = int(NA_integer)
INT64_NA = np.iinfo(np.int64).min


def operand_of(x):
    cp, ri, vv = x.to_csc()
    leaf = np.repeat(np.arange(len(cp) - 1, dtype=np.int64), np.diff(cp))
    return lc.Operand(x.dim, x.type, leaf * x.dim[0] + ri, vv, x.na_background)


def svt_of(dim, type_, cells, vals):
    return lc.Operand(dim, type_, cells, vals).svt()


# ---------------------------------------------------------------------------
# the expectation itself
# ---------------------------------------------------------------------------
def restate(op, L, value, v_type):
    """subassign_leaf_by_OPBuf leaf by leaf: the (offset, position) pairs that land in a leaf, in index order, leave
    idx0_to_k_map[offset] = the last position; the walk over the rows then takes the leaf's own entry where no position
    landed, the new value where one did and it is not zero, and nothing where it is zero."""
    new_type = lc.wider(op.type, v_type)
    v = lc.widen(value, v_type, new_type)
    cp, ri, vv = op.csc()
    xv = lc.widen(vv, op.type, new_type)
    opbufs = {}
    for p, cell in enumerate(L.tolist()):
        opbufs.setdefault(cell // op.nrow, []).append((cell % op.nrow, p))
    cells, vals = [], []
    for leaf in sorted(set(opbufs) | set(np.flatnonzero(np.diff(cp)).tolist())):
        k_map = {}
        for idx0, p in opbufs.get(leaf, ()):
            k_map[idx0] = p
        own = {int(ri[e]): e for e in range(cp[leaf], cp[leaf + 1])}
        for i in sorted(set(k_map) | set(own)):
            if i in k_map:
                new = v[k_map[i] % v.size]
                if new == 0:                                # Rvector_elt_is_zero_FUN: -0.0 and 0; not a NaN
                    continue
                cells.append(leaf * op.nrow + i)
                vals.append(new)
            else:
                cells.append(leaf * op.nrow + i)
                vals.append(xv[own[i]])
    return new_type, np.array(cells, dtype=np.int64), np.array(vals, dtype=NP_DTYPE[new_type])


@pytest.mark.parametrize("name", lc.ASSIGN_NAMES)
def test_subassign_expectation_dense_cells_and_per_leaf_agree(name):
    op, L, value, v_type = lc.assign_case(name)
    new_type, cells, vals = lc.assign_expected(name)
    r_type, r_cells, r_vals = restate(op, L, value, v_type)
    assert r_type == new_type and np.array_equal(r_cells, cells) and np.array_equal(bits(r_vals), bits(vals))
    if op.has_dense:
        d_type, flat, stored = lc.dense_subassign(op, L, value, v_type)
        assert d_type == new_type and lc.same_as_dense(cells, vals, flat, stored)
        assert not flat[~stored].any() and not np.signbit(flat[~stored].astype(np.float64)).any()


@pytest.mark.parametrize("name", lc.GATHER_NAMES)
def test_subset_expectation_dense_and_cells_agree(name):
    op, L = lc.GATHER[name]
    want = lc.expect_subset(op, L)
    assert want.dtype == NP_DTYPE[op.type] and want.size == len(L)
    if op.has_dense:
        assert np.array_equal(bits(lc.dense_subset(op, L)), bits(want))


def test_the_cases_reach_what_they_are_named_for():
    from sparsearray_amd.device import lindex_sort_passes
    # the sort: K around the tile edge, the passes by the array's cells, the run across the tile edges
    assert [lc.assign_case(f"unsorted_K_{k}")[1].size for k in (2047, 2048, 2049)] == [lc.S - 1, lc.S, lc.S + 1]
    for name, passes in (("one_pass_200_cells", 1), ("three_passes_90000_cells", 3), ("five_passes_past_2_32_cells", 5)):
        op = lc.assign_case(name)[0]
        assert lindex_sort_passes(op.nrow, op.ncol) == passes == -(-(op.ncells - 1).bit_length() // 8)
    assert lc.assign_case("five_passes_past_2_32_cells")[0].ncells > 2 ** 32
    for name, last_is_zero in (("run_of_5000_last_nonzero", False), ("run_of_5000_last_zero", True)):
        op, L, value, _ = lc.assign_case(name)
        s = np.sort(L)
        run = np.flatnonzero(s == 6000)
        assert lc.longest_run(name) == run.size == 5000
        assert run[0] < lc.S < 2 * lc.S == lc.SCAN < run[-1]        # across two sort tile edges and the scan tile's
        assert (value[np.flatnonzero(L == 6000)[-1]] == 0) == last_is_zero
        assert (6000 in lc.assign_expected(name)[1]) != last_is_zero
    # routes
    for name in lc.ASSIGN_NAMES:
        L = lc.assign_case(name)[1]
        assert (L.size < 2 or bool((np.diff(L) > 0).all())) == (name in lc.SORTED_ROUTE), name
    a, b = lc.assign_case("route_sorted"), lc.assign_case("route_shuffled")
    assert np.unique(b[1]).size == b[1].size and np.array_equal(np.sort(b[1]), a[1]) and not np.array_equal(a[1], b[1])
    assert lc.assign_expected("route_sorted")[1].tobytes() == lc.assign_expected("route_shuffled")[1].tobytes()
    # leaves
    op, L = lc.assign_case("one_index_per_leaf_5000_leaves")[:2]
    assert np.array_equal(L // op.nrow, np.arange(5000) * 2) and op.ncol == 10000
    op, L = lc.assign_case("every_index_in_one_leaf")[:2]
    assert set((L // op.nrow).tolist()) == {3}
    # the merge
    assert [lc.merged_length(f"merged_length_{s}") for s in ("T_minus_1", "T", "T_plus_1")] == [lc.T - 1, lc.T, lc.T + 1]
    op, L = lc.assign_case("pair_split_across_a_tile_edge")[:2]
    places = sorted([(int(c), 0) for c in op.cells] + [(int(c), 1) for c in L])
    assert places.index((1024, 0)) == lc.T - 1 and places.index((1024, 1)) == lc.T
    assert lc.merged_length("route_sorted") > 2 * lc.T
    # zeros and specials: every combination the name lists occurs
    op, L, value, _ = lc.assign_case("zeros_minus_zero_NaN_NA_and_stored_zeros")
    stored_zero = set(op.cells[op.vals == 0].tolist())
    assigned = dict(zip(L.tolist(), value.tolist()))
    zero_cells = {c for c, v in assigned.items() if v == 0}
    assert stored_zero - set(assigned) and stored_zero & zero_cells and stored_zero & (set(assigned) - zero_cells)
    assert zero_cells & set(op.cells.tolist()) and zero_cells - set(op.cells.tolist())
    assert {0x8000000000000000, 0x7FF00000000007A2, 0x7FF8000000000001} <= set(bits(value).tolist())
    kept = dict(zip(*[a.tolist() for a in lc.assign_expected("zeros_minus_zero_NaN_NA_and_stored_zeros")[1:]]))
    assert all(c in kept and kept[c] == 0 for c in stored_zero - set(assigned))          # an uncovered stored zero stays
    assert not any(c in kept for c in zero_cells)
    # types and recycling
    assert {(lc.assign_case(n)[0].type, lc.assign_case(n)[3]) for n in lc.ASSIGN_NAMES if n.startswith("types_")} >= \
           {("integer", "double"), ("logical", "integer"), ("double", "integer")}
    assert (lc.assign_case("types_double_x_integer_values_with_NA")[2] == NA).any()
    K = lc.assign_case("nvals_K")[1].size
    assert [lc.assign_case(n)[2].size for n in ("nvals_1", "nvals_K", "nvals_divides_K")] == [1, K, 30] and K % 30 == 0
    # the gather
    op = lc.column_lengths_operand()
    assert tuple(np.diff(op.csc()[0]).tolist()) == lc.COLUMN_LENGTHS == (0, 1, 2, 3, 64, 65, 5000, 0)
    q = lc.GATHER["column_edges"][1]
    hit = np.isin(q, op.cells)
    for c, n in enumerate(lc.COLUMN_LENGTHS):
        in_c = (q // op.nrow) == c
        assert in_c.any() and (hit[in_c].sum() >= min(n, 2)) and (~hit[in_c]).sum() >= 2
    sp = lc.specials_operand("double")
    assert {0x0, 0x8000000000000000, 0x7FF8000000000001, 0x7FF00000000007A2} <= set(bits(sp.vals).tolist())
    huge, L = lc.GATHER["past_2_32_cells"]
    assert huge.ncells > 2 ** 32 and (L > 2 ** 32).any() and np.isin(huge.cells, L).all()
    assert lc.three_d_operand().dim == (11, 7, 5)


def test_mindex_of_is_the_column_major_coordinates():
    dim = (11, 7, 5)
    L = np.array([0, 10, 11, 76, 77, 384])
    M = lc.mindex_of(dim, L)
    assert M.tolist() == [[0, 0, 0], [10, 0, 0], [0, 1, 0], [10, 6, 0], [0, 0, 1], [10, 6, 4]]
    assert np.array_equal(np.ravel_multi_index(tuple(M.T), dim, order="F"), L)


# ---------------------------------------------------------------------------
# the Session methods over a recording dispatcher
# ---------------------------------------------------------------------------
class Recorder:
    """offers every entry point, records the calls and answers them by the expectation on the cells"""

    def __init__(self):
        self.calls = []

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        x, index = args[:2]
        op = operand_of(x)
        if name in (SUBSET_M, ASSIGN_M):
            assert index.dtype == np.int32 and index.ndim == 2 and index.shape[1] == x.ndim
            L = np.ravel_multi_index(tuple((index.astype(np.int64) - 1).T), x.dim, order="F")
        else:
            assert index.dtype == np.int64 and index.ndim == 1
            L = np.where(index == INT64_NA, INT64_NA, index - 1)
        if name in (SUBSET_L, SUBSET_M):
            return lc.expect_subset(op, L)
        assert name in (ASSIGN_L, ASSIGN_M)
        value = args[2]
        v_type = "logical" if value.dtype == np.bool_ else "double" if value.dtype == np.float64 else "integer"
        assert lc.wider(v_type, x.type) == x.type          # x arrives in the result's type, the value in it or narrower
        new_type, cells, vals = lc.expect_subassign(op, L, value.astype(np.int32) if v_type == "logical" else value, v_type)
        return svt_of(x.dim, new_type, cells, vals)


@pytest.fixture()
def rec():
    r = Recorder()
    return Session(r), r


def _value_for_session(value, v_type):
    if v_type == "logical" and not (np.asarray(value) == NA_integer).any():
        return np.asarray(value) != 0
    return value


SESSION_CASES = [n for n in lc.ASSIGN_NAMES if lc.assign_case(n)[0].has_dense]


@pytest.mark.parametrize("name", SESSION_CASES)
def test_session_subassign_by_Lindex_is_one_call(rec, name):
    s, r = rec
    op, L, value, v_type = lc.assign_case(name)
    new_type, cells, vals = lc.assign_expected(name)
    res = s.subassign_by_Lindex(op.svt(), L + 1, _value_for_session(value, v_type))
    got = operand_of(res)
    assert res.type == new_type and res.dim == op.dim
    assert np.array_equal(got.cells, cells) and np.array_equal(bits(got.vals), bits(vals))
    (call,) = r.calls
    assert call[0] == ASSIGN_L and call[1].type == new_type and np.array_equal(call[2], L + 1)
    # storage.mode(value) <- the result's type
    want_dtype = np.float64 if new_type == "double" else np.bool_ if call[3].dtype == np.bool_ else np.int32
    assert call[3].dtype == want_dtype
    assert np.array_equal(bits(lc.widen(value, v_type, new_type)), bits(call[3].astype(np.int32) if call[3].dtype == np.bool_ else call[3]))


@pytest.mark.parametrize("name", ["three_d", "v_0_w_on_one_cell", "types_integer_x_double_values"])
def test_session_subassign_by_Mindex_is_one_call(rec, name):
    s, r = rec
    op, L, value, v_type = lc.assign_case(name)
    new_type, cells, vals = lc.assign_expected(name)
    M = lc.mindex_of(op.dim, L) + 1
    res = s.subassign_by_Mindex(op.svt(), M.astype(np.float64) + 0.5, value)        # doubles: truncated toward zero
    got = operand_of(res)
    assert res.type == new_type and np.array_equal(got.cells, cells) and np.array_equal(bits(got.vals), bits(vals))
    (call,) = r.calls
    assert call[0] == ASSIGN_M and np.array_equal(call[2], M)


@pytest.mark.parametrize("name", [n for n in lc.GATHER_NAMES if lc.GATHER[n][0].has_dense])
def test_session_subset_by_Lindex_and_Mindex(rec, name):
    s, r = rec
    op, L = lc.GATHER[name]
    want = lc.expect_subset(op, L)
    x = op.svt()
    L1 = np.where(L == lc.LINDEX_NA, np.nan, (L + 1).astype(np.float64))           # a double index, NA as NaN
    got = s.subset_by_Lindex(x, L1)
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want))
    assert r.calls[-1][0] == SUBSET_L and r.calls[-1][2].dtype == np.int64
    if not (L == lc.LINDEX_NA).any() and not (x.svt_is_null and x.ndim > 1):
        got = s.subset_by_Mindex(x, lc.mindex_of(op.dim, L) + 1)
        assert np.array_equal(bits(got), bits(want)) and r.calls[-1][0] == SUBSET_M


def _x(dim=(5, 4), type_="double", n=9, seed=1):
    cells = lc.random_cells(int(np.prod(dim)), n, seed)
    return svt_of(dim, type_, cells, lc.tracer(type_, cells))


def test_every_check_and_message_in_the_reference_s_order():
    from test_arith_cpu import NoCall
    s = Session(NoCall())
    x = _x()
    vector_msg = "the supplied value must be a vector for this form of subassignment to an SVT_SparseArray object"
    # adjust_left_type comes first: the value's class before the index is looked at
    for bad_value in (np.ones((2, 2)), {"a": 1}, _x((1, 1), n=1)):
        with pytest.raises(SparseArrayError, match=vector_msg):
            s.subassign_by_Lindex(x, [999], bad_value)
        with pytest.raises(SparseArrayError, match=vector_msg):
            s.subassign_by_Mindex(x, [[99, 99]], bad_value)
    with pytest.raises(SparseArrayError, match="'Lindex' must be an integer or numeric vector"):
        s.subassign_by_Lindex(x, ["a"], 1.0)
    with pytest.raises(SparseArrayUnsupported, match="character"):
        s.subassign_by_Lindex(x, [1], "a")
    with pytest.raises(SparseArrayUnsupported, match="complex"):
        s.subassign_by_Lindex(x, [1], 1j)
    na = SVT_SparseArray(x.dim, x.type, x.leaves, na_background=True)
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        s.subassign_by_Lindex(na, [1], 1.0)
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        s.subassign_by_Mindex(na, [[1, 1]], 1.0)
    # the empty index comes before the value's length: a value of length zero passes
    assert s.subassign_by_Lindex(x, [], np.zeros(0)) is x
    assert s.subassign_by_Mindex(x, np.zeros((0, 2)), np.zeros(0)) is x
    with pytest.raises(SparseArrayError, match="replacement has length zero"):
        s.subassign_by_Lindex(x, [999], np.zeros(0))                    # before the index's values
    with pytest.raises(SparseArrayError, match="replacement has length zero"):
        s.subassign_by_Mindex(x, [[99, 99]], np.zeros(0))
    for n in (4, 7, 12):                                                # 6 indices: not 1, not 6, no divisor of 6
        with pytest.raises(SparseArrayUnsupported, match="does not\\s+divide it"):
            s.subassign_by_Lindex(x, [999] * 6, np.ones(n))
    for bad in ([0], [21], [1, 20, 20.999, 21.0], [-1], [0.5], np.array([2 ** 40])):
        with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains out-of-bound indices"):
            s.subassign_by_Lindex(x, bad, 1.0)
        with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains out-of-bound indices"):
            s.subset_by_Lindex(x, bad)
    for with_na in ([1, float("nan")], np.array([3, NA], dtype=np.int32)):
        with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains NAs"):
            s.subassign_by_Lindex(x, with_na, 1.0)
    with pytest.raises(SparseArrayError, match="contains out-of-bound indices"):      # element by element: 21 is met first
        s.subassign_by_Lindex(x, [21, float("nan")], 1.0)
    with pytest.raises(SparseArrayError, match="contains NAs"):
        s.subassign_by_Lindex(x, [float("nan"), 21], 1.0)
    with pytest.raises(SparseArrayError, match="contains out-of-bound indices"):      # subsetting: an NA is no offender
        s.subset_by_Lindex(x, [float("nan"), 21])
    # the M-index
    with pytest.raises(SparseArrayError, match="'Mindex' must be a matrix"):
        s.subassign_by_Mindex(x, [1, 1], 1.0)
    with pytest.raises(SparseArrayError, match="ncol\\(Mindex\\) != length\\(dim\\(x\\)\\)"):
        s.subassign_by_Mindex(x, [[1, 1, 1]], 1.0)
    with pytest.raises(SparseArrayError, match="ncol\\(Mindex\\) != length\\(dim\\(x\\)\\)"):
        s.subset_by_Mindex(x, [[1, 1, 1]])
    for call in (lambda M: s.subset_by_Mindex(x, M), lambda M: s.subassign_by_Mindex(x, M, 1.0)):
        for bad in ([[6, 1]], [[1, 5]], [[0, 1]], [[1, 1], [5, 4], [5, 4.999], [5, 5.0]]):
            with pytest.raises(SparseArrayError, match="matrix subscript \\(M-index\\) contains out-of-bound indices"):
                call(bad)
        for with_na in ([[1, float("nan")]], np.array([[1, 1], [NA, 2]], dtype=np.int32)):
            with pytest.raises(SparseArrayError, match="matrix subscript \\(M-index\\) contains NAs"):
                call(with_na)
        with pytest.raises(SparseArrayError, match="contains NAs"):       # row by row: the NA of row 1 before the 9 of row 2
            call([[1, float("nan")], [9, 1]])
        with pytest.raises(SparseArrayError, match="contains out-of-bound indices"):
            call([[9, 1], [1, float("nan")]])
    # a character matrix, in the order of .subset_SVT_by_Mindex
    with pytest.raises(SparseArrayError, match="SparseArray object to subset has no dimnames"):
        s.subset_by_Mindex(x, [["a", "b"]])
    named = SVT_SparseArray(x.dim, x.type, x.leaves, dimnames=[list("abcde"), None])
    with pytest.raises(SparseArrayError, match="subsetting a SparseArray object by a character matrix is not supported at the moment"):
        s.subset_by_Mindex(named, [["a", "b"]])
    with pytest.raises(SparseArrayError, match="invalid matrix subscript type"):
        s.subset_by_Mindex(x, [[{"a": 1}, None]])


def test_paths_without_a_call(rec):
    s, r = rec
    xi = svt_of((5, 4), "integer", [1, 7, 12], lc.specials("integer", 3))
    assert s.subassign_by_Lindex(xi, [], 7) is xi
    res = s.subassign_by_Lindex(xi, [], 2.5)             # the retyped x, NA_integer_ become NA_real_
    assert res.type == "double" and np.array_equal(bits(operand_of(res).vals), bits(lc.widen(lc.specials("integer", 3), "integer", "double")))
    xl = svt_of((5, 4), "logical", [1, 7, 12], lc.specials("logical", 3))
    res = s.subassign_by_Mindex(xl, np.zeros((0, 2), dtype=np.int32), 3)
    assert res.type == "integer" and np.array_equal(operand_of(res).vals, lc.specials("logical", 3))
    # an empty N-d array answers an M-index before it looks at it (C_subset_SVT_by_Mindex)
    empty = SVT_SparseArray((5, 4), "double", [None] * 4)
    assert empty.svt_is_null and s.subset_by_Mindex(empty, [[99, 99], [1, 1]]).tolist() == [0.0, 0.0]
    assert r.calls == []
    # an empty index is still a call for the subsetting (the reference makes it), with an empty answer
    assert s.subset_by_Lindex(xi, []).size == 0 and s.subset_by_Lindex(xi, []).dtype == np.int32


def test_double_indices_are_truncated_toward_zero_after_the_minus_one(rec):
    s, r = rec
    x = _x()
    s.subset_by_Lindex(x, [1.0, 1.9, 20.5, 2.0000001])
    assert r.calls[-1][2].tolist() == [1, 1, 20, 2]
    s.subassign_by_Lindex(x, np.array([3.7, 20.99]), 1.0)
    assert r.calls[-1][2].tolist() == [3, 20]
    s.subset_by_Mindex(x, [[5.9, 4.2]])
    assert r.calls[-1][2].tolist() == [[5, 4]]
    s.subset_by_Lindex(x, np.array([2, NA], dtype=np.int32))
    assert r.calls[-1][2].tolist() == [2, INT64_NA]


@pytest.mark.parametrize("tx", lc.TYPE_ORDER)
@pytest.mark.parametrize("tv", lc.TYPE_ORDER)
def test_type_rule_and_dimnames(rec, tx, tv):
    s, r = rec
    x = _x((5, 4), tx)
    x = SVT_SparseArray(x.dim, x.type, x.leaves, dimnames=[list("abcde"), None])
    value = {"logical": True, "integer": 3, "double": 2.5}[tv]
    s.subassign_by_Lindex(x, [2, 9], value)
    name, passed, _, v = r.calls[0]
    assert passed.type == lc.wider(tx, tv) and passed.dimnames == [list("abcde"), None]
    assert v.dtype == {"logical": np.bool_, "integer": np.int32, "double": np.float64}[lc.wider(tx, tv)]


def test_a_library_without_the_entries_is_unsupported():
    class Lacking:
        def has_entry(self, name):
            return False

        def __call__(self, name, *args):
            raise AssertionError(f"{name} was called")

    s, x = Session(Lacking()), _x()
    for entry, call in ((SUBSET_L, lambda: s.subset_by_Lindex(x, [1])), (SUBSET_M, lambda: s.subset_by_Mindex(x, [[1, 1]])),
                        (ASSIGN_L, lambda: s.subassign_by_Lindex(x, [1], 1.0)),
                        (ASSIGN_M, lambda: s.subassign_by_Mindex(x, [[1, 1]], 1.0))):
        with pytest.raises(SparseArrayUnsupported, match=f"{entry} is not offered"):
            call()
    assert s.subassign_by_Lindex(x, [], 1.0) is x        # no call: no entry needed


# ---------------------------------------------------------------------------
# the library without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


def test_ws_bytes_and_sort_passes(lib):
    f = lib.svt_dev_subassign_place_lindex_ws_bytes
    assert f(0, 0) % 256 == 0 and f(0, 0) >= 256 and f(-3, -9) == f(0, 0)
    for K in (1, 2047, 2048, 2049, 100000, 2 ** 31 - 1):
        # carved at multiples of 256: the head; per index three 8-byte keys and three 4-byte positions; the sort's
        # table of 256 counters per tile of 2048 keys
        ntiles = -(-K // lc.S)
        assert f(K, 5) % 256 == 0 and f(K, 5) >= 256 + 36 * K + 8 + 256 * 8 * ntiles
        assert f(K, 5) == f(K, 5000000)                     # nothing is sized by the leaves
    assert all(f(n + 1, 5) >= f(n, 5) for n in range(0, 9000, 61))
    p = lib.svt_dev_lindex_sort_passes
    assert [p(1, 1), p(16, 16), p(257, 1), p(256, 256), p(256, 257), p(2 ** 16, 2 ** 16), p(65536, 65537),
            p(2 ** 31 - 1, 2 ** 31 - 2)] == [1, 1, 2, 2, 3, 4, 5, 8]
    assert p(0, 5) == 1 and p(5, 0) == 1


def _poison():
    return (np.full(8, -7, dtype=np.int64), ctypes.c_int64(-7), np.full(1 << 16, 0xA5, dtype=np.uint8))


def _untouched(cp, nnz, ws):
    return (cp == -7).all() and nnz.value == -7 and (ws == 0xA5).all()


PLACE_REFUSALS = [
    # (what, nrow, ncol, index given, K, ndim, dim, nvals, v_Rtype, status sign, message)
    ("nvals_0", 5, 4, True, 2, 0, None, 0, REALSXP, -1, "replacement has length zero"),
    ("type_character", 5, 4, True, 2, 0, None, 1, 16, -1, "logical.*integer.*double"),
    ("negative_extent", -1, 4, True, 2, 0, None, 1, REALSXP, -1, "extents"),
    ("too_many_leaves", 5, 2 ** 31 - 1, True, 2, 0, None, 1, REALSXP, -1, "extents"),
    ("index_missing", 5, 4, False, 2, 0, None, 1, REALSXP, -1, "an index of K >= 0 elements is needed"),
    ("K_negative", 5, 4, True, -1, 0, None, 1, REALSXP, -1, "an index of K >= 0 elements is needed"),
    ("K_past_the_limit", 5, 4, True, 2 ** 31, 0, None, 1, REALSXP, 1, "more than 2\\^31 - 1 indices"),
    ("ndim_9", 5, 4, True, 2, 9, (5, 4), 1, REALSXP, -1, "between 1 and 8 dimensions"),
    ("dim_missing", 5, 4, True, 2, 2, None, 1, REALSXP, -1, "between 1 and 8 dimensions"),
    ("dim_rows_differ", 5, 4, True, 2, 2, (4, 5), 1, REALSXP, -1, "'dim' does not match"),
    ("dim_leaves_differ", 5, 4, True, 2, 3, (5, 2, 3), 1, REALSXP, -1, "'dim' does not match"),
]


@pytest.mark.parametrize("what,nrow,ncol,given,K,ndim,dim,nvals,rt,sign,msg", PLACE_REFUSALS, ids=[r[0] for r in PLACE_REFUSALS])
def test_placement_refusals_need_no_gpu(lib, what, nrow, ncol, given, K, ndim, dim, nvals, rt, sign, msg):
    idx = np.zeros(64, dtype=np.int64)
    vals = np.ones(8)
    cp, nnz, ws = _poison()
    dims = None if dim is None else (ctypes.c_int64 * len(dim))(*dim)
    args = (nrow, ncol, idx.ctypes.data if given else None, K, ndim, dims, vals.ctypes.data, nvals, rt)
    big = 1 << 62                                           # (a size no check can find too small: the arrays are never read)
    rc = lib.svt_dev_subassign_place_lindex_count(*args, cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data, big, None)
    assert (rc > 0) if sign > 0 else (rc < 0)
    assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
    rc = lib.svt_dev_subassign_place_lindex_fill(*args, cp.ctypes.data, 0, None, None, ws.ctypes.data, big, None)
    assert (rc > 0) if sign > 0 else (rc < 0)
    assert _untouched(cp, nnz, ws)


def test_short_workspace_gather_and_compositions_need_no_gpu(lib):
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN
    idx = np.zeros(8, dtype=np.int64)
    vals = np.ones(8)
    cp, nnz, ws = _poison()
    need = lib.svt_dev_subassign_place_lindex_ws_bytes(2, 4)
    args = (5, 4, idx.ctypes.data, 2, 0, None, vals.ctypes.data, 1, REALSXP)
    assert lib.svt_dev_subassign_place_lindex_count(*args, cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data, need - 1, None) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_subassign_place_lindex_fill(*args, cp.ctypes.data, 0, None, None, ws.ctypes.data, need - 1, None) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_subassign_place_lindex_count(*args, None, ctypes.byref(nnz), ws.ctypes.data, ws.size, None) < 0
    x, y, xc = [lib.svt_wrap_device_csc(rt, nr, nc, 0, None, None, None)
                for rt, nr, nc in ((REALSXP, 5, 4), (REALSXP, 5, 3), (16, 5, 4))]
    try:
        out, bad = np.full(8, -7.0), np.full(1, -7, dtype=np.int32)
        # the gather: K == 0 is nothing at all; the refusals come before a launch
        assert lib.svt_dev_subset_lindex(x, None, 0, None, None, None) == 0
        assert lib.svt_dev_subset_lindex(None, idx.ctypes.data, 2, out.ctypes.data, bad.ctypes.data, None) < 0
        assert lib.svt_dev_subset_lindex(x, None, 2, out.ctypes.data, bad.ctypes.data, None) < 0
        assert lib.svt_dev_subset_lindex(x, idx.ctypes.data, 2, None, bad.ctypes.data, None) < 0
        assert lib.svt_dev_subset_lindex(x, idx.ctypes.data, 2, out.ctypes.data, None, None) < 0
        assert lib.svt_dev_subset_lindex(xc, idx.ctypes.data, 2, out.ctypes.data, bad.ctypes.data, None) < 0
        assert lib.svt_dev_subset_mindex(x, idx.ctypes.data, 2, 0, None, out.ctypes.data, bad.ctypes.data, None) < 0
        assert lib.svt_dev_subset_mindex(x, idx.ctypes.data, 2, 2, (ctypes.c_int64 * 2)(4, 5), out.ctypes.data, bad.ctypes.data, None) < 0
        assert "'dim' does not match" in lib.svt_last_error().decode()
        assert (out == -7.0).all() and bad[0] == -7
        # the merge: extents of y that differ, a short workspace, an NaArray operand
        m_out = (cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data)
        assert lib.svt_dev_assign_cells_merge_count(x, y, *m_out, ws.size, None) < 0
        assert "extents of x" in lib.svt_last_error().decode()
        assert lib.svt_dev_assign_cells_merge_count(x, None, *m_out, ws.size, None) < 0
        short = lib.svt_dev_arith_merge_ws_bytes(4, 0, 0) - 1
        assert lib.svt_dev_assign_cells_merge_count(x, x, *m_out, short, None) < 0
        assert "workspace too small" in lib.svt_last_error().decode()
        assert lib.svt_dev_assign_cells_merge_fill(x, x, cp.ctypes.data, None, None, ws.ctypes.data, short, None) < 0
        ctypes.c_int32.from_address(x + 56).value = 1       # struct svt_dev_csc: na_background follows the three pointers
        assert lib.svt_dev_assign_cells_merge_count(x, x, *m_out, ws.size, None) > 0
        # the compositions: the allocator is never asked
        asked = []
        alloc, release = ALLOC_FN(lambda nbytes, ctx: asked.append(nbytes)), FREE_FN(lambda p, ctx: None)
        res = [ctypes.c_int(-7), ctypes.c_int64(-7)] + [ctypes.c_void_p(0) for _ in range(3)]
        tail = (alloc, release, None, *[ctypes.byref(o) for o in res], None)
        assert lib.svt_dev_subassign_lindex(x, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, *tail) > 0
        assert "NaArray" in lib.svt_last_error().decode()
        ctypes.c_int32.from_address(x + 56).value = 0
        assert lib.svt_dev_subassign_lindex(x, idx.ctypes.data, 2, vals.ctypes.data, 0, REALSXP, *tail) < 0
        assert "replacement has length zero" in lib.svt_last_error().decode()
        assert lib.svt_dev_subassign_lindex(x, idx.ctypes.data, 2 ** 31, vals.ctypes.data, 1, REALSXP, *tail) > 0
        assert lib.svt_dev_subassign_lindex(x, idx.ctypes.data, 2, vals.ctypes.data, 1, 16, *tail) < 0
        assert lib.svt_dev_subassign_lindex(xc, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, *tail) < 0
        assert lib.svt_dev_subassign_lindex(None, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, *tail) < 0
        assert lib.svt_dev_subassign_mindex(x, idx.ctypes.data, 2, 0, None, vals.ctypes.data, 1, REALSXP, *tail) < 0
        assert lib.svt_dev_subassign_mindex(x, idx.ctypes.data, 2, 2, (ctypes.c_int64 * 2)(5, 5), vals.ctypes.data, 1, REALSXP, *tail) < 0
        assert lib.svt_dev_subassign_lindex(x, idx.ctypes.data, 2, vals.ctypes.data, 1, REALSXP, ALLOC_FN(), FREE_FN(), None,
                                            *[ctypes.byref(o) for o in res], None) < 0
        assert "an allocator is needed" in lib.svt_last_error().decode()
        assert asked == [] and [o.value for o in res[:2]] == [-7, -7] and not any(o.value for o in res[2:])
        assert _untouched(cp, nnz, ws)
    finally:
        for h in (x, y, xc):
            lib.svt_release(h)


def test_route_counts_start_at_zero_and_reset(lib):
    buf = (ctypes.c_int64 * 2)(-1, -1)
    lib.svt_dev_lindex_route_counts(buf, 1)
    lib.svt_dev_lindex_route_counts(buf, 0)
    assert list(buf) == [0, 0]


# ---------------------------------------------------------------------------
# the host side of the element rule
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/lindex_rules_main.cpp, built with the host compiler like tests/assign_rules_main.cpp"""
    exe = tmp_path_factory.mktemp("lindex_rules") / "lindex_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", str(exe),
                    os.path.join(ROOT, "tests", "lindex_rules_main.cpp"), "-lm"], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:-1]
    return ask


def _hexbits(v, t):
    return f"{int(bits(np.array([v], dtype=np.float64 if t == 'd' else np.int32))[0]):x}"


def test_rule_program_states_the_rule_of_the_cells(rules):
    """stored in Y: Y's value in the result type, kept iff it is not zero; stored in x alone: x's value in the result
    type, always kept -- a stored zero, a -0.0 and an NA included"""
    ints = [0, 1, -1, 7, 2 ** 31 - 1, NA]
    dbls = list(SPECIALS_F64) + [2.5]
    lines, want = [], []
    for tx, xs in (("i", ints), ("d", dbls)):
        for ty, ys in (("i", ints), ("d", dbls)):
            out_t = "d" if "d" in (tx, ty) else "i"
            for in_y in (0, 1):
                for xv in xs:
                    for yv in ys:
                        lines.append(f"C {tx} {ty} {in_y} {_hexbits(xv, tx)} {_hexbits(yv, ty)}")
                        src, st = (yv, ty) if in_y else (xv, tx)
                        val = lc.widen(np.array([src], dtype=np.float64 if st == "d" else np.int32),
                                       "double" if st == "d" else "integer", "double" if out_t == "d" else "integer")[0]
                        kept = not (in_y and val == 0)
                        want.append((int(kept), int(bits(np.array([val]))[0]) if kept else 0))
    got = [(int(a), int(b, 16)) for a, b in (s.split() for s in rules(lines))]
    assert len(got) == len(want) > 300
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:5]
    # x alone always stays: a stored 0.0 and a stored -0.0 with their own bits
    assert (1, 0) in got and (1, 0x8000000000000000) in got
