"""Subsetting and subassignment by an L-index or M-index on the device (kernels_lindex.hip gathers and places,
kernels_arith.hip merges under the rule of the cells): every case of tests/lindex_cases.py through
DeviceCSC.subset_lindex / subset_mindex / subassign_lindex / subassign_mindex on resident operands, values AS BITS and
the stored cells at tolerance 0; the two routes of the placement, asserted by their counters; the count / fill primitives
in arenas of poisoned bytes with guard bands; every status, with the outputs keeping their contents; determinism; the
chains nzwhich -> subassign and nzwhich -> subset; and the four Session methods over the HIP dispatcher."""
import ctypes

import numpy as np
import pytest

import lindex_cases as lc
from helpers import Arena
from subset_cases import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    import sparsearray_amd.device as d
    assert d.arith_tile() == lc.T and d.LINDEX_NA == lc.LINDEX_NA
    return d


def to_dev(dev, op):
    cp, ri, vv = op.csc()
    A = dev.DeviceCSC.from_host(op.nrow, cp, ri, np.array(vv))      # (a copy: the cases' arrays are read-only)
    if op.type == "logical":
        A = dev.DeviceCSC(op.nrow, A.col_ptr, A.row_idx, A.val, logical=True)
    if op.na_background:
        ctypes.c_int32.from_address(A._h + 56).value = 1   # struct svt_dev_csc: na_background follows the three pointers
    return A


def cells_of(R):
    """(type, sorted stored cells, values) of a device operand; the rows of every leaf must ascend"""
    from sparsearray_amd.svt import LGLSXP, REALSXP
    cp, ri, vv = R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()
    assert cp[0] == 0 and cp[-1] == ri.size == vv.size == R.nnz and (np.diff(cp) >= 0).all()
    leaf = np.repeat(np.arange(R.ncol, dtype=np.int64), np.diff(cp))
    cells = leaf * R.nrow + ri
    assert (np.diff(cells) > 0).all() and (ri >= 0).all() and (ri < max(R.nrow, 1)).all()
    return ("double" if R.Rtype == REALSXP else "logical" if R.Rtype == LGLSXP else "integer"), cells, vv


def check_assigned(R, name, what=""):
    new_type, cells, vals = lc.assign_expected(name)
    got_type, got_cells, got_vals = cells_of(R)
    assert got_type == new_type, f"{what}{name}: type"
    assert np.array_equal(got_cells, cells), f"{what}{name}: the stored cells"
    assert got_vals.dtype == vals.dtype and np.array_equal(bits(got_vals), bits(vals)), f"{what}{name}: the values as bits"


def arrays(R):
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def same_arrays(a, b, what=""):
    for x, y, part in zip(a, b, ("col_ptr", "row_idx", "val")):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x) if x.dtype != np.int64 else x,
                                                                             bits(y) if y.dtype != np.int64 else y), f"{what}: {part}"


def _t(a):
    import torch
    return torch.as_tensor(np.array(a, order="C"), device="cuda")            # (a copy: the cases' arrays are read-only)


# ---------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.GATHER_NAMES)
def test_gather_by_lindex_and_by_mindex(dev, name):
    op, L = lc.GATHER[name]
    want = lc.expect_subset(op, L)
    X = to_dev(dev, op)
    got = X.subset_lindex(_t(np.asarray(L, dtype=np.int64)))
    assert got.numel() == len(L) and np.array_equal(bits(got.cpu().numpy().astype(want.dtype, copy=False)), bits(want)), name
    if not (np.asarray(L) == lc.LINDEX_NA).any():         # an M-index has no NA
        got = X.subset_mindex(_t(lc.mindex_of(op.dim, L)), dim=op.dim)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), name + ": M-index"
        got = X.subset_mindex(lc.mindex_of(op.dim, L), dim=op.dim)           # an array-like: uploaded row-major, handed over column-major
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), name + ": M-index from the host"


def test_gather_out_of_bound_raises_and_writes_nothing(dev):
    import torch
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd._hip import init
    lib = init()
    op = lc.column_lengths_operand()
    X = to_dev(dev, op)
    for bad_index in (op.ncells, -1, 2 ** 62, lc.LINDEX_NA + 1):
        L = np.array([7, bad_index, 8], dtype=np.int64)
        with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains out-of-bound indices"):
            X.subset_lindex(L)
        arena = Arena([8 * 3, 4])
        arena.part(1, torch.int32)[:] = 0
        idx = _t(L)
        assert lib.svt_dev_subset_lindex(X.handle, idx.data_ptr(), 3, arena.part(0).data_ptr(), arena.part(1).data_ptr(),
                                         _stream()) == 0
        torch.cuda.synchronize()
        assert int(arena.part(1, torch.int32)[0]) == 1 and bool((arena.part(0) == 0xA5).all()) and arena.guards_intact()
    d3 = lc.three_d_operand()
    X3 = to_dev(dev, d3)
    for row in ([11, 0, 0], [0, 7, 0], [0, 0, 5], [-1, 0, 0], [0, int(lc.NA_integer), 0]):
        with pytest.raises(SparseArrayError, match="matrix subscript \\(M-index\\) contains out-of-bound indices"):
            X3.subset_mindex(np.array([[1, 1, 1], row], dtype=np.int32), dim=d3.dim)
    with pytest.raises(SparseArrayError, match="'dim' does not match"):
        X3.subset_mindex(np.zeros((1, 3), dtype=np.int32), dim=(11, 5, 7, 1)[:3][::-1])
    # a good index after all of this: the word was the call's own
    assert np.array_equal(bits(X.subset_lindex(op.cells[:5]).cpu().numpy()), bits(op.vals[:5]))


def test_gather_takes_what_nzwhich_gives(dev):
    for op in (lc.column_lengths_operand(), lc.specials_operand("double"), lc.three_d_operand(), lc.huge_operand()):
        X = to_dev(dev, op)
        same = X.subset_lindex(X.nzwhich())
        assert np.array_equal(bits(same.cpu().numpy()), bits(op.vals))
        if op.ncol <= 2 ** 31 - 1:
            same = X.subset_mindex(X.nzwhich(dim=op.dim, arr_ind=True), dim=op.dim)
            assert np.array_equal(bits(same.cpu().numpy()), bits(op.vals))


# ---------------------------------------------------------------------------
# placement and merge
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.ASSIGN_NAMES)
def test_subassign_by_lindex(dev, name):
    op, L, value, v_type = lc.assign_case(name)
    X = to_dev(dev, op)
    dev.lindex_route_counts(reset=True)
    R = X.subassign_lindex(_t(L), _t(value), logical=v_type == "logical")
    check_assigned(R, name, "subassign_lindex: ")
    sorted_route = name in lc.SORTED_ROUTE
    assert dev.lindex_route_counts() == {"sorted": int(sorted_route), "unsorted": int(not sorted_route)}


@pytest.mark.parametrize("name", ["three_d", "v_0_w_on_one_cell", "run_of_5000_last_zero", "route_sorted", "route_shuffled",
                                  "three_passes_90000_cells", "types_double_x_integer_values_with_NA"])
def test_subassign_by_mindex(dev, name):
    op, L, value, v_type = lc.assign_case(name)
    R = to_dev(dev, op).subassign_mindex(_t(lc.mindex_of(op.dim, L)), value, dim=op.dim, logical=v_type == "logical")
    check_assigned(R, name, "subassign_mindex: ")


def test_the_two_routes_give_identical_bits(dev):
    a, b = lc.assign_case("route_sorted"), lc.assign_case("route_shuffled")
    X = to_dev(dev, a[0])
    dev.lindex_route_counts(reset=True)
    Ra = X.subassign_lindex(a[1], a[2])
    assert dev.lindex_route_counts() == {"sorted": 1, "unsorted": 0}
    Rb = X.subassign_lindex(b[1], b[2])
    assert dev.lindex_route_counts(reset=True) == {"sorted": 1, "unsorted": 1}
    same_arrays(arrays(Ra), arrays(Rb), "sorted and shuffled")
    assert dev.lindex_route_counts() == {"sorted": 0, "unsorted": 0}


@pytest.mark.parametrize("name", ["unsorted_K_2049", "run_of_5000_last_nonzero", "five_passes_past_2_32_cells", "route_sorted",
                                  "types_integer_x_double_values"])
def test_the_same_call_twice_gives_the_same_arrays(dev, name):
    op, L, value, v_type = lc.assign_case(name)
    X = to_dev(dev, op)
    same_arrays(arrays(X.subassign_lindex(L, value)), arrays(X.subassign_lindex(L, value)), name)


def test_empty_index_is_the_widening_copy(dev):
    op = lc.specials_operand("integer")
    X = to_dev(dev, op)
    R = X.subassign_lindex(np.zeros(0, dtype=np.int64), 2.5)
    t, cells, vals = cells_of(R)
    assert t == "double" and np.array_equal(cells, op.cells) and np.array_equal(bits(vals), bits(lc.widen(op.vals, "integer", "double")))
    R = X.subassign_mindex(np.zeros((0, 2), dtype=np.int32), 7)
    same_arrays(arrays(R), arrays(X), "an empty M-index")


# ---------------------------------------------------------------------------
# the workspace contract (include/svt_hip.h, "Workspaces"): the four primitives in arenas with guard bands
# ---------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _primitives(dev, name, prior, matrix):
    """(col_ptr, row_idx, val) of the placement's count + fill and the merge's count + fill, each pair in an Arena whose
    workspace held ``prior`` bytes; the guards of both arenas checked; Y checked against the last value per cell"""
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    op, L, value, v_type = lc.assign_case(name)
    new_type, cells, _ = lc.assign_expected(name)
    X = to_dev(dev, op)
    K, nrow, ncol = L.size, op.nrow, op.ncol
    if matrix:
        idx = _t(np.ascontiguousarray(lc.mindex_of(op.dim, L).T))
        index = (idx.data_ptr(), K, len(op.dim), (ctypes.c_int64 * len(op.dim))(*op.dim))
    else:
        idx = _t(L)
        index = (idx.data_ptr(), K, 0, None)
    vals, v_Rtype = dev._assign_values(value, X.val.device, v_type == "logical")
    y_nnz = int(np.unique(L).size)
    v_esz = vals.element_size()
    need = lib.svt_dev_subassign_place_lindex_ws_bytes(K, ncol)
    a1 = Arena([need, 8 * (ncol + 1), 4 * y_nnz, v_esz * y_nnz])
    a1.part(0)[:] = prior
    p = [_ptr(a1.part(k)) for k in range(4)]
    what = (nrow, ncol, *index, vals.data_ptr(), vals.numel(), v_Rtype, p[1])
    got = ctypes.c_int64(-1)
    assert lib.svt_dev_subassign_place_lindex_count(*what, ctypes.byref(got), p[0], need, _stream()) == 0, lib.svt_last_error()
    assert got.value == y_nnz
    assert lib.svt_dev_subassign_place_lindex_fill(*what, y_nnz, p[2], p[3], p[0], need, _stream()) == 0, lib.svt_last_error()
    torch.cuda.synchronize()
    assert a1.guards_intact(), name + ": the placement"
    Y = dev.DeviceCSC(nrow, a1.part(1, torch.int64), a1.part(2, torch.int32),
                      a1.part(3, torch.float64 if v_esz == 8 else torch.int32), logical=v_type == "logical")
    # Y: one entry per distinct cell, the last value of the cell, zeros included
    _, y_cells, y_vals = cells_of(Y)
    last = {}
    for q, cell in enumerate(L.tolist()):
        last[cell] = value[q % value.size]
    assert np.array_equal(y_cells, np.array(sorted(last), dtype=np.int64)), name + ": the cells of Y"
    assert np.array_equal(bits(y_vals), bits(np.array([last[c] for c in sorted(last)], dtype=value.dtype))), name + ": the values of Y"
    nnz, esz = cells.size, 8 if new_type == "double" else 4
    need2 = lib.svt_dev_arith_merge_ws_bytes(ncol, X.nnz, y_nnz)
    a2 = Arena([need2, 8 * (ncol + 1), 4 * nnz, esz * nnz])
    a2.part(0)[:] = prior
    q = [_ptr(a2.part(k)) for k in range(4)]
    got = ctypes.c_int64(-1)
    assert lib.svt_dev_assign_cells_merge_count(X.handle, Y.handle, q[1], ctypes.byref(got), q[0], need2, _stream()) == 0, \
        lib.svt_last_error()
    assert got.value == nnz
    assert lib.svt_dev_assign_cells_merge_fill(X.handle, Y.handle, q[1], q[2], q[3], q[0], need2, _stream()) == 0
    torch.cuda.synchronize()
    assert a2.guards_intact() and a1.guards_intact(), name + ": the merge"
    return (a2.part(1, torch.int64).cpu().numpy(), a2.part(2, torch.int32).cpu().numpy(),
            a2.part(3, torch.float64 if esz == 8 else torch.int32).cpu().numpy())


@pytest.mark.parametrize("name", ["unsorted_K_2048", "run_of_5000_last_zero", "one_index_per_leaf_shuffled", "merged_length_T",
                                  "pair_split_across_a_tile_edge", "zeros_minus_zero_NaN_NA_and_stored_zeros",
                                  "types_logical_x_integer_values", "nvals_divides_K", "three_d", "x_empty"])
def test_workspace_discipline(dev, name):
    op = lc.assign_case(name)[0]
    new_type, cells, vals = lc.assign_expected(name)
    want = lc.Operand(op.dim, new_type, cells, vals).csc()
    same_arrays(_primitives(dev, name, 0xA5, False), want, name)    # every output cell is written: none is 0xA5 by luck
    same_arrays(_primitives(dev, name, 0x00, True), want, name + ", M-index, workspace of zeros")
    same_arrays(_primitives(dev, name, 0xFF, False), want, name + ", workspace of ones")


# ---------------------------------------------------------------------------
# statuses: a non-zero status leaves every output as it was
# ---------------------------------------------------------------------------
def _refused_placement(dev, lib, L, nvals, sign, msg, nrow=37, ncol=23, short=0, M=None, dim=None):
    import re
    import torch
    if M is not None:
        idx = _t(np.ascontiguousarray(np.asarray(M, dtype=np.int32).T))
        index = (idx.data_ptr(), len(M), len(dim), (ctypes.c_int64 * len(dim))(*dim))
    else:
        idx = _t(np.asarray(L, dtype=np.int64))
        index = (idx.data_ptr(), len(L), 0, None)
    vals = _t(np.ones(4))
    need = lib.svt_dev_subassign_place_lindex_ws_bytes(index[1], ncol)
    arena = Arena([need, 8 * (ncol + 1), 4096, 4096])
    p = [arena.part(k).data_ptr() for k in range(4)]
    nnz = ctypes.c_int64(-7)
    from sparsearray_amd.svt import REALSXP
    rc = lib.svt_dev_subassign_place_lindex_count(nrow, ncol, *index, vals.data_ptr(), nvals, REALSXP, p[1], ctypes.byref(nnz),
                                                  p[0], need - short, _stream())
    assert (rc > 0) if sign > 0 else (rc < 0), (rc, lib.svt_last_error())
    assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.guards_intact()
    assert all(bool((arena.part(k) == 0xA5).all()) for k in range(1, 4)), "an output was written on a non-zero status"
    if short or nvals < 1:
        assert arena.untouched()


def test_placement_statuses_leave_the_outputs_untouched(dev):
    from sparsearray_amd._hip import init
    lib = init()
    bad = "linear index \\(L-index\\) contains out-of-bound indices or NAs"
    _refused_placement(dev, lib, [0, 37 * 23], 1, -1, bad)
    _refused_placement(dev, lib, [0, -1], 1, -1, bad)
    _refused_placement(dev, lib, [5, lc.LINDEX_NA, 6], 1, -1, bad)
    _refused_placement(dev, lib, list(range(3000)) + [2 ** 40], 1, -1, bad)        # the offender in the second block
    _refused_placement(dev, lib, [0, 1], 0, -1, "replacement has length zero")
    _refused_placement(dev, lib, [0, 1], 1, -1, "workspace too small", short=1)
    badm = "matrix subscript \\(M-index\\) contains out-of-bound indices or NAs"
    _refused_placement(dev, lib, None, 1, -1, badm, M=[[0, 0], [37, 0]], dim=(37, 23))
    _refused_placement(dev, lib, None, 1, -1, badm, M=[[0, 23], [1, 1]], dim=(37, 23))
    _refused_placement(dev, lib, None, 1, -1, badm, M=[[0, 0], [1, int(lc.NA_integer)]], dim=(37, 23))


def test_composition_statuses(dev):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    op = lc.specials_operand("double")
    X = to_dev(dev, op)
    before = arrays(X)
    with pytest.raises(SparseArrayError, match="out-of-bound indices or NAs"):
        X.subassign_lindex([0, op.ncells], 1.0)
    with pytest.raises(SparseArrayError, match="out-of-bound indices or NAs"):
        X.subassign_lindex([0, lc.LINDEX_NA], 1.0)
    with pytest.raises(SparseArrayError, match="M-index.*out-of-bound indices or NAs"):
        X.subassign_mindex(np.array([[0, 0], [0, 23]], dtype=np.int32), 1.0)
    with pytest.raises(SparseArrayError, match="replacement has length zero"):
        X.subassign_lindex([0, 1], np.zeros(0))
    with pytest.raises(SparseArrayError, match="'dim' does not match"):
        X.subassign_mindex(np.zeros((1, 2), dtype=np.int32), 1.0, dim=(23, 37))
    NA_X = to_dev(dev, lc.Operand(op.dim, op.type, op.cells, op.vals, na_background=True))
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        NA_X.subassign_lindex([0, 1], 1.0)
    same_arrays(arrays(X), before, "x after the refusals")


def test_merge_status_of_a_short_workspace_leaves_the_outputs_untouched(dev):
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    op, L, value, _ = lc.assign_case("route_shuffled")
    X = to_dev(dev, op)
    Y = dev.lindex_place(X, L, value)
    need = lib.svt_dev_arith_merge_ws_bytes(X.ncol, X.nnz, Y.nnz)
    arena = Arena([need, 8 * (X.ncol + 1), 4096, 4096])
    p = [arena.part(k).data_ptr() for k in range(4)]
    nnz = ctypes.c_int64(-7)
    assert lib.svt_dev_assign_cells_merge_count(X.handle, Y.handle, p[1], ctypes.byref(nnz), p[0], need - 1, _stream()) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_assign_cells_merge_fill(X.handle, Y.handle, p[1], p[2], p[3], p[0], need - 1, _stream()) < 0
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.untouched()
    # and the two-call route gives what the composition gives
    same_arrays(arrays(dev.assign_cells_merge(X, Y)), arrays(X.subassign_lindex(L, value)), "two calls")


# ---------------------------------------------------------------------------
# chains that stay resident
# ---------------------------------------------------------------------------
def test_chain_cap_the_outliers(dev):
    """x[nzwhich(x > s)] <- s is min(x, s) on an operand without negative zeros; three tiles of the merge"""
    rng = np.random.default_rng(90)
    cells = lc.random_cells(500 * 40, 4500, 91)
    vals = np.round(rng.normal(0.0, 4.0, cells.size), 2)
    vals[vals == 0] = 0.5
    op = lc.Operand((500, 40), "double", cells, vals)
    X = to_dev(dev, op)
    s = 3.0
    which = X.compare(">", s).nzwhich()
    assert which.numel() == int((vals > s).sum()) > 500 and X.nnz + which.numel() > 2 * lc.T
    dev.lindex_route_counts(reset=True)
    R = X.subassign_lindex(which, s)
    assert dev.lindex_route_counts() == {"sorted": 1, "unsorted": 0}
    t, got_cells, got_vals = cells_of(R)
    assert t == "double" and np.array_equal(got_cells, cells) and np.array_equal(bits(got_vals), bits(np.minimum(vals, s)))
    dense = np.zeros(op.ncells)
    dense[cells] = vals
    assert np.array_equal(R.to_dense().cpu().numpy().reshape(-1, order="F"), np.minimum(dense, s))
    # by coordinates, and with s = 0: every outlier deleted
    R0 = X.subassign_mindex(X.compare(">", s).nzwhich(arr_ind=True), 0.0)
    t, got_cells, got_vals = cells_of(R0)
    assert np.array_equal(got_cells, cells[vals <= s]) and np.array_equal(bits(got_vals), bits(vals[vals <= s]))
    assert np.array_equal(bits(X.subset_lindex(X.nzwhich()).cpu().numpy()), bits(X.val.cpu().numpy()))


# ---------------------------------------------------------------------------
# host level: Session over the HIP dispatcher
# ---------------------------------------------------------------------------
def _host_cells(x):
    cp, ri, vv = x.to_csc()
    leaf = np.repeat(np.arange(len(cp) - 1, dtype=np.int64), np.diff(cp))
    return x.type, leaf * x.dim[0] + ri, vv


@pytest.mark.parametrize("name", ["unsorted_K_2049", "zeros_minus_zero_NaN_NA_and_stored_zeros", "types_integer_x_double_values",
                                  "route_sorted"])
def test_session_subassign_by_Lindex(hip, name):
    op, L, value, v_type = lc.assign_case(name)
    new_type, cells, vals = lc.assign_expected(name)
    res = hip.subassign_by_Lindex(op.svt(), L + 1, value)
    t, got_cells, got_vals = _host_cells(res)
    assert t == new_type and res.dim == op.dim
    assert np.array_equal(got_cells, cells) and np.array_equal(bits(got_vals), bits(vals)), name


def test_session_subassign_by_Mindex_three_d(hip):
    op, L, value, v_type = lc.assign_case("three_d")
    new_type, cells, vals = lc.assign_expected("three_d")
    res = hip.subassign_by_Mindex(op.svt(), lc.mindex_of(op.dim, L) + 1, value)
    t, got_cells, got_vals = _host_cells(res)
    assert t == new_type and res.dim == op.dim and np.array_equal(got_cells, cells) and np.array_equal(bits(got_vals), bits(vals))


@pytest.mark.parametrize("name", ["column_edges_shuffled_with_repeats", "NA_indices", "specials_double_every_cell",
                                  "na_background_double", "three_d", "K_0"])
def test_session_subset_by_Lindex_and_Mindex(hip, name):
    op, L = lc.GATHER[name]
    want = lc.expect_subset(op, L)
    x = op.svt()
    L1 = np.where(np.asarray(L) == lc.LINDEX_NA, np.nan, (np.asarray(L) + 1).astype(np.float64))
    got = hip.subset_by_Lindex(x, L1)
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), name
    if not (np.asarray(L) == lc.LINDEX_NA).any():
        got = hip.subset_by_Mindex(x, lc.mindex_of(op.dim, L) + 1)
        assert np.array_equal(bits(got), bits(want)), name + ": M-index"


def test_session_refusals_of_the_library(hip):
    from sparsearray_amd import SparseArrayError
    x = lc.specials_operand("double").svt()
    ones = np.ones(1)
    with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains out-of-bound indices"):
        hip.SparseArray_Call("C_subassign_SVT_by_Lindex", x, np.array([1, 37 * 23 + 1], dtype=np.int64), ones)
    with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains NAs"):
        hip.SparseArray_Call("C_subassign_SVT_by_Lindex", x, np.array([1, lc.LINDEX_NA], dtype=np.int64), ones)
    with pytest.raises(SparseArrayError, match="linear index \\(L-index\\) contains out-of-bound indices"):
        hip.SparseArray_Call("C_subset_SVT_by_Lindex", x, np.array([0], dtype=np.int64))
    with pytest.raises(SparseArrayError, match="matrix subscript \\(M-index\\) contains out-of-bound indices"):
        hip.SparseArray_Call("C_subset_SVT_by_Mindex", x, np.array([[1, 24]], dtype=np.int32))
    with pytest.raises(SparseArrayError, match="matrix subscript \\(M-index\\) contains NAs"):
        hip.SparseArray_Call("C_subassign_SVT_by_Mindex", x, np.array([[int(lc.NA_integer), 1]], dtype=np.int32), ones)
