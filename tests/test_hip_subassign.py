"""Subassignment x[i, j, ...] <- value on the device (kernels_subassign.hip places, kernels_arith.hip merges under the
assign rule): every case of tests/subassign_cases.py through DeviceCSC.subassign on resident operands and through
Session.subassign, values AS BITS and the stored mask at tolerance 0; the count / fill primitives in arenas of poisoned
bytes with guard bands; every status, with the outputs keeping their contents; determinism; and a chain that stays
resident: subset -> arith -> subassign back -> colSums."""
import ctypes

import numpy as np
import pytest

import subassign_cases as sa
from helpers import Arena
from subset_cases import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    import sparsearray_amd.device as d
    assert d.subassign_tile() == sa.P and d.arith_tile() == sa.T
    return d


def to_dev(dev, x):
    cp, ri, vv = x.to_csc()
    A = dev.DeviceCSC.from_host(x.dim[0], cp, ri, vv)
    if x.type == "logical":
        A = dev.DeviceCSC(x.dim[0], A.col_ptr, A.row_idx, A.val, logical=True)
    return A


def to_host(R, dim):
    from sparsearray_amd import SVT_SparseArray
    from sparsearray_amd.svt import LGLSXP, REALSXP
    type_ = "double" if R.Rtype == REALSXP else "logical" if R.Rtype == LGLSXP else "integer"
    assert R.nrow == dim[0] and R.ncol == sa.nleaves_of(dim)
    return SVT_SparseArray.from_csc(tuple(dim), type_, R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy())


def arrays(R):
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def same_arrays(a, b, what=""):
    for x, y, part in zip(a, b, ("col_ptr", "row_idx", "val")):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x) if x.dtype != np.int64 else x,
                                                                             bits(y) if y.dtype != np.int64 else y), f"{what}: {part}"


def device_operands(dev, name):
    """(resident x, rows, leaves, value, logical flag) of a case: 0-based subscripts, None for a whole axis"""
    from sparsearray_amd import SVT_SparseArray
    x, index, value, v_type = sa.case(name)[:4]
    rows = None if index[0] is None else np.asarray(index[0], dtype=np.int32).reshape(-1) - 1
    leaves = sa.leaf_list(x.dim, index)
    if isinstance(value, SVT_SparseArray):
        value = to_dev(dev, value)
    return to_dev(dev, x), rows, leaves, value, v_type == "logical"


def _session_value(value, v_type):
    if v_type == "logical" and isinstance(value, np.ndarray):
        return value != 0
    return value


# ---------------------------------------------------------------------------
# the routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sa.NAMES)
def test_device_route(dev, name):
    X, rows, leaves, value, logical = device_operands(dev, name)
    R = X.subassign(rows, leaves, value, logical=logical)
    sa.check(to_host(R, sa.case(name)[0].dim), name, "DeviceCSC.subassign: ")


@pytest.mark.parametrize("name", sa.NAMES)
def test_session_route(hip, name):
    x, index, value, v_type = sa.case(name)[:4]
    sa.check(hip.subassign(x, _session_value(value, v_type), *index), name, "Session.subassign: ")


@pytest.mark.parametrize("name", ["merged_length_T_plus_1", "patch_leaf_over_400_leaves", "rows_repeated_last_wins",
                                  "svt_put_back_of_subset", "types_integer_vector_double"])
def test_the_same_call_twice_gives_the_same_arrays(dev, name):
    X, rows, leaves, value, logical = device_operands(dev, name)
    same_arrays(arrays(X.subassign(rows, leaves, value, logical=logical)),
                arrays(X.subassign(rows, leaves, value, logical=logical)), name)


def test_session_refusals_of_the_library(hip):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    x = sa.case("rows_reversed")[0]
    v = sa.make((3, 2), "double", np.ones((3, 2), dtype=bool))
    with pytest.raises(SparseArrayUnsupported, match="not strictly increasing, or a leaf is repeated"):
        hip.subassign(x, v, [3, 2, 1], [1, 2])
    with pytest.raises(SparseArrayUnsupported, match="not strictly increasing, or a leaf is repeated"):
        hip.subassign(x, v, [1, 2, 3], [2, 2])
    with pytest.raises(SparseArrayError, match="subscript contains out-of-bound indices or NAs"):
        hip.SparseArray_Call("C_subassign_SVT_with_short_Rvector", x, [np.array([38], dtype=np.int32), None], np.ones(1))


# ---------------------------------------------------------------------------
# the workspace contract (include/svt_hip.h, "Workspaces"): the four primitives in arenas with guard bands
# ---------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _placed_entries(name):
    """how many entries the placed operand Y of a case holds"""
    from sparsearray_amd import SVT_SparseArray
    x, index, value = sa.case(name)[:3]
    if isinstance(value, SVT_SparseArray):
        return value.nzcount()
    sub = sa.index0(x.dim, index)
    last = {}
    for p, r in enumerate(sub[0]):
        last[int(r)] = value[p % len(value)]
    leaves = sa.leaf_list(x.dim, index)
    ncov = len(x.leaves) if leaves is None else len(set(leaves.tolist()))
    return ncov * sum(1 for v in last.values() if v != 0 or v != v)


def _primitives(dev, name, prior):
    """(col_ptr, row_idx, val) of the placement's count + fill and the merge's count + fill, each pair in an Arena whose
    workspace held ``prior`` bytes; the guards of both arenas checked"""
    import torch
    from sparsearray_amd._hip import init
    from sparsearray_amd.svt import REALSXP
    lib = init()
    x, index, value, v_type, new_type, _, want_stored = sa.case(name)
    X, rows, leaves, V, logical = device_operands(dev, name)
    nrow, ncol = X.nrow, X.ncol
    sub = [None if s is None else dev._subscript(s, X.val.device) for s in (rows, leaves)]
    idx = [a for s in sub for a in ((None, -1) if s is None else (s.data_ptr(), s.numel()))]
    if isinstance(V, dev.DeviceCSC):
        what, v_esz, count, fill = (V.handle,), V.val.element_size(), lib.svt_dev_subassign_place_svt_count, \
            lib.svt_dev_subassign_place_svt_fill
    else:
        vals, v_Rtype = dev._assign_values(V, X.val.device, logical)
        what, v_esz, count, fill = (vals.data_ptr(), vals.numel(), v_Rtype), vals.element_size(), \
            lib.svt_dev_subassign_place_vector_count, lib.svt_dev_subassign_place_vector_fill
    y_nnz = _placed_entries(name)
    need = lib.svt_dev_subassign_place_ws_bytes(nrow, ncol)
    a1 = Arena([need, 8 * (ncol + 1), 0 if rows is None else nrow, 0 if leaves is None else ncol, 4 * y_nnz, v_esz * y_nnz])
    a1.part(0)[:] = prior
    p = [_ptr(a1.part(k)) for k in range(6)]
    got = ctypes.c_int64(-1)
    assert count(nrow, ncol, *idx, *what, p[1], p[2], p[3], ctypes.byref(got), p[0], need, _stream()) == 0, lib.svt_last_error()
    assert got.value == y_nnz
    assert fill(nrow, ncol, *idx, *what, p[1], y_nnz, p[4], p[5], p[0], need, _stream()) == 0, lib.svt_last_error()
    torch.cuda.synchronize()
    assert a1.guards_intact(), name + ": the placement"
    for k, s in ((2, rows), (3, leaves)):               # the tables: 1 exactly where the subscript reaches
        if s is not None:
            want = np.zeros(a1.part(k).numel(), dtype=np.uint8)
            want[np.asarray(s)] = 1
            assert np.array_equal(a1.part(k).cpu().numpy(), want), f"{name}: cover table {k - 2}"
    Y = dev.DeviceCSC(nrow, a1.part(1, torch.int64), a1.part(4, torch.int32),
                      a1.part(5, torch.float64 if v_esz == 8 else torch.int32), logical=v_type == "logical")
    nnz = int(want_stored.sum())
    esz = 8 if new_type == "double" else 4
    need2 = lib.svt_dev_arith_merge_ws_bytes(ncol, X.nnz, y_nnz)
    a2 = Arena([need2, 8 * (ncol + 1), 4 * nnz, esz * nnz])
    a2.part(0)[:] = prior
    q = [_ptr(a2.part(k)) for k in range(4)]
    got = ctypes.c_int64(-1)
    assert lib.svt_dev_assign_merge_count(X.handle, Y.handle, p[2], p[3], q[1], ctypes.byref(got), q[0], need2, _stream()) == 0, \
        lib.svt_last_error()
    assert got.value == nnz
    assert lib.svt_dev_assign_merge_fill(X.handle, Y.handle, p[2], p[3], q[1], q[2], q[3], q[0], need2, _stream()) == 0
    torch.cuda.synchronize()
    assert a2.guards_intact() and a1.guards_intact(), name + ": the merge"
    return (a2.part(1, torch.int64).cpu().numpy(), a2.part(2, torch.int32).cpu().numpy(),
            a2.part(3, torch.float64 if esz == 8 else torch.int32).cpu().numpy())


@pytest.mark.parametrize("name", ["merged_length_T", "pair_split_across_a_tile_edge", "300_empty_columns_around_two_full_ones",
                                  "filter_value_zero", "x_without_nonzeros", "patch_leaf_over_400_leaves",
                                  "rows_repeated_last_wins", "types_integer_vector_double", "svt_leaves_reversed",
                                  "svt_whole_axes", "types_double_svt_integer"])
def test_workspace_discipline(dev, name):
    x, index, value, v_type = sa.case(name)[:4]
    want = sa.restate(x, index, value, v_type).to_csc()
    same_arrays(_primitives(dev, name, 0xA5), want, name)      # every output cell is written: none is 0xA5 by luck
    same_arrays(_primitives(dev, name, 0x00), want, name + ", workspace of zeros")
    same_arrays(_primitives(dev, name, 0xFF), want, name + ", workspace of ones")


# ---------------------------------------------------------------------------
# statuses: a non-zero status leaves every output as it was
# ---------------------------------------------------------------------------
def _refused_placement(dev, lib, rows, leaves, value, sign, msg, nrow=37, ncol=23, short=0):
    import re
    import torch
    device = torch.device("cuda")
    sub = [dev._subscript(np.asarray(s, dtype=np.int32), device) for s in (rows, leaves)]
    idx = [a for s in sub for a in (s.data_ptr(), s.numel())]
    need = lib.svt_dev_subassign_place_ws_bytes(nrow, ncol)
    arena = Arena([need, 8 * (ncol + 1), nrow, ncol, 4096, 4096])
    p = [arena.part(k).data_ptr() for k in range(6)]
    nnz = ctypes.c_int64(-7)
    if isinstance(value, dev.DeviceCSC):
        what, count = (value.handle,), lib.svt_dev_subassign_place_svt_count
    else:
        vals, rt = dev._assign_values(value, device)
        what, count = (vals.data_ptr(), vals.numel(), rt), lib.svt_dev_subassign_place_vector_count
    rc = count(nrow, ncol, *idx, *what, p[1], p[2], p[3], ctypes.byref(nnz), p[0], need - short, _stream())
    assert (rc > 0) if sign > 0 else (rc < 0), (rc, lib.svt_last_error())
    assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.guards_intact()
    assert all(bool((arena.part(k) == 0xA5).all()) for k in range(1, 6)), "an output was written on a non-zero status"
    if short:
        assert arena.untouched()


def test_placement_statuses_leave_the_outputs_untouched(dev):
    from sparsearray_amd._hip import init
    lib = init()
    ones = np.ones(1)
    bad = "subscript contains out-of-bound indices or NAs"
    _refused_placement(dev, lib, [0, 37], [1], ones, -1, bad)
    _refused_placement(dev, lib, [0, -1], [1], ones, -1, bad)
    _refused_placement(dev, lib, [0, 1], [23], ones, -1, bad)
    _refused_placement(dev, lib, [0, 1], [5, -2 ** 31], ones, -1, bad)
    _refused_placement(dev, lib, [0, 1], [1], ones, -1, "workspace too small", short=1)
    v = to_dev(dev, sa.make((3, 2), "double", np.ones((3, 2), dtype=bool)))
    order = "not strictly increasing, or a leaf is repeated"
    _refused_placement(dev, lib, [3, 2, 1], [0, 1], v, +1, order)
    _refused_placement(dev, lib, [1, 1, 2], [0, 1], v, +1, order)
    _refused_placement(dev, lib, [1, 2, 3], [4, 4], v, +1, order)
    _refused_placement(dev, lib, [1, 2, 37], [0, 1], v, -1, bad)
    _refused_placement(dev, lib, [1, 2, 3], [0, 23], v, -1, bad)
    _refused_placement(dev, lib, [1, 2, 3], [0, 1], v, -1, "workspace too small", short=1)


def test_composition_statuses(dev):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    X = to_dev(dev, sa.case("rows_reversed")[0])
    with pytest.raises(SparseArrayError, match="out-of-bound"):
        X.subassign([0, 37], None, 1.0)
    with pytest.raises(SparseArrayError, match="out-of-bound"):
        X.subassign(None, [0, 23], 1.0)
    V = to_dev(dev, sa.make((3, 2), "double", np.ones((3, 2), dtype=bool)))
    with pytest.raises(SparseArrayUnsupported, match="not strictly increasing"):
        X.subassign([2, 1, 0], [0, 1], V)
    with pytest.raises(SparseArrayUnsupported, match="repeated"):
        X.subassign([0, 1, 2], [1, 1], V)
    with pytest.raises(SparseArrayError, match="same dimensions"):
        X.subassign([0, 1], [0, 1], V)
    with pytest.raises(SparseArrayError, match="replacement has length zero"):
        X.subassign([0, 1], None, np.zeros(0))
    # an empty selection: a copy that may widen (the one-object case of abind)
    XI = to_dev(dev, sa.case("leaves_repeated")[0])
    R = XI.subassign([], None, 2.5)
    want = sa.widen(sa.case("leaves_repeated")[0].to_dense(), "integer", "double")
    assert np.array_equal(bits(to_host(R, (29, 31)).to_dense()), bits(want))


def test_merge_status_of_a_short_workspace_leaves_the_outputs_untouched(dev):
    from sparsearray_amd._hip import init
    lib = init()
    X, rows, leaves, value, logical = device_operands(dev, "rows_reversed")
    Y, cr, cl = dev.subassign_place(X.nrow, X.ncol, rows, leaves, value)
    need = lib.svt_dev_arith_merge_ws_bytes(X.ncol, X.nnz, Y.nnz)
    arena = Arena([need, 8 * (X.ncol + 1), 4096, 4096])
    p = [arena.part(k).data_ptr() for k in range(4)]
    nnz = ctypes.c_int64(-7)
    assert lib.svt_dev_assign_merge_count(X.handle, Y.handle, cr.data_ptr(), cl.data_ptr(), p[1], ctypes.byref(nnz), p[0],
                                          need - 1, _stream()) < 0
    assert "workspace too small" in lib.svt_last_error().decode()
    assert lib.svt_dev_assign_merge_fill(X.handle, Y.handle, cr.data_ptr(), cl.data_ptr(), p[1], p[2], p[3], p[0], need - 1,
                                         _stream()) < 0
    import torch
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.untouched()
    # and the two-call route gives what the composition gives
    same_arrays(arrays(dev.assign_merge(X, Y, cr, cl)), arrays(X.subassign(rows, leaves, value)), "two calls")


# ---------------------------------------------------------------------------
# a chain that stays resident: take a block, double it on the device, put it back, column sums of the result
# ---------------------------------------------------------------------------
def test_chain_subset_arith_subassign_colsums(dev):
    x, index = sa.case("svt_put_back_of_subset")[:2]
    rows, cols = [np.asarray(s, dtype=np.int32) - 1 for s in index]
    X = to_dev(dev, x)
    block = X.subset(rows, cols)
    back = X.subassign(rows, cols, block)                # the block as subset took it: x again, bit for bit
    same_arrays(arrays(back), arrays(X), "put-back of subset")
    R = X.subassign(rows, cols, block.arith("*", 2.0))
    sa.check(to_host(R, x.dim), "svt_put_back_of_subset_times_2", "chain: ")
    want = sa.case("svt_put_back_of_subset_times_2")[5]
    got = dev.colstats(R, "sum")[0].cpu().numpy().reshape(-1)
    assert np.allclose(got, want.sum(axis=0), rtol=1e-13, atol=0)
    cleared = R.subassign(None, cols, 0.0).subassign(rows, None, 0)      # x[, j] <- 0, then x[i, ] <- 0: the filter twice
    d = want.copy()
    d[:, cols] = 0
    d[rows, :] = 0
    assert np.array_equal(to_host(cleared, x.dim).to_dense(), d) and cleared.nnz == int((d != 0).sum())
