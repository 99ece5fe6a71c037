"""abind / cbind / rbind on the device (kernels_abind.hip): every case of tests/abind_cases.py through Session.abind and
through device.abind on resident operands, against numpy's concatenation of the dense arrays and of the stored masks,
values AS BITS at tolerance 0; more tiles than the copy kernel's grid; determinism; the workspace contract in an arena of
0xA5 bytes; the refusals; and a chain rbind -> cbind -> colSums / crossprod."""
import ctypes

import numpy as np
import pytest

import abind_cases as ab
from helpers import Arena
from subset_cases import bits, same_object

pytestmark = pytest.mark.gpu

T = ab.T


@pytest.fixture(scope="module")
def dev(hip):
    import sparsearray_amd.device as d
    assert d.abind_tile() == T
    return d


def to_dev(dev, x):
    cp, ri, vv = x.to_csc()
    A = dev.DeviceCSC.from_host(x.dim[0], cp, ri, vv)
    if x.type == "logical":
        import torch  # noqa: F401
        A = dev.DeviceCSC(x.dim[0], A.col_ptr, A.row_idx, A.val, logical=True)
    return A


def to_host(R, dim, na_background=False):
    from sparsearray_amd import SVT_SparseArray
    from sparsearray_amd.svt import LGLSXP, REALSXP
    type_ = "double" if R.Rtype == REALSXP else "logical" if R.Rtype == LGLSXP else "integer"
    assert R.nrow == dim[0] and R.ncol == int(np.prod(dim[1:], dtype=np.int64))
    x = SVT_SparseArray.from_csc(tuple(dim), type_, R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy())
    x.na_background = na_background
    return x


def arrays(R):
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def same_arrays(a, b, what=""):
    for x, y, part in zip(a, b, ("col_ptr", "row_idx", "val")):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x) if x.dtype != np.int64 else x,
                                                                             bits(y) if y.dtype != np.int64 else y), f"{what}: {part}"


# ---------------------------------------------------------------------------
# the routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ab.NAMES)
def test_session_route(hip, name):
    along, objects = ab.case(name)[:2]
    res = hip.abind(*objects, along=along)
    if len(objects) == 1:
        assert res is objects[0]
        # the one-object copy of the library itself, which may widen: the entry point under the Session
        res = hip.SparseArray_Call("C_abind_SVT_SparseArray_objects", objects, along, objects[0].type)
    ab.check(res, name, "Session.abind: ")


@pytest.mark.parametrize("name", ab.NAMES)
def test_device_route_gives_the_arrays_of_the_session_route(hip, dev, name):
    along, objects = ab.case(name)[:2]
    dims = ab.padded_dims(name)
    R, new_dim = dev.abind([to_dev(dev, x) for x in objects], along=along, dim=dims)
    res = to_host(R, new_dim, objects[0].na_background)
    ab.check(res, name, "device.abind: ")
    via = hip.SparseArray_Call("C_abind_SVT_SparseArray_objects", [hip._add_missing_dims(x, len(dims[0])) for x in objects],
                               along, res.type)
    same_object(res, via, name)
    same_arrays(arrays(R), via.to_csc(), name)


def test_cbind_and_rbind_of_operands_made_by_subset_and_arith(dev):
    x = ab.obj((60, 40), seed=80, density=0.3)
    X = to_dev(dev, x)
    dense = x.to_dense()
    cols = np.array([39, 0, 0, 17, 5], dtype=np.int32)
    rows = np.arange(3, 50, 2, dtype=np.int32)
    A = X.subset(cols=cols)                             # 60 x 5, the column gather
    B = X.arith("*", 2.0)                               # 60 x 40, the map
    C = X.subset(rows=rows)                             # 24 x 40, the row filter
    got = to_host(dev.cbind(A, B, X), (60, 85)).to_dense()
    assert np.array_equal(bits(got), bits(np.concatenate([dense[:, cols], dense * 2.0, dense], axis=1)))
    got = to_host(dev.rbind(C, B, C), (24 + 60 + 24, 40)).to_dense()
    assert np.array_equal(bits(got), bits(np.concatenate([dense[rows], dense * 2.0, dense[rows]], axis=0)))
    xi = ab.obj((60, 40), "integer", seed=81, density=0.3)
    XI = to_dev(dev, xi)
    got = to_host(dev.rbind(XI.arith("*", 3), X.math("sqrt")), (120, 40)).to_dense()      # integer result + double result
    with np.errstate(invalid="ignore"):
        want = np.concatenate([(xi.to_dense() * 3).astype(np.float64), np.sqrt(dense)], axis=0)
    assert np.array_equal(bits(got), bits(want))


def test_result_is_logical_only_when_every_object_is(dev):
    from sparsearray_amd.svt import INTSXP, LGLSXP
    a, b = to_dev(dev, ab.obj((9, 4), "logical", seed=1)), to_dev(dev, ab.obj((9, 2), "logical", seed=2))
    i = to_dev(dev, ab.obj((9, 3), "integer", seed=3))
    assert dev.cbind(a, b).Rtype == LGLSXP and dev.cbind(a, i, b).Rtype == INTSXP
    gt = i.compare(">", 0)                              # a logical operand made on the device
    assert dev.cbind(gt, a).Rtype == LGLSXP


def test_a_mixed_naarray_pair_is_refused_by_the_library(hip):
    from sparsearray_amd import SparseArrayError
    a, b = ab.obj((5, 3), seed=1), ab.obj((4, 3), seed=2, na_background=True)
    with pytest.raises(SparseArrayError, match="NaArray objects and ordinary objects cannot be bound together"):
        hip.SparseArray_Call("C_abind_SVT_SparseArray_objects", [a, b], 1, "double")
    with pytest.raises(SparseArrayError, match="NaArray objects and ordinary SparseArray objects"):
        hip.rbind(a, b)


def test_host_level_messages_of_the_entry_point(hip):
    from sparsearray_amd import SparseArrayError
    call = lambda *a: hip.SparseArray_Call("C_abind_SVT_SparseArray_objects", *a)        # noqa: E731
    a, b = ab.obj((4, 3, 2), seed=1), ab.obj((4, 3, 2), seed=2)
    for bad in (0, 4):
        with pytest.raises(SparseArrayError, match="'along' must be >= 1 and <= the number of dimensions of the objects to bind"):
            call([a, b], bad, "double")
    with pytest.raises(SparseArrayError, match="all the objects to bind must have the same number of dimensions"):
        call([a, ab.obj((4, 3))], 1, "double")
    with pytest.raises(SparseArrayError, match=r"same extent along dimension 3 \(they are bound along dimension 2\)"):
        call([a, ab.obj((4, 3, 1))], 2, "double")
    with pytest.raises(SparseArrayError, match="narrower"):
        call([a, b], 1, "integer")
    with pytest.raises(SparseArrayError, match="cannot be an empty list"):
        call([], 1, "double")


# ---------------------------------------------------------------------------
# more tiles than the copy kernel's grid: 2 x 4.2 M integer entries, made on the device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(dev):
    import torch
    nrow, ncol = 1050, 4000                             # 2 * 1050 * 4000 entries: 2050.8 tiles of 4096 > the grid of 2048
    objs = []
    for k in range(2):
        cp = torch.arange(ncol + 1, dtype=torch.int64, device="cuda") * nrow
        ri = torch.arange(nrow, dtype=torch.int32, device="cuda").repeat(ncol)
        vv = torch.arange(nrow * ncol, dtype=torch.int32, device="cuda") * (k + 1) - 7
        objs.append(dev.DeviceCSC(nrow, cp, ri, vv))
    assert 2 * nrow * ncol > 2048 * T
    return nrow, ncol, objs


def test_more_tiles_than_the_grid_rows_form(dev, big):
    import torch
    nrow, ncol, (A, B) = big
    R = dev.rbind(A, B)
    assert (R.nrow, R.ncol, R.nnz) == (2 * nrow, ncol, 2 * nrow * ncol)
    assert torch.equal(R.col_ptr, torch.arange(ncol + 1, dtype=torch.int64, device="cuda") * (2 * nrow))
    assert torch.equal(R.row_idx, torch.arange(2 * nrow, dtype=torch.int32, device="cuda").repeat(ncol))
    assert torch.equal(R.val.view(ncol, 2 * nrow), torch.cat([A.val.view(ncol, nrow), B.val.view(ncol, nrow)], dim=1))


def test_more_tiles_than_the_grid_leaf_form(dev, big):
    import torch
    nrow, ncol, (A, B) = big
    R = dev.cbind(A, B)
    assert (R.nrow, R.ncol, R.nnz) == (nrow, 2 * ncol, 2 * nrow * ncol)
    assert torch.equal(R.col_ptr, torch.arange(2 * ncol + 1, dtype=torch.int64, device="cuda") * nrow)
    assert torch.equal(R.row_idx, torch.cat([A.row_idx, B.row_idx])) and torch.equal(R.val, torch.cat([A.val, B.val]))


# ---------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows_nnz_2T_plus_1", "cbind_300_empty_columns_inside_a_tile", "types_logical_integer_double_rows"])
def test_the_same_call_twice_gives_the_same_arrays(dev, name):
    along, objects = ab.case(name)[:2]
    D = [to_dev(dev, x) for x in objects]
    first = arrays(dev.abind(D, along=along, dim=ab.padded_dims(name))[0])
    same_arrays(first, arrays(dev.abind(D, along=along, dim=ab.padded_dims(name))[0]), name)


# ---------------------------------------------------------------------------
# the workspace contract (include/svt_hip.h, "Workspaces"): _count + _fill in an arena with guard bands
# ---------------------------------------------------------------------------
def _two_calls(dev, name, prior):
    """(col_ptr, row_idx, val) of svt_dev_abind_count + _fill in an Arena whose workspace held ``prior`` bytes"""
    import torch
    from sparsearray_amd._hip import init
    from sparsearray_amd.svt import REALSXP
    lib = init()
    along, objects, ans_type, want, want_stored = ab.case(name)
    dims = ab.padded_dims(name)
    D = [to_dev(dev, x) for x in objects]
    _, handles, inner, ext, ans_Rtype, new_dim = dev._abind_operands(D, along, dims)
    nleaves = int(np.prod(new_dim[1:], dtype=np.int64))
    nnz = int(want_stored.sum())
    esz = 8 if ans_Rtype == REALSXP else 4
    need = lib.svt_dev_abind_ws_bytes(len(D), nleaves, int(ext is None))
    arena = Arena([need, 8 * (nleaves + 1), 4 * nnz, esz * nnz])
    arena.part(0)[:] = prior
    got_nnz = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = [arena.part(k).data_ptr() if arena.part(k).numel() else None for k in range(4)]
    assert lib.svt_dev_abind_count(handles, len(D), inner, ext, ans_Rtype, ptr[1], ctypes.byref(got_nnz), ptr[0], need,
                                   stream) == 0, lib.svt_last_error()
    assert got_nnz.value == nnz
    assert lib.svt_dev_abind_fill(handles, len(D), inner, ext, ans_Rtype, ptr[1], ptr[2], ptr[3], ptr[0], need, stream) == 0
    torch.cuda.synchronize()
    assert arena.guards_intact(), name
    return (arena.part(1, torch.int64).cpu().numpy(), arena.part(2, torch.int32).cpu().numpy(),
            arena.part(3, torch.float64 if esz == 8 else torch.int32).cpu().numpy())


@pytest.mark.parametrize("name", ["rows_all_empty", "rows_nnz_T", "rows_nnz_2T_plus_1", "rows_300_empty_leaves_inside_a_tile",
                                  "cbind_piece_on_the_tile_boundary", "types_logical_integer_double_cols"])
def test_workspace_discipline(hip, dev, name):
    along, objects, ans_type = ab.case(name)[:3]
    ndim = len(ab.padded_dims(name)[0])
    want = ab.restate([hip._add_missing_dims(x, ndim) for x in objects], along, ans_type).to_csc()
    got = _two_calls(dev, name, 0xA5)
    same_arrays(got, want, name)                        # every output cell is written: none of them is 0xA5 by luck
    same_arrays(_two_calls(dev, name, 0x00), want, name + ", workspace of zeros")
    same_arrays(_two_calls(dev, name, 0xFF), want, name + ", workspace of ones")


# ---------------------------------------------------------------------------
# refusals: answered on the host, nothing is launched and nothing outside ws is written (nor inside it)
# ---------------------------------------------------------------------------
def _refused(lib, arena, table, n, inner, ext, ans, msg, ws_bytes=None):
    import re
    import torch
    e = None if ext is None else (ctypes.c_int64 * len(ext))(*ext)
    nnz = ctypes.c_int64(-7)
    ws, cp, ri, vv = [arena.part(k).data_ptr() for k in range(4)]
    ws_bytes = arena.part(0).numel() if ws_bytes is None else ws_bytes
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.svt_dev_abind_count(table, n, inner, e, ans, cp, ctypes.byref(nnz), ws, ws_bytes, stream) < 0
    assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
    assert lib.svt_dev_abind_fill(table, n, inner, e, ans, cp, ri, vv, ws, ws_bytes, stream) < 0
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.untouched()


@pytest.mark.parametrize("what,specs,nobj,inner,ext,ans,msg", ab.REFUSALS, ids=[r[0] for r in ab.REFUSALS])
def test_refusals_leave_everything_untouched(dev, what, specs, nobj, inner, ext, ans, msg):
    from sparsearray_amd._hip import init
    lib = init()
    hs, table = ab.bare_handles(lib, specs)
    try:
        _refused(lib, Arena([1 << 16, 256, 256, 256]), table, len(hs) if nobj is None else nobj, inner, ext, ans, msg)
    finally:
        for h in hs:
            lib.svt_release(h)


def test_null_object_mixed_background_and_small_workspace_are_refused(dev):
    from sparsearray_amd._hip import init
    from sparsearray_amd.svt import REALSXP
    lib = init()
    D = [to_dev(dev, x) for x in ab.case("rows_5_and_7")[1]]
    table = (ctypes.c_void_p * 2)(*[d._h for d in D])
    arena = Arena([1 << 16, 256, 4096, 4096])
    _refused(lib, arena, (ctypes.c_void_p * 2)(D[0]._h, None), 2, 1, None, REALSXP, "object 2 is NULL")
    _refused(lib, arena, table, 2, 1, None, REALSXP, "workspace too small", ws_bytes=lib.svt_dev_abind_ws_bytes(2, 3, 1) - 1)
    na = ctypes.c_int32.from_address(D[1]._h + 56)      # struct svt_dev_csc: na_background follows the three pointers
    na.value = 1
    try:
        _refused(lib, arena, table, 2, 1, None, REALSXP, "NaArray objects and ordinary objects")
    finally:
        na.value = 0


# ---------------------------------------------------------------------------
# a chain: rbind the row halves of each column half, cbind the two; then statistics and a product on the result
# ---------------------------------------------------------------------------
def test_chain_split_and_bind_back_then_colsums_and_crossprod(dev):
    import torch
    x = ab.obj((300, 90), seed=90, density=0.2, palette="specials")
    X = to_dev(dev, x)
    r_top, r_bot = np.arange(0, 140, dtype=np.int32), np.arange(140, 300, dtype=np.int32)
    c_left, c_right = np.arange(0, 37, dtype=np.int32), np.arange(37, 90, dtype=np.int32)
    halves = []
    for cols in (c_left, c_right):
        top, bot = X.subset(rows=r_top, cols=cols), X.subset(rows=r_bot, cols=cols)
        halves.append(dev.rbind(top, bot))
        same_arrays(arrays(halves[-1]), arrays(X.subset(cols=cols)), "rbind of the row halves")
    R = dev.cbind(*halves)
    same_arrays(arrays(R), arrays(X), "cbind of the column halves")
    assert (R.nrow, R.ncol, R.nnz) == (X.nrow, X.ncol, X.nnz)
    # the statistics and the product on the same chain over a tracer operand: whole numbers below 2^15 against whole
    # numbers in -3 .. 3, so that every sum is exact in double whatever its order and "equal" means equal
    y = ab.obj((300, 90), seed=91, density=0.2)
    Y = to_dev(dev, y)
    Rb = dev.cbind(*[dev.rbind(Y.subset(rows=r_top, cols=c), Y.subset(rows=r_bot, cols=c)) for c in (c_left, c_right)])
    same_arrays(arrays(Rb), arrays(Y), "the tracer operand")
    sums = dev.colstats(Rb, "sum")[0]
    assert torch.equal(sums, dev.colstats(Y, "sum")[0])
    assert np.array_equal(sums.cpu().numpy(), y.to_dense().sum(axis=0))
    d = np.random.default_rng(5).integers(-3, 4, (8, 300)).astype(np.float64)
    dense = torch.as_tensor(d, device="cuda")
    prod = dev.crossprod_csc_dense(Rb, dense)
    assert torch.equal(prod, dev.crossprod_csc_dense(Y, dense))
    assert np.array_equal(prod.cpu().numpy(), d @ y.to_dense())
