"""Coercion dense array <-> resident operand and nzwhich on the device (kernels_coerce.hip): every case of
tests/coerce_cases.py through DeviceCSC.from_dense, DeviceCSC.to_dense and DeviceCSC.nzwhich against the numpy
expectations, values AS BITS at tolerance 0; the C-contiguous routes; the refusals of the Python surface; determinism; the
workspace contract in an arena of 0xA5 bytes; a malformed operand inside an arena; chains on operands the device made;
and one array past 2^31 cells."""
import ctypes

import numpy as np
import pytest

import coerce_cases as cc
from helpers import Arena
from subset_cases import bits

pytestmark = pytest.mark.gpu

T = cc.T
RTYPE = {"logical": 10, "integer": 13, "double": 14}


@pytest.fixture(scope="module")
def dev(hip):
    import sparsearray_amd.device as d
    assert d.coerce_tile() == T
    return d


def to_torch(a):
    """the numpy array as a CUDA tensor of the same shape in R's layout (column-major), bits kept"""
    import torch
    t = torch.from_numpy(np.array(a.transpose(), order="C", copy=True)).cuda()
    return t.permute(*reversed(range(a.ndim)))


def arrays(R):
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def same_arrays(got, want, what=""):
    for x, y, part in zip(got, want, ("col_ptr", "row_idx", "val")):
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {part} {x.dtype}{x.shape} != {y.dtype}{y.shape}"
        assert np.array_equal(x if x.dtype == np.int64 else bits(x), y if y.dtype == np.int64 else bits(y)), f"{what}: {part}"


def same_dense(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    assert np.array_equal(bits(got), bits(want)), what


def upload(dev, a, type_, na):
    """the expected arrays of (a, type_, na) in the array's own type as a resident operand"""
    import torch
    cp, ri, vv, pos = cc.expected(a, type_, na, type_)
    return dev.DeviceCSC(a.shape[0], *[torch.as_tensor(x, device="cuda") for x in (cp, ri, vv)], logical=type_ == "logical"), pos


# ---------------------------------------------------------------------------
# the three calls on every case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_from_dense(dev, name):
    a, type_, na, ans_type, want = cc.case(name)
    R = dev.DeviceCSC.from_dense(to_torch(a), ans_type=ans_type, na_background=na, logical=type_ == "logical")
    assert (R.nrow, R.ncol, R.Rtype) == (a.shape[0], int(np.prod(a.shape[1:], dtype=np.int64)), RTYPE[ans_type])
    same_arrays(arrays(R), want[:3], name)


@pytest.mark.parametrize("name", cc.NAMES)
def test_to_dense(dev, name):
    a, type_, na, ans_type, _ = cc.case(name)
    X, _ = upload(dev, a, type_, na)
    got = X.to_dense(dim=a.shape, out_type=ans_type, na_background=na)
    assert tuple(got.shape) == a.shape
    same_dense(got, cc.dense_of(a, type_, na, ans_type), name)
    assert int(got.bad.item()) == 0


@pytest.mark.parametrize("name", cc.NAMES)
def test_nzwhich(dev, name):
    a, type_, na, ans_type, _ = cc.case(name)
    X, pos = upload(dev, a, type_, na)
    lin = X.nzwhich(dim=a.shape).cpu().numpy()
    assert lin.dtype == np.int64 and np.array_equal(lin, pos), name
    coo = X.nzwhich(dim=a.shape, arr_ind=True).cpu().numpy()
    want = (np.stack(np.unravel_index(pos, a.shape, order="F"), axis=1) if pos.size else
            np.zeros((0, a.ndim), dtype=np.int64))
    assert coo.dtype == np.int32 and coo.shape == (pos.size, a.ndim) and np.array_equal(coo, want), name


def test_bool_tensor_is_logical(dev):
    import torch
    a = np.random.default_rng(3).random((33, 9)) < 0.4
    R = dev.DeviceCSC.from_dense(to_torch(a))
    assert R.Rtype == RTYPE["logical"]
    same_arrays(arrays(R), cc.expected(a.astype(np.int32), "logical", False, "logical")[:3])


# ---------------------------------------------------------------------------
# the layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["doubles_dense_specials", "nrow_65", "widen_integer_to_double_na", "dim_5_4_3",
                                  "dim_3_4_2_5_na", "widen_logical_to_double_3d"])
def test_c_contiguous_route_gives_the_arrays_of_the_column_major_route(dev, name):
    import torch
    a, type_, na, ans_type, want = cc.case(name)
    t = torch.from_numpy(np.array(a, order="C", copy=True)).cuda()
    assert t.is_contiguous() and not t.permute(*reversed(range(t.ndim))).is_contiguous()
    R = dev.DeviceCSC.from_dense(t, ans_type=ans_type, na_background=na, logical=type_ == "logical")
    assert (R.nrow, R.ncol) == (a.shape[0], int(np.prod(a.shape[1:])))
    same_arrays(arrays(R), want[:3], name)
    same_arrays(arrays(R), arrays(dev.DeviceCSC.from_dense(to_torch(a), ans_type=ans_type, na_background=na,
                                                           logical=type_ == "logical")), name)


def test_other_layouts_and_types_are_refused(dev):
    import torch
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd.api import SparseArrayUnsupported
    t = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(SparseArrayError, match="column-major or C-contiguous"):
        dev.DeviceCSC.from_dense(t[::2, 1:])
    for dtype in (torch.float32, torch.int64, torch.float16):
        with pytest.raises(SparseArrayError, match="logical .bool., integer .int32. or double .float64."):
            dev.DeviceCSC.from_dense(t.to(dtype))
    with pytest.raises(SparseArrayError, match="at least one dimension"):
        dev.DeviceCSC.from_dense(torch.zeros((), dtype=torch.float64, device="cuda"))
    with pytest.raises(SparseArrayError, match="CUDA tensor"):
        dev.DeviceCSC.from_dense(torch.zeros(3, dtype=torch.float64))
    with pytest.raises(SparseArrayUnsupported, match="narrower"):
        dev.DeviceCSC.from_dense(t, ans_type="integer")
    with pytest.raises(SparseArrayError, match="invalid requested type"):
        dev.DeviceCSC.from_dense(t, ans_type="complex")
    X = dev.DeviceCSC.from_dense(t)
    with pytest.raises(SparseArrayUnsupported, match="narrower"):
        X.to_dense(out_type="logical")
    with pytest.raises(SparseArrayError, match="'dim' does not match"):
        X.to_dense(dim=(8, 5))
    with pytest.raises(SparseArrayError, match="'dim' does not match"):
        X.nzwhich(dim=(6, 8))
    for wrong in (torch.empty(47, dtype=torch.float64, device="cuda"), torch.empty(48, dtype=torch.int32, device="cuda"),
                  torch.empty((8, 6), dtype=torch.float64, device="cuda"), torch.empty(96, dtype=torch.float64, device="cuda")[::2],
                  torch.empty(48, dtype=torch.float64)):
        with pytest.raises(SparseArrayError, match="'out' must be a flat contiguous CUDA tensor of 48 elements"):
            X.to_dense(out=wrong)


# ---------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrow_7_3000_leaves", "more_tiles_than_the_grid_na", "nrow_3T_plus_5_2_leaves"])
def test_the_same_calls_twice_give_the_same_bits(dev, name):
    import torch
    a, type_, na, ans_type, _ = cc.case(name)
    t = to_torch(a)
    runs = []
    for _ in range(2):
        R = dev.DeviceCSC.from_dense(t, na_background=na, logical=type_ == "logical")
        runs.append((R, R.to_dense(dim=a.shape, na_background=na), R.nzwhich(dim=a.shape), R.nzwhich(dim=a.shape, arr_ind=True)))
    same_arrays(arrays(runs[0][0]), arrays(runs[1][0]), name)
    for x, y in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(x.contiguous().view(-1).view(torch.int32), y.contiguous().view(-1).view(torch.int32)), name


# ---------------------------------------------------------------------------
# the workspace contract (include/svt_hip.h, "Workspaces"): _count + _fill in an arena with guard bands
# ---------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _two_calls(name, prior):
    """(col_ptr, row_idx, val) of svt_dev_from_dense_count + _fill in an Arena whose workspace held ``prior`` bytes"""
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    a, type_, na, ans_type, (cp, ri, vv, pos) = cc.case(name)
    x = to_torch(a)
    nrow, nleaves, nnz = a.shape[0], cp.size - 1, pos.size
    esz = 8 if ans_type == "double" else 4
    need = lib.svt_dev_from_dense_ws_bytes(a.size)
    arena = Arena([need, 8 * (nleaves + 1), 4 * nnz, esz * nnz])
    arena.part(0)[:] = prior
    got_nnz = ctypes.c_int64(-1)
    ptr = [arena.part(k).data_ptr() if arena.part(k).numel() else None for k in range(4)]
    args = (x.data_ptr() if a.size else None, RTYPE[type_], nrow, nleaves, RTYPE[ans_type], int(na))
    assert lib.svt_dev_from_dense_count(*args, ptr[1], ctypes.byref(got_nnz), ptr[0], need, _stream()) == 0, lib.svt_last_error()
    assert got_nnz.value == nnz
    assert lib.svt_dev_from_dense_fill(*args, ptr[1], ptr[2], ptr[3], ptr[0], need, _stream()) == 0, lib.svt_last_error()
    torch.cuda.synchronize()
    assert arena.guards_intact(), name
    return (arena.part(1, torch.int64).cpu().numpy(), arena.part(2, torch.int32).cpu().numpy(),
            arena.part(3, torch.float64 if esz == 8 else torch.int32).cpu().numpy())


@pytest.mark.parametrize("name", ["all_background", "all_kept", "nrow_1", "nrow_7_3000_leaves_na", "nrow_T_plus_1_3_leaves",
                                  "cells_2T_minus_1_1d", "cells_2T_plus_1_1d_na", "empty_leaves_first_last_and_in_runs",
                                  "dim_0_5", "dim_4_0_3", "widen_integer_to_double"])
def test_workspace_discipline(dev, name):
    want = cc.case(name)[4][:3]
    same_arrays(_two_calls(name, 0xA5), want, name)     # every output cell is written: none of them is 0xA5 by luck
    same_arrays(_two_calls(name, 0x00), want, name + ", workspace of zeros")
    same_arrays(_two_calls(name, 0xFF), want, name + ", workspace of ones")


def test_a_workspace_one_byte_short_is_refused_with_nothing_written(dev):
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    a, type_, na, ans_type, (cp, ri, vv, pos) = cc.case("nrow_7_3000_leaves")
    x = to_torch(a)
    need = lib.svt_dev_from_dense_ws_bytes(a.size)
    arena = Arena([need, 8 * cp.size, 4 * pos.size, 4 * pos.size])
    ptr = [arena.part(k).data_ptr() for k in range(4)]
    nnz = ctypes.c_int64(-7)
    args = (x.data_ptr(), RTYPE[type_], a.shape[0], cp.size - 1, RTYPE[ans_type], 0)
    assert lib.svt_dev_from_dense_count(*args, ptr[1], ctypes.byref(nnz), ptr[0], need - 1, _stream()) < 0
    assert b"workspace too small" in lib.svt_last_error()
    assert lib.svt_dev_from_dense_fill(*args, ptr[1], ptr[2], ptr[3], ptr[0], need - 1, _stream()) < 0
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.untouched()


# ---------------------------------------------------------------------------
# to_dense of an operand that breaks the layout's promises, inside an arena
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("defects", [("row_nrow",), ("row_minus_1",), ("col_ptr_descends",),
                                     ("row_nrow", "row_minus_1", "col_ptr_descends")], ids="+".join)
def test_to_dense_never_follows_a_bad_row_or_pointer(dev, defects):
    """Four leaves of T rows, one tile each.  Leaf 0 ends with a row == nrow, leaf 1 starts with a row == -1, the pointers
    of leaf 3 descend: `bad` goes up, the guard bands stay, and every entry that is in order arrives in its cell."""
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    nrow, ncol = T, 4
    rows = [[5, 77, 4000], [3, 64, 4095], [0, 1, 2], [9, 10]]
    cp = [0, 3, 6, 9, 11]
    if "row_nrow" in defects:
        rows[0][2] = nrow
    if "row_minus_1" in defects:
        rows[1][0] = -1
    if "col_ptr_descends" in defects:
        cp[4] = 8
    ri = np.array([r for leaf in rows for r in leaf], dtype=np.int32)
    vv = np.arange(1, ri.size + 1, dtype=np.float64) * 1.5
    arena = Arena([256, 8 * 5, 4 * ri.size, 8 * ri.size, 8 * nrow * ncol, 4])
    arena.part(1, torch.int64)[:] = torch.as_tensor(cp)
    arena.part(2, torch.int32)[:] = torch.as_tensor(ri)
    arena.part(3, torch.float64)[:] = torch.as_tensor(vv)
    arena.part(5, torch.int32)[:] = 0
    h = lib.svt_wrap_device_csc(RTYPE["double"], nrow, ncol, ri.size, *[arena.part(k).data_ptr() for k in (1, 2, 3)])
    try:
        assert lib.svt_dev_to_dense(h, 0, RTYPE["double"], arena.part(4).data_ptr(), arena.part(5).data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
    finally:
        lib.svt_release(h)
    assert arena.guards_intact()
    assert int(arena.part(5, torch.int32).item()) != 0
    assert torch.equal(arena.part(1, torch.int64).cpu(), torch.as_tensor(cp))           # the operand is only read
    want = np.zeros((nrow, ncol), order="F")
    for q in range(ncol):
        if q == 3 and "col_ptr_descends" in defects:
            continue                                    # nothing is read through these pointers
        for k, r in enumerate(rows[q]):
            if 0 <= r < nrow:
                want[r, q] = vv[cp[q] + k]
    got = arena.part(4, torch.float64).cpu().numpy().reshape((nrow, ncol), order="F")
    same_dense(got, want)


# ---------------------------------------------------------------------------
# chains on operands the device made, against numpy
# ---------------------------------------------------------------------------
def test_chain_from_dense_times_two_log1p_to_dense(dev):
    import arith_cases as ac
    rng = np.random.default_rng(11)
    d = np.where(rng.random((130, 70)) < 0.2, np.round(rng.random((130, 70)) * 9, 3), 0.0)
    got = dev.DeviceCSC.from_dense(to_torch(d)).arith("*", 2.0).math("log1p").to_dense()
    want = np.array([ac.r_log1p(v) for v in (d * 2.0).reshape(-1)]).reshape(d.shape)    # the correctly rounded value
    same_dense(got, want)
    assert np.allclose(want, np.log1p(d * 2.0), rtol=1e-15, atol=0)


def test_chain_subset_to_dense(dev):
    a = cc.case("nrow_65")[0]
    d = cc.dense(a.shape, "double", density=0.4, seed=5)
    X = dev.DeviceCSC.from_dense(to_torch(d))
    rows, cols = np.array([64, 3, 3, 17], dtype=np.int32), np.arange(129, -1, -3, dtype=np.int32)
    same_dense(X.subset(rows, cols).to_dense(), cc.dense_of(d, "double", False, "double")[np.ix_(rows, cols)])


def test_chain_from_dense_of_a_crossprod_result(dev):
    import torch
    rng = np.random.default_rng(12)
    x = np.where(rng.random((300, 40)) < 0.1, rng.integers(-3, 4, (300, 40)), 0).astype(np.float64)
    y = np.where(rng.random((300, 24)) < 0.3, rng.integers(-3, 4, (300, 24)), 0).astype(np.float64)
    X = dev.DeviceCSC.from_dense(to_torch(x))
    Y = to_torch(y)                                     # 300 x 24 column-major: the (24, 300) C-contiguous tensor below
    prod = dev.crossprod_csc_dense(X, Y.t())            # (24, 40) C-contiguous = the column-major 40 x 24 result
    want = x.T @ y                                      # whole numbers: exact whatever the order of the sums
    R = dev.DeviceCSC.from_dense(prod.t())              # the column-major view, read in place
    same_arrays(arrays(R), cc.expected(want, "double", False, "double")[:3], "column-major view")
    Rt = dev.DeviceCSC.from_dense(prod)                 # the C-contiguous tensor: t(want), through t()
    same_arrays(arrays(Rt), cc.expected(np.ascontiguousarray(want.T), "double", False, "double")[:3], "C-contiguous")
    same_dense(R.to_dense(), cc.dense_of(want, "double", False, "double"))
    assert torch.equal(R.to_dense().contiguous(), prod.t().contiguous() + 0.0)


def test_chain_compare_nzwhich(dev):
    d = cc.dense((65, 130), "double", density=0.4, seed=6)
    X = dev.DeviceCSC.from_dense(to_torch(d))
    with np.errstate(invalid="ignore"):
        stored = (d > 0) | np.isnan(d)                  # x > 0 is TRUE or NA where it is stored
    assert np.array_equal(X.compare(">", 0).nzwhich().cpu().numpy(), np.flatnonzero(stored.reshape(-1, order="F")))


# ---------------------------------------------------------------------------
# past 2^31 cells: an int32 array of 65536 x 32769, 8.6 GB; its copy, the masks and torch's temporaries next to it
# ---------------------------------------------------------------------------
def test_past_2e31_cells(dev):
    import torch
    nrow, ncol = 65536, 32769
    n = nrow * ncol
    assert n > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * 4 * n + 6 * 2 ** 30:
        pytest.skip(f"needs {(3 * 4 * n) / 2 ** 30 + 6:.0f} GiB of free device memory, {free / 2 ** 30:.1f} GiB free")
    flat = torch.zeros(n, dtype=torch.int32, device="cuda")
    at = torch.tensor([0, 1, 4095, 4096, nrow - 1, nrow, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, n - nrow + 5, n - 1], device="cuda")
    assert at.unique().numel() == at.numel() and bool((at[1:] > at[:-1]).all())
    flat[at] = torch.arange(1, at.numel() + 1, dtype=torch.int32, device="cuda")
    a = flat.view(ncol, nrow).t()                       # the column-major 65536 x 32769 array
    R = dev.DeviceCSC.from_dense(a)
    assert (R.nrow, R.ncol, R.nnz) == (nrow, ncol, at.numel())
    assert torch.equal(R.nzwhich(), at) and int(R.nzwhich().max()) > 2 ** 31
    assert torch.equal(R.row_idx.to(torch.int64), at % nrow) and torch.equal(R.val, flat[at])
    assert torch.equal(R.col_ptr, torch.searchsorted(at, torch.arange(ncol + 1, device="cuda") * nrow))
    coo = R.nzwhich(arr_ind=True)
    assert torch.equal(coo[:, 0].to(torch.int64), at % nrow) and torch.equal(coo[:, 1].to(torch.int64), at // nrow)
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    back = R.to_dense(out=out)
    assert back.data_ptr() == out.data_ptr() and tuple(back.shape) == (nrow, ncol)
    assert torch.equal(out, flat) and int(back.bad.item()) == 0
    del flat, a, out, back, R
    torch.cuda.empty_cache()
