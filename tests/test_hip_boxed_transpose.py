"""The boxed driver of the device transposition (kernels_transpose.hip, launch_transpose_boxed) at mid size: with
the box limit forced small (svt_dev_set_box_nnz) every operand of more nonzeros than the limit is cut into boxes of
consecutive columns, each transposed by the unboxed routes and placed.  The result must be bit for bit the unboxed
one; boxed_calls() proves which path ran."""
import numpy as np
import pytest

from helpers import check_case, golden_cases

pytestmark = pytest.mark.gpu

LIMITS = [257, 4096, 100000]


def _torch():
    import torch
    return torch


def _operand(nrow, lens, kind, seed, long_col=None):
    """Columns of the given lengths, rows drawn without replacement and sorted (the SVT leaf order)."""
    from sparsearray_amd import device
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.asarray(lens, np.int64), nrow)
    if long_col is not None:
        lens[long_col[0]] = min(long_col[1], nrow)
    cp = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=cp[1:])
    ri = np.empty(int(cp[-1]), np.int32)
    for j, n in enumerate(lens):
        if n:
            ri[cp[j]:cp[j + 1]] = np.sort(rng.choice(nrow, int(n), replace=False))
    nnz = len(ri)
    if kind == "double":
        val = rng.standard_normal(nnz)
        val[::7] = -np.abs(val[::7])
    elif kind == "int":
        val = rng.integers(-1000, 1000, nnz).astype(np.int32)
        val[val == 0] = 7
    else:                                                # logical: TRUE, with some NA
        val = np.ones(nnz, np.int32)
        val[::11] = np.iinfo(np.int32).min
    torch = _torch()
    return device.DeviceCSC(nrow, torch.as_tensor(cp, device="cuda"), torch.as_tensor(ri, device="cuda"),
                            torch.as_tensor(val, device="cuda"), logical=kind == "logical"), nnz


def _bits(t):
    torch = _torch()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    torch = _torch()
    assert a.nrow == b.nrow and a.ncol == b.ncol and a.nnz == b.nnz and a.Rtype == b.Rtype
    assert torch.equal(a.col_ptr, b.col_ptr)
    assert torch.equal(a.row_idx, b.row_idx)
    assert torch.equal(_bits(a.val), _bits(b.val))


def _forced_t(A, limit):
    """(unforced t(A), forced t(A), boxed calls of the forced call, route count deltas of the forced call)"""
    from sparsearray_amd import device
    torch = _torch()
    device.set_box_nnz(0)
    c0 = device.boxed_calls()
    ref = A.t()
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0, "an unforced call took the boxed driver"
    r0 = device.aperm_route_counts()
    try:
        device.set_box_nnz(limit)
        got = A.t()
        torch.cuda.synchronize()
    finally:
        device.set_box_nnz(0)
    r1 = device.aperm_route_counts()
    return ref, got, device.boxed_calls() - c0, {k: r1[k] - r0[k] for k in r0}


SHAPES = {
    # name: (nrow, column lengths, long column)
    "random": (700, lambda rng: rng.integers(0, 120, 900), None),
    "empty_columns": (500, lambda rng: np.where(rng.random(3000) < 0.8, 0, rng.integers(1, 60, 3000)), None),
    "long_column": (5000, lambda rng: rng.integers(0, 20, 400), (123, 4500)),
    "nrow_1": (1, lambda rng: (rng.random(6000) < 0.4).astype(np.int64), None),
    "ncol_1": (9000, lambda rng: np.array([6000]), None),
    "wide_sparse": (300, lambda rng: np.where(rng.random(1_200_000) < 0.002, 1, 0), None),
}


@pytest.mark.parametrize("kind", ["double", "int", "logical"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("limit", LIMITS)
def test_boxed_t_bit_identical(hip, shape, kind, limit):
    nrow, lens_of, long_col = SHAPES[shape]
    lens = lens_of(np.random.default_rng(len(shape)))
    A, nnz = _operand(nrow, lens, kind, seed=limit + len(kind), long_col=long_col)
    ref, got, boxed, _ = _forced_t(A, limit)
    _same(ref, got)
    assert boxed == (1 if nnz > limit else 0)


def test_boxed_t_empty_operand(hip):
    A, nnz = _operand(40, np.zeros(30, np.int64), "double", seed=1)
    assert nnz == 0
    ref, got, boxed, _ = _forced_t(A, 257)
    _same(ref, got)
    assert boxed == 0
    assert int(got.col_ptr.abs().sum()) == 0


@pytest.mark.parametrize("kind", ["double", "int"])
def test_boxed_t_bucketed_route(hip, kind):
    # boxes of 1e5 nonzeros over ~333 columns of 3000 rows: the bucketed route, box after box
    A, nnz = _operand(3000, np.random.default_rng(5).integers(200, 400, 2000), kind, seed=3)
    ref, got, boxed, routes = _forced_t(A, 100000)
    _same(ref, got)
    assert boxed == 1
    assert routes["t_bucketed"] >= nnz // 100000 and routes["t_key_sort"] == 0, routes


@pytest.mark.parametrize("kind", ["double", "int"])
def test_boxed_t_key_sort_route(hip, kind):
    # less than one nonzero per column and coarse bucket: the key sort, box after box
    A, nnz = _operand(50000, np.random.default_rng(6).integers(0, 20, 3000), kind, seed=4)
    ref, got, boxed, routes = _forced_t(A, 4096)
    _same(ref, got)
    assert boxed == 1
    assert routes["t_key_sort"] >= nnz // 4096 and routes["t_bucketed"] == 0, routes


def test_boxed_t_twice_is_identity(hip):
    from sparsearray_amd import device
    A, _ = _operand(800, np.random.default_rng(8).integers(0, 90, 1500), "double", seed=9)
    try:
        device.set_box_nnz(1000)
        tt = A.t().t()
    finally:
        device.set_box_nnz(0)
    _same(A, tt)


def test_boxed_colmedians_of_t(hip):
    from sparsearray_amd import device
    torch = _torch()
    A, _ = _operand(600, np.random.default_rng(10).integers(0, 500, 700), "double", seed=11)
    want = device.colmedians(A.t())
    try:
        device.set_box_nnz(4096)
        c0 = device.boxed_calls()
        got = device.colmedians(A.t())
        torch.cuda.synchronize()
        assert device.boxed_calls() == c0 + 1
    finally:
        device.set_box_nnz(0)
    assert torch.equal(want.view(torch.int64), got.view(torch.int64))


def test_unforced_calls_do_not_box(hip):
    from sparsearray_amd import device
    torch = _torch()
    device.set_box_nnz(0)
    A, _ = _operand(700, np.random.default_rng(12).integers(0, 120, 900), "int", seed=13)
    c0 = device.boxed_calls()
    for _ in range(3):
        A.t()
    device.colmedians(A)
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0


def test_boxed_calls_reset(hip):
    from sparsearray_amd import device
    A, _ = _operand(300, np.random.default_rng(14).integers(0, 50, 200), "int", seed=15)
    try:
        device.set_box_nnz(257)
        A.t()
    finally:
        device.set_box_nnz(0)
    before = device.boxed_calls(reset=True)
    assert before >= 1
    assert device.boxed_calls() == 0


def test_ws_bytes_unchanged_below_threshold(hip):
    """Below the limit the workspace is the unboxed routes' own; the boxed one does not grow with nnz."""
    from sparsearray_amd import device
    lib = device._lib()
    device.set_box_nnz(0)
    small = [lib.svt_dev_transpose_ws_bytes(2000, n) for n in (10, 10**6, 10**8)]
    try:
        device.set_box_nnz(10**8)
        assert [lib.svt_dev_transpose_ws_bytes(2000, n) for n in (10, 10**6, 10**8)] == small
        boxed = [lib.svt_dev_transpose_ws_bytes(2000, n) for n in (2 * 10**8, 10**9, 10**10)]
    finally:
        device.set_box_nnz(0)
    assert max(boxed) < 1.01 * min(boxed)
    # the route's workspace at the box size + the box temporary (12 B per entry) + the rebased col_ptr (<= 2^20 + 1
    # entries) + O(nrow + nnz / box): nothing that grows with nnz
    assert max(boxed) <= small[2] + 12 * 10**8 + 2**25


# ---- host entry points with the limit forced: the golden cases that reach the transposition ----
# (t() and the unary tcrossprod transpose their SVT operand on the device; aperm does not use the transposition)
HOST_CASES = [c for c in golden_cases() if c["fn"] == "t" or (c["fn"] == "tcrossprod" and len(c["args"]) == 1)]


def _clear_resident():
    # the host entry points keep t(x) of a resident operand (keyed by its contents): a t(x) kept by an earlier test
    # would not be transposed again
    from sparsearray_amd import device
    device._lib().svt_resident_clear()


@pytest.mark.parametrize("case", HOST_CASES, ids=[f"{c['id']}-{c['fn']}" for c in HOST_CASES])
def test_host_entry_points_forced(hip, case):
    from helpers import dec
    from sparsearray_amd import device
    x = dec(case["args"][0])
    nnz = int(np.count_nonzero(np.asarray(x.to_dense())))
    _clear_resident()
    try:
        device.set_box_nnz(2)
        c0 = device.boxed_calls()
        check_case(hip, case, lacunar=True, gpu=True)
        moved = device.boxed_calls() - c0
    finally:
        device.set_box_nnz(0)
    if "error" not in case:
        assert (moved >= 1) == (nnz > 2), (nnz, moved)


def test_host_t_forced_boxes(hip):
    from sparsearray_amd import SVT_SparseArray, device
    rng = np.random.default_rng(20)
    d = np.where(rng.random((60, 45)) < 0.3, rng.integers(-9, 9, (60, 45)), 0).astype(np.int32)
    x = SVT_SparseArray.from_dense(d, type="integer")
    _clear_resident()
    try:
        device.set_box_nnz(50)
        c0 = device.boxed_calls()
        tx = hip.t(x)
        assert device.boxed_calls() > c0
    finally:
        device.set_box_nnz(0)
    assert np.array_equal(tx.to_dense(), d.T)


def test_host_rowmedians_and_tcrossprod_forced(hip):
    from sparsearray_amd import SVT_SparseArray, device
    rng = np.random.default_rng(21)
    d = np.where(rng.random((80, 70)) < 0.4, rng.standard_normal((80, 70)), 0.0)
    _clear_resident()
    try:
        device.set_box_nnz(64)
        c0 = device.boxed_calls()
        med = hip.rowMedians(SVT_SparseArray.from_dense(d, type="double"))
        tcp = hip.tcrossprod(SVT_SparseArray.from_dense(d, type="double"))
        assert device.boxed_calls() >= c0 + 2
    finally:
        device.set_box_nnz(0)
    assert np.array_equal(np.asarray(med), np.median(d, axis=1))
    np.testing.assert_allclose(np.asarray(tcp), d @ d.T, rtol=1e-12, atol=1e-12)
