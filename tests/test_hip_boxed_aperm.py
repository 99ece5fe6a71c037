"""The boxed driver of the device aperm for permutations that move the rows (kernels_transpose.hip,
launch_aperm_boxed) at mid size: with the box limit forced small (svt_dev_set_box_nnz) every such operand of more
nonzeros than the limit is cut into boxes -- ranges of indices of the old axis that becomes the rows --, each gathered,
permuted by the unboxed routes and placed.  The result must be bit for bit the unboxed one, and equal numpy's transpose
of the dense array; boxed_calls() proves which path ran."""
import itertools

import numpy as np
import pytest

from helpers import check_case, golden_cases

pytestmark = pytest.mark.gpu

LIMITS = [257, 4096, 100000]
KINDS = ["double", "int", "logical"]
NA_INT = np.iinfo(np.int32).min


def _torch():
    import torch
    return torch


def _dense(dim, nnz, kind, seed, shape_fn=None):
    """A dense array (Fortran order) of `nnz` nonzeros at random cells; shape_fn(a) may zero parts of it."""
    rng = np.random.default_rng(seed)
    a = np.zeros(dim, dtype=np.float64 if kind == "double" else np.int32, order="F")
    flat = a.reshape(-1, order="F")
    assert np.shares_memory(flat, a)
    if nnz:
        idx = rng.choice(a.size, size=nnz, replace=False)
        if kind == "double":
            v = rng.standard_normal(nnz)
            v[v == 0] = 1.5
            v[::7] = -np.abs(v[::7])
        elif kind == "int":
            v = rng.integers(-1000, 1000, nnz).astype(np.int32)
            v[v == 0] = 7
        else:                                            # logical: TRUE, with some NA
            v = np.ones(nnz, np.int32)
            v[::11] = NA_INT
        flat[idx] = v
    if shape_fn is not None:
        shape_fn(a)
    return a


def _csc(a):
    """(col_ptr, row_idx, val) of a dense array in the SVT leaf order: leaves by the outer axes, rows ascending."""
    flat = a.reshape(-1, order="F")
    nz = np.flatnonzero(flat)
    d0 = a.shape[0]
    nleaves = a.size // d0 if d0 else 0
    cp = np.zeros(nleaves + 1, np.int64)
    if nz.size:
        np.cumsum(np.bincount(nz // d0, minlength=nleaves), out=cp[1:])
    return cp, (nz % max(d0, 1)).astype(np.int32), flat[nz]


def _dev(a, kind):
    from sparsearray_amd import device
    torch = _torch()
    cp, ri, v = _csc(a)
    return device.DeviceCSC(a.shape[0], torch.as_tensor(cp, device="cuda"), torch.as_tensor(ri, device="cuda"),
                            torch.as_tensor(v, device="cuda"), logical=kind == "logical"), len(ri)


def _bits(t):
    torch = _torch()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    torch = _torch()
    assert a.nrow == b.nrow and a.ncol == b.ncol and a.nnz == b.nnz and a.Rtype == b.Rtype
    assert torch.equal(a.col_ptr, b.col_ptr)
    assert torch.equal(a.row_idx, b.row_idx)
    assert torch.equal(_bits(a.val), _bits(b.val))


def _same_as_numpy(T, new_dim, a, perm):
    want = np.transpose(a, [p - 1 for p in perm])
    assert tuple(new_dim) == want.shape
    wcp, wri, wv = _csc(want)
    assert np.array_equal(T.col_ptr.cpu().numpy(), wcp)
    assert np.array_equal(T.row_idx.cpu().numpy(), wri)
    got = T.val.cpu().numpy()
    assert got.dtype == wv.dtype
    assert np.array_equal(got.view(np.int64 if got.dtype == np.float64 else np.int32),
                          wv.view(np.int64 if wv.dtype == np.float64 else np.int32))


def _forced_aperm(A, dim, perm, limit):
    """(unforced result, forced result, new dim, boxed calls of the forced call)"""
    from sparsearray_amd import device
    torch = _torch()
    device.set_box_nnz(0)
    c0 = device.boxed_calls()
    ref, _ = A.aperm(dim, perm)
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0, "an unforced call took the boxed driver"
    try:
        device.set_box_nnz(limit)
        got, new_dim = A.aperm(dim, perm)
        torch.cuda.synchronize()
    finally:
        device.set_box_nnz(0)
    return ref, got, new_dim, device.boxed_calls() - c0


def _one_index_of_axis_2(a):
    keep = a[:, 7, :].copy()
    a[...] = 0
    a[:, 7, :] = keep


def _empty_slabs(a):
    a[:, :, 5] = 0
    a[:, 3, :] = 0
    a[:, :, 22] = 0


ROW_MOVING_3D = [(2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]

# name: (dim, nonzeros before shape_fn, permutations, shape_fn)
SHAPES = {
    # every row-moving permutation of a 3-d array: q = 2 (not outermost) and q = 3 (outermost); key sort / slab form
    "d3": ((700, 40, 23), 20000, ROW_MOVING_3D, None),
    # the first two axes swapped: the batched bucketed transposition inside the boxes
    "swap01": ((5000, 300, 7), 900_000, [(2, 1, 3)], None),
    "slab": ((900, 30, 16), 40000, [(3, 1, 2)], None),
    # the 4-d / 5-d general permutations of test_device_aperm_general_permutations
    "g4a": ((1500, 900, 4, 3), 1_500_000, [(2, 4, 1, 3), (3, 1, 4, 2)], None),
    "g4b": ((1500, 4, 900, 3), 1_500_000, [(3, 2, 4, 1), (3, 4, 2, 1)], None),
    "g5": ((1200, 5, 3, 700, 2), 1_200_000, [(4, 5, 1, 3, 2), (4, 1, 2, 3, 5)], None),
    "g4c": ((300, 6, 5, 4), 9000, [(2, 4, 3, 1), (4, 3, 2, 1)], None),
    "g5b": ((40, 30, 20, 10, 3), 50_000, [(5, 3, 1, 4, 2)], None),
    "d2": ((300, 500), 20000, [(2, 1)], None),
    # a unit extent on the axis that becomes the rows: one box of one index, over the limit
    "unit_q_outer": ((64, 50, 1), 1500, [(3, 1, 2), (3, 2, 1)], None),
    "unit_q_inner": ((50, 1, 40), 1200, [(2, 1, 3), (2, 3, 1)], None),
    "unit_rows": ((1, 60, 45), 1500, ROW_MOVING_3D, None),
    # all nonzeros on one index of axis 2: a single-index box over the limit
    "one_index": ((200, 30, 20), 50000, [(2, 1, 3), (2, 3, 1)], _one_index_of_axis_2),
    "empty_slabs": ((700, 40, 23), 30000, ROW_MOVING_3D, _empty_slabs),
    "empty": ((900, 30, 16), 0, [(3, 1, 2), (2, 1, 3)], None),
}

_cache = {}


def _operand(shape, kind):
    """The operand of a shape and element type, kept for the consecutive cases that use it."""
    key = (shape, kind)
    if _cache.get("key") != key:
        _cache.clear()
        dim, nnz, _, fn = SHAPES[shape]
        a = _dense(dim, nnz, kind, seed=len(shape) * 31 + len(kind), shape_fn=fn)
        A, n = _dev(a, kind)
        _cache.update(key=key, a=a, A=A, nnz=n)
    return _cache["a"], _cache["A"], _cache["nnz"]


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_boxed_aperm_bit_identical(hip, shape, kind, limit):
    dim, _, perms, _ = SHAPES[shape]
    a, A, nnz = _operand(shape, kind)
    if shape == "one_index":
        assert nnz > 1000 and np.count_nonzero(a[:, 7, :]) == nnz
    for perm in perms:
        ref, got, new_dim, boxed = _forced_aperm(A, dim, perm, limit)
        _same(ref, got)
        _same_as_numpy(got, new_dim, a, perm)
        assert boxed == (1 if nnz > limit else 0), (perm, nnz, boxed)


@pytest.mark.parametrize("limit", LIMITS)
def test_leaf_preserving_permutations_are_not_boxed(hip, limit):
    from sparsearray_amd import device
    torch = _torch()
    for dim, perm in (((700, 40, 23), (1, 3, 2)), ((300, 6, 5, 4), (1, 3, 2, 4)), ((300, 6, 5, 4), (1, 4, 2, 3))):
        a = _dense(dim, 20000, "double", seed=3)
        A, nnz = _dev(a, "double")
        ref, got, new_dim, boxed = _forced_aperm(A, dim, perm, limit)
        _same(ref, got)
        _same_as_numpy(got, new_dim, a, perm)
        assert boxed == 0
        del A
    torch.cuda.synchronize()


def test_unforced_calls_do_not_box(hip):
    from sparsearray_amd import device
    torch = _torch()
    device.set_box_nnz(0)
    a = _dense((700, 40, 23), 20000, "int", seed=5)
    A, _ = _dev(a, "int")
    c0 = device.boxed_calls()
    for perm in itertools.permutations((1, 2, 3)):
        A.aperm((700, 40, 23), perm)
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0


@pytest.mark.parametrize("dim,perm", [
    ((700, 40, 23), (2, 3, 1)), ((700, 40, 23), (3, 2, 1)), ((300, 6, 5, 4), (3, 4, 1, 2)),
    ((40, 30, 20, 10, 3), (5, 3, 1, 4, 2)),
])
def test_boxed_aperm_round_trip(hip, dim, perm):
    """aperm(aperm(x, p), p^-1) == x with both calls boxed"""
    from sparsearray_amd import device
    a = _dense(dim, 20000, "double", seed=7)
    A, nnz = _dev(a, "double")
    inv = tuple(int(i) + 1 for i in np.argsort(perm))
    try:
        device.set_box_nnz(1000)
        c0 = device.boxed_calls()
        B, bdim = A.aperm(dim, perm)
        C, cdim = B.aperm(bdim, inv)
        _torch().cuda.synchronize()
        assert device.boxed_calls() == c0 + 2
    finally:
        device.set_box_nnz(0)
    assert tuple(cdim) == tuple(dim)
    _same(A, C)


def _ws(lib, nnz, dim):
    d = np.asarray(dim, np.int64)
    return lib.svt_dev_aperm_ws_bytes(nnz, len(d), d.ctypes.data)


def _ws_perm(lib, nnz, dim, perm):
    d, p = np.asarray(dim, np.int64), np.asarray(perm, np.int32)
    return lib.svt_dev_aperm_perm_ws_bytes(nnz, len(d), d.ctypes.data, p.ctypes.data)


def test_ws_bytes_unchanged_below_threshold(hip):
    """Below the limit the workspace is the unboxed routes' own; the boxed one does not grow with nnz; the need of
    one permutation never exceeds that of all."""
    from sparsearray_amd import device
    lib = device._lib()
    dim = (2000, 300, 50)
    device.set_box_nnz(0)
    small = [_ws(lib, n, dim) for n in (10, 10**6, 10**8)]
    small_perm = [_ws_perm(lib, n, dim, (2, 1, 3)) for n in (10, 10**6, 10**8)]
    assert small_perm == small                           # the driver not taken: one value for both functions
    try:
        device.set_box_nnz(10**8)
        assert [_ws(lib, n, dim) for n in (10, 10**6, 10**8)] == small
        boxed = [_ws(lib, n, dim) for n in (2 * 10**8, 10**9, 10**10)]
        for shape in (dim, (40, 30000, 7)):
            for n in (10**6, 2 * 10**8, 10**10):
                every = _ws(lib, n, shape)
                for perm in itertools.permutations((1, 2, 3)):
                    assert _ws_perm(lib, n, shape, perm) <= every, (shape, n, perm)
        # leaf-preserving past the limit: the scratch of one scan over 15000 leaf counts
        assert _ws_perm(lib, 10**10, dim, (1, 3, 2)) < 2**20
    finally:
        device.set_box_nnz(0)
    assert max(boxed) < 1.01 * min(boxed)
    # with no limit set the driver starts at 2^31 nonzeros: below it the value still grows with nnz, past it not
    assert _ws(lib, 2**31 - 1, dim) > small[2]
    big = [_ws(lib, n, dim) for n in (2**31, 10**10, 10**11)]
    assert max(big) < 1.01 * min(big)


def test_workspace_too_small_is_an_error(hip):
    """A boxed call checks its workspace against the permutation's own need before it writes anything."""
    from sparsearray_amd import SparseArrayError, device
    torch = _torch()
    dim, perm = (700, 40, 23), (2, 3, 1)
    a = _dense(dim, 20000, "double", seed=9)
    A, nnz = _dev(a, "double")
    lib = device._lib()
    d, p = np.asarray(dim, np.int64), np.asarray(perm, np.int32)
    cp = torch.empty(23 * 700 + 1, dtype=torch.int64, device="cuda")
    ri = torch.empty(nnz, dtype=torch.int32, device="cuda")
    vv = torch.empty(nnz, dtype=torch.float64, device="cuda")
    try:
        device.set_box_nnz(1000)
        need = _ws_perm(lib, nnz, dim, perm)
        ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
        rc = lib.svt_dev_aperm(A.handle, 3, d.ctypes.data, p.ctypes.data, cp.data_ptr(), ri.data_ptr(), vv.data_ptr(),
                               ws.data_ptr(), ws.numel(), device._stream())
        assert rc < 0 and b"workspace too small" in lib.svt_last_error()
        with pytest.raises(SparseArrayError):
            device._check(rc)
    finally:
        device.set_box_nnz(0)


# ---- host entry points with the limit forced ----
HOST_CASES = [c for c in golden_cases() if c["fn"] == "aperm"]


@pytest.mark.parametrize("case", HOST_CASES, ids=[str(c["id"]) for c in HOST_CASES])
def test_host_aperm_forced(hip, case):
    from helpers import dec
    from sparsearray_amd import device
    x = dec(case["args"][0])
    nnz = int(np.count_nonzero(np.asarray(x.to_dense())))
    perm = case["kwargs"].get("perm") or list(range(x.ndim, 0, -1))
    try:
        device.set_box_nnz(2)
        c0 = device.boxed_calls()
        check_case(hip, case, lacunar=True, gpu=True)
        moved = device.boxed_calls() - c0
    finally:
        device.set_box_nnz(0)
    assert moved == (1 if perm[0] != 1 and nnz > 2 else 0), (perm, nnz, moved)


def test_host_aperm_forced_boxes(hip):
    from sparsearray_amd import SVT_SparseArray, device
    rng = np.random.default_rng(20)
    d = np.where(rng.random((60, 45, 12)) < 0.3, rng.integers(-9, 9, (60, 45, 12)), 0).astype(np.int32)
    x = SVT_SparseArray.from_dense(np.asfortranarray(d), type="integer")
    for perm in ((2, 1, 3), (3, 1, 2), (2, 3, 1), (3, 2, 1), (1, 3, 2)):
        try:
            device.set_box_nnz(50)
            c0 = device.boxed_calls()
            tx = hip.aperm(x, perm)
            assert device.boxed_calls() - c0 == (1 if perm[0] != 1 else 0)
        finally:
            device.set_box_nnz(0)
        assert np.array_equal(tx.to_dense(), np.transpose(d, [p - 1 for p in perm])), perm
