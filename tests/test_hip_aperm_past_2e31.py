"""Device aperm() with permutations that move the rows on an operand past 2^31 nonzeros: the closed-form operand of
test_hip_past_2e31.py (2 274 460 118 nonzeros) as the 3-d array A of extents (32768, 1120, 1000), column j of the
matrix being leaf (j1, j2) with j = j1 + 1120 j2.  A slice along axis 2 holds 2.00e6 to 3.23e6 nonzeros, one along
axis 3 2.27e6 to 2.30e6, and every permuted array has 3.3e7 or 3.7e7 leaves: no remaining limit is met and every box
(2^28 nonzeros at most by default) is far from a single-index one.
Peak device memory: the round trip aperm(B, c(2,1,3)) while A, B, the result (3 x 18.2 GB of entries, 0.3 GB of leaf
pointers each for B and C) and the boxed driver's workspace (19.0 GiB for q = 2, 16.0 GiB for q = 3) are alive = ~76 GB
(71 GiB), plus torch's own temporaries of the checks (below 3 GiB); the tests skip when less than that and a margin is
free."""
import numpy as np
import pytest

from test_hip_past_2e31 import NCOL, R, S, _build, _lengths, _same_as_closed_form

pytestmark = pytest.mark.gpu

D1, D2 = 1120, 1000
DIM = (R, D1, D2)
PEAK = 74 * 2**30
POS_CHUNK = 1 << 27


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def big(hip):
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < PEAK + 6 * 2**30:
        pytest.skip(f"needs {PEAK / 2**30 + 6:.0f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    A, cp, nnz = _build(torch)
    assert nnz == 2_274_460_118 and D1 * D2 == NCOL
    yield A, cp, nnz
    del A, cp
    torch.cuda.empty_cache()


def _well_formed(torch, T, nnz):
    """pointers from 0 to nnz, never decreasing; row indices strictly ascending inside every leaf (all entries)"""
    op = T.col_ptr
    assert int(op[0]) == 0 and int(op[-1]) == nnz
    assert bool(torch.all(op[1:] >= op[:-1]))
    for p0 in range(0, nnz, POS_CHUNK):
        p1 = min(p0 + POS_CHUNK + 1, nnz)               # (one entry of overlap: the pair across the chunk's end)
        r = T.row_idx[p0:p1]
        up = r[1:] > r[:-1]
        lo, hi = torch.searchsorted(op, torch.tensor([p0 + 1, p1], device="cuda")).tolist()
        starts = op[lo:hi] - (p0 + 1)                   # pairs (k, k + 1) whose second entry opens a leaf
        up[starts[(starts >= 0) & (starts < up.numel())]] = True
        assert bool(torch.all(up)), f"row indices of positions {p0}..{p1}"
        del r, up, starts
    assert 0 <= int(T.row_idx.min()) and int(T.row_idx.max()) < T.nrow


def _leaf_from_closed_form(torch, r, j):
    """Of the columns j (int64 tensor) of the matrix, those with a nonzero at row r: (mask, values)"""
    L = _lengths(torch, j)
    dense = j % 1000 == 0
    hit = dense | (((5 * j) % S == r % S) & (r // S < L))
    k = torch.where(dense, torch.full_like(j, r), torch.full_like(j, r // S))
    v = (31 * j + 17 * k) % 2001 - 1000
    v = torch.where(v == 0, torch.full_like(v, 1001), v)
    return hit, v


def _sampled_leaves(torch, T, nleaves_per_r, column_of, seed):
    """64 sampled leaves (r, o) of T plus the first and the last against the closed form: leaf r + R * o holds, for
    every index t of the axis that became the rows with A[r, column_of(t, o)] != 0, the entry (t, value)."""
    gen = torch.Generator().manual_seed(seed)
    rs = torch.randint(0, R, (64,), generator=gen).tolist() + [0, R - 1]
    os_ = torch.randint(0, nleaves_per_r, (64,), generator=gen).tolist() + [0, nleaves_per_r - 1]
    nt = NCOL // nleaves_per_r
    t = torch.arange(nt, dtype=torch.int64, device="cuda")
    op = T.col_ptr
    for r, o in zip(rs, os_):
        hit, v = _leaf_from_closed_form(torch, r, column_of(t, o))
        b, e = int(op[r + R * o]), int(op[r + R * o + 1])
        assert e - b == int(hit.sum()), f"length of leaf ({r}, {o})"
        assert torch.equal(T.row_idx[b:e].to(torch.int64), t[hit]), f"rows of leaf ({r}, {o})"
        assert torch.equal(T.val[b:e].to(torch.int64), v[hit]), f"values of leaf ({r}, {o})"


def test_aperm_213_past_2e31(big):
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    device.set_box_nnz(0)
    c0 = device.boxed_calls()
    B, bdim = A.aperm(DIM, (2, 1, 3))
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0 + 1
    assert tuple(bdim) == (D1, R, D2) and B.nrow == D1 and B.ncol == R * D2
    _well_formed(torch, B, nnz)
    # leaf (r, j2) of B: the entries (j1, A[r, j1 + 1120 j2])
    _sampled_leaves(torch, B, D2, lambda t, o: t + D1 * o, seed=7)
    # exact integer identities through kernels this change does not touch
    sb, _ = device.colstats(B, "sum", inner=R)
    sa, _ = device.colstats(A, "sum", inner=D1)
    assert sb.numel() == D2 and torch.equal(sb, sa)
    rs = device.rowsums(B)
    cs, _ = device.colstats(A, "sum")
    assert torch.equal(rs, cs.to(torch.float64).reshape(D2, D1).sum(0))
    del sa, sb, rs, cs
    # back to the closed form
    torch.cuda.empty_cache()
    A2, adim = B.aperm(bdim, (2, 1, 3))
    torch.cuda.synchronize()
    del B
    torch.cuda.empty_cache()
    assert device.boxed_calls() == c0 + 2
    assert tuple(adim) == DIM
    _same_as_closed_form(torch, A2, cp)


def test_aperm_312_and_231_past_2e31(big):
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    device.set_box_nnz(0)
    c0 = device.boxed_calls()
    C, cdim = A.aperm(DIM, (3, 1, 2))
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0 + 1
    assert tuple(cdim) == (D2, R, D1) and C.nrow == D2 and C.ncol == R * D1
    _well_formed(torch, C, nnz)
    # leaf (r, j1) of C: the entries (j2, A[r, j1 + 1120 j2])
    _sampled_leaves(torch, C, D1, lambda t, o: o + D1 * t, seed=8)
    # aperm(C, c(2, 3, 1)) has the extents (R, D1, D2): the closed form again
    torch.cuda.empty_cache()
    A2, adim = C.aperm(cdim, (2, 3, 1))
    torch.cuda.synchronize()
    del C
    torch.cuda.empty_cache()
    assert device.boxed_calls() == c0 + 2
    assert tuple(adim) == DIM
    _same_as_closed_form(torch, A2, cp)


def test_leaf_preserving_workspace_past_2e31(big):
    """The per-permutation function gives the leaf-preserving call at this size a workspace below 1 GB."""
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    lib = device._lib()
    d, p = np.asarray(DIM, np.int64), np.asarray((1, 3, 2), np.int32)
    need = lib.svt_dev_aperm_perm_ws_bytes(nnz, 3, d.ctypes.data, p.ctypes.data)
    assert need < 10**9
    assert need <= lib.svt_dev_aperm_ws_bytes(nnz, 3, d.ctypes.data)
    c0 = device.boxed_calls()
    B, bdim = A.aperm(DIM, (1, 3, 2))                    # (DeviceCSC.aperm sizes its workspace by that function)
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0
    assert tuple(bdim) == (R, D2, D1) and int(B.col_ptr[-1]) == nnz
