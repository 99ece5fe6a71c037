"""Device t(), leaf-preserving aperm and colMedians of an operand past 2^31 nonzeros (about 2.27e9), built on the
device from a closed form, so that every row and every column is known without a reduction of that size:
  32768 rows, 1 120 000 columns; column j holds L_j = 2000 + (j * 7919 mod 49) - 24 entries at the rows
  k * 16 + (5 j mod 16); every 1000th column is dense (all 32768 rows); value(j, k) = (31 j + 17 k) mod 2001 - 1000,
  1001 where that is 0.
Peak device memory: t(t(A)) while A, t(A) and the boxed driver's workspace are alive -- 3 x 18.2 GB of operands + ~35.4 GB
of workspace = ~90 GB (84 GiB), plus torch's own temporaries; the tests skip when less than that and a margin is free."""
import pytest

pytestmark = pytest.mark.gpu

R, NCOL, S = 32768, 1_120_000, 16
CHUNK = 40_000
PEAK = 84 * 2**30


def _torch():
    import torch
    return torch


def _lengths(torch, j):
    L = 2000 + (j * 7919) % 49 - 24
    return torch.where(j % 1000 == 0, torch.full_like(L, R), L)


def _entries(torch, j0, j1, cp):
    """rows, values of columns [j0, j1) (int32), in the operand's order"""
    j = torch.arange(j0, j1, dtype=torch.int64, device="cuda")
    L = _lengths(torch, j)
    jj = torch.repeat_interleave(j, L)
    k = torch.arange(int(cp[j1] - cp[j0]), dtype=torch.int64, device="cuda") - (cp[jj] - cp[j0])
    dense = jj % 1000 == 0
    rows = torch.where(dense, k, k * S + (5 * jj) % S)
    v = (31 * jj + 17 * k) % 2001 - 1000
    v = torch.where(v == 0, torch.full_like(v, 1001), v)
    return rows.to(torch.int32), v.to(torch.int32)


def _build(torch):
    from sparsearray_amd import device
    j = torch.arange(NCOL, dtype=torch.int64, device="cuda")
    cp = torch.zeros(NCOL + 1, dtype=torch.int64, device="cuda")
    cp[1:] = torch.cumsum(_lengths(torch, j), 0)
    nnz = int(cp[-1])
    ri = torch.empty(nnz, dtype=torch.int32, device="cuda")
    val = torch.empty(nnz, dtype=torch.int32, device="cuda")
    for j0 in range(0, NCOL, CHUNK):
        j1 = min(j0 + CHUNK, NCOL)
        r, v = _entries(torch, j0, j1, cp)
        ri[int(cp[j0]):int(cp[j1])] = r
        val[int(cp[j0]):int(cp[j1])] = v
        del r, v
    return device.DeviceCSC(R, cp, ri, val), cp, nnz


def _same_as_closed_form(torch, A, cp):
    assert torch.equal(A.col_ptr, cp)
    for j0 in range(0, NCOL, CHUNK):
        j1 = min(j0 + CHUNK, NCOL)
        r, v = _entries(torch, j0, j1, cp)
        assert torch.equal(A.row_idx[int(cp[j0]):int(cp[j1])], r), f"rows of columns {j0}..{j1}"
        assert torch.equal(A.val[int(cp[j0]):int(cp[j1])], v), f"values of columns {j0}..{j1}"
        del r, v


@pytest.fixture(scope="module")
def big(hip):
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < PEAK + 6 * 2**30:
        pytest.skip(f"needs {PEAK / 2**30 + 6:.0f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    A, cp, nnz = _build(torch)
    assert nnz >= 2**31 + 2**26
    yield A, cp, nnz
    del A, cp
    torch.cuda.empty_cache()


def test_t_past_2e31(big):
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    device.set_box_nnz(0)
    c0 = device.boxed_calls()
    tA = A.t()
    torch.cuda.synchronize()
    assert device.boxed_calls() == c0 + 1
    op = tA.col_ptr
    assert int(op[0]) == 0 and int(op[-1]) == nnz
    assert bool(torch.all(op[1:] >= op[:-1]))
    # 64 sampled output leaves against the closed form, enumerated over all columns
    j = torch.arange(NCOL, dtype=torch.int64, device="cuda")
    L = _lengths(torch, j)
    dense = j % 1000 == 0
    gen = torch.Generator().manual_seed(7)
    rows = torch.randint(0, R, (62,), generator=gen).tolist() + [0, R - 1]
    for r in rows:
        hit = dense | (((5 * j) % S == r % S) & (r // S < L))
        js = j[hit]
        k = torch.where(dense[hit], torch.full_like(js, r), torch.full_like(js, r // S))
        v = (31 * js + 17 * k) % 2001 - 1000
        v = torch.where(v == 0, torch.full_like(v, 1001), v)
        b, e = int(op[r]), int(op[r + 1])
        assert e - b == js.numel(), f"length of row {r}"
        assert torch.equal(tA.row_idx[b:e].to(torch.int64), js), f"columns of row {r}"
        assert torch.equal(tA.val[b:e].to(torch.int64), v), f"values of row {r}"
    # colSums(t(A)) == rowSums(A), exact in int
    cs, _ = device.colstats(tA, "sum")
    rs = device.rowsums(A)
    assert torch.equal(cs.to(torch.float64), rs)
    del cs, rs
    # t(t(A)) == A: A itself is rebuilt afterwards by the fixture's closed form
    tt = tA.t()
    torch.cuda.synchronize()
    del tA
    torch.cuda.empty_cache()
    assert device.boxed_calls() == c0 + 2
    _same_as_closed_form(torch, tt, cp)


def test_leaf_preserving_aperm_past_2e31(big):
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    dim = (R, 1120, 1000)
    B, bdim = A.aperm(dim, (1, 3, 2))
    assert tuple(bdim) == (R, 1000, 1120)
    C, cdim = B.aperm(bdim, (1, 3, 2))
    torch.cuda.synchronize()
    del B
    torch.cuda.empty_cache()
    assert tuple(cdim) == dim
    _same_as_closed_form(torch, C, cp)


def test_colmedians_past_2e31(big):
    from sparsearray_amd import device
    torch = _torch()
    A, cp, nnz = big
    med = device.colmedians(A)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(11)
    cols = list(range(0, NCOL, 1000)) + torch.randint(0, NCOL, (64,), generator=gen).tolist() + [NCOL - 1]
    for j in cols:
        n = int(cp[j + 1] - cp[j])
        k = torch.arange(n, dtype=torch.int64, device="cuda")
        v = (31 * j + 17 * k) % 2001 - 1000
        v = torch.where(v == 0, torch.full_like(v, 1001), v).to(torch.float64)
        s = torch.sort(torch.cat([v, torch.zeros(R - n, dtype=torch.float64, device="cuda")])).values
        want = float((s[R // 2 - 1] + s[R // 2]) * 0.5)          # R is even
        assert float(med[j]) == want, f"column {j}"
