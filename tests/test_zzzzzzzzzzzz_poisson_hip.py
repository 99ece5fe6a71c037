"""poissonSparseArray() and simple_rpois() on the device (kernels_coerce.hip over svt_random_rules.h): every case compares
col_ptr, row_idx and val bit for bit with the numpy restatement of tests/poisson_cases.py, which never calls the library.
Extents, lambdas, seeds, windows of leaves, the dense road, the workspace contract in an arena of 0xA5 bytes, the
refusals, the law of the counts, and the host-level Session methods."""
import ctypes

import numpy as np
import pytest

import poisson_cases as pc
from helpers import Arena

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.HAVE_LONGDOUBLE, reason="numpy.longdouble has no 63-bit mantissa here")]

SEED = 7
BIG = (3000001, 3)                      # more tiles than the count kernel's grid
BIG_LAMBDA = -np.log(0.99)
BIG_TOTAL = 4                           # the leaves of the array the two windows of BIG are cut from


@pytest.fixture(scope="module")
def dev(hip):
    import sparsearray_amd.device as d
    return d


@pytest.fixture(scope="module")
def T(dev):
    return dev.coerce_tile()


def arrays(R):
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def same_arrays(got, want, what=""):
    for x, y, part in zip(got, want, ("col_ptr", "row_idx", "val")):
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {part} {x.dtype}{x.shape} != {y.dtype}{y.shape}"
        assert np.array_equal(x, y), f"{what}: {part}"


def check(dev, shape, lam, seed, first_leaf=0, nleaves=None, total=None):
    dim = shape if total is None else (shape[0], total)
    R = dev.poisson(dim, lambda_=lam, seed=seed, first_leaf=first_leaf, nleaves=nleaves)
    n = shape[1] if nleaves is None else nleaves
    assert (R.nrow, R.ncol, R.Rtype) == (shape[0], n, 13)
    same_arrays(arrays(R), pc.expected(seed, float(lam), shape[0], n, first_leaf, total), f"{shape} {lam} {seed} {first_leaf}")
    return R


# ---------------------------------------------------------------------------
# extents, lambdas, seeds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(9))
def test_extents(dev, T, k):
    shape, lam = pc.extents(T)[k]
    assert shape != BIG
    check(dev, shape, lam, SEED)


def test_more_tiles_than_the_grid(dev, T):
    assert pc.extents(T)[9] == (BIG, BIG_LAMBDA) and BIG[0] * BIG[1] > 2048 * T
    R = check(dev, BIG, BIG_LAMBDA, SEED, 0, BIG[1], BIG_TOTAL)           # (the first 3 leaves of 4 are the array of 3)
    same_arrays(arrays(dev.poisson(BIG, lambda_=BIG_LAMBDA, seed=SEED)), arrays(R))


def test_more_tiles_than_the_grid_from_an_odd_cell(dev, T):
    """first_leaf * nrow odd: the count kernel that makes a block per cell, over more tiles than its grid"""
    assert BIG[0] % 2 == 1
    check(dev, BIG, BIG_LAMBDA, SEED, 1, BIG[1], BIG_TOTAL)


@pytest.mark.parametrize("lam", pc.LAMBDAS)
def test_lambdas(dev, lam):
    R = check(dev, (37, 333), lam, SEED)
    if lam < 1e-16:
        assert R.nnz == 0
    if lam == 4.0:
        assert int(R.val.max()) >= 9            # the long search of find_interval runs


def test_density_is_lambda(dev):
    same_arrays(arrays(dev.poisson((37, 333), density=0.05, seed=SEED)), pc.expected(SEED, float(-np.log(1 - 0.05)), 37, 333))
    same_arrays(arrays(dev.poisson((37, 333), seed=SEED)), pc.expected(SEED, float(pc.DEFAULT_LAMBDA), 37, 333))


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_seeds(dev, seed):
    check(dev, (37, 333), pc.DEFAULT_LAMBDA, seed)


def test_seeds_give_different_arrays(dev):
    got = [arrays(dev.poisson((37, 333), seed=s))[1].tobytes() for s in pc.SEEDS]
    assert len(set(got)) == len(got)


# ---------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------
def test_windows_are_the_array(dev):
    whole = check(dev, (37, 333), pc.DEFAULT_LAMBDA, SEED)
    parts = []
    for first, n in ((0, 100), (100, 1), (101, 232)):           # 37 * 100 is even, 37 * 101 odd: both count kernels
        W = check(dev, (37, 333), pc.DEFAULT_LAMBDA, SEED, first, n, 333)
        same_arrays(arrays(W), arrays(dev.subset_cols(whole, np.arange(first, first + n, dtype=np.int32))), f"window {first}")
        parts.append(W)
    same_arrays(arrays(dev.cbind(*parts)), arrays(whole), "cbind of the windows")


def test_window_past_2_to_32_cells(dev):
    nrow, first, n = 65537, 65536, 2
    assert first * nrow > 2 ** 32
    R = dev.poisson((nrow, first + n), seed=SEED, first_leaf=first)
    assert R.ncol == n
    same_arrays(arrays(R), pc.expected(SEED, float(pc.DEFAULT_LAMBDA), nrow, n, first))


def test_windows_outside_the_array_are_refused(dev):
    from sparsearray_amd import SparseArrayError
    for kw in (dict(first_leaf=-1), dict(first_leaf=334), dict(first_leaf=300, nleaves=34), dict(nleaves=-1)):
        with pytest.raises(SparseArrayError, match="window of leaves"):
            dev.poisson((37, 333), **kw)
    assert dev.poisson((37, 333), first_leaf=333).ncol == 0


# ---------------------------------------------------------------------------
# two roads
# ---------------------------------------------------------------------------
def test_rpois_is_the_restatement(dev, T):
    for n, lam, seed, first in ((0, 1.0, 3, 0), (1, 1.0, 3, 0), (2 * T + 3, 1.0, 3, 0), (1000, 4.0, 2 ** 64 - 1, 2 ** 40 + 1),
                                (777, pc.DEFAULT_LAMBDA, 0, 2 ** 32 - 5), (100, 0.0, 1, 0)):
        got = dev.rpois(n, lam, seed=seed, first=first).cpu().numpy()
        want = pc.values(seed, np.uint64(first) + np.arange(n, dtype=np.uint64), lam)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, lam, seed, first)


@pytest.mark.parametrize("shape,lam", [((37, 333), pc.DEFAULT_LAMBDA), (BIG, BIG_LAMBDA)])
def test_dense_road_gives_the_sparse_road(dev, shape, lam):
    nrow, ncol = shape
    d = dev.rpois(nrow * ncol, lam, seed=SEED).view(ncol, nrow).t()         # column-major (nrow, ncol)
    same_arrays(arrays(dev.DeviceCSC.from_dense(d)), arrays(dev.poisson(shape, lambda_=lam, seed=SEED)), str(shape))


# ---------------------------------------------------------------------------
# the contract: _count + _fill in an arena with guard bands
# ---------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _two_calls(lam, seed, nrow, first, nleaves, prior):
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    cp, ri, vv = pc.expected(seed, float(lam), nrow, nleaves, first)
    nnz = ri.size
    need = lib.svt_dev_poisson_ws_bytes(nrow * nleaves)
    arena = Arena([need, 8 * (nleaves + 1), 4 * nnz, 4 * nnz])
    arena.part(0)[:] = prior
    got_nnz = ctypes.c_int64(-1)
    ptr = [arena.part(k).data_ptr() if arena.part(k).numel() else None for k in range(4)]
    args = (float(lam), seed, nrow, first, nleaves)
    assert lib.svt_dev_poisson_count(*args, ptr[1], ctypes.byref(got_nnz), ptr[0], need, _stream()) == 0, lib.svt_last_error()
    assert got_nnz.value == nnz
    assert lib.svt_dev_poisson_fill(*args, ptr[1], ptr[2], ptr[3], ptr[0], need, _stream()) == 0, lib.svt_last_error()
    torch.cuda.synchronize()
    assert arena.guards_intact()
    return (arena.part(1, torch.int64).cpu().numpy(), arena.part(2, torch.int32).cpu().numpy(),
            arena.part(3, torch.int32).cpu().numpy())


@pytest.mark.parametrize("lam,nrow,first,nleaves", [(pc.DEFAULT_LAMBDA, 37, 0, 333), (pc.DEFAULT_LAMBDA, 37, 101, 232),
                                                    (4.0, 4097, 0, 3), (1.0, 1, 0, 3 * 4096 + 5), (0.0, 37, 0, 333),
                                                    (1.0, 0, 0, 5), (1.0, 7, 0, 0)])
def test_workspace_discipline(dev, lam, nrow, first, nleaves):
    want = pc.expected(SEED, float(lam), nrow, nleaves, first)
    for prior in (0xA5, 0x00, 0xFF):
        same_arrays(_two_calls(lam, SEED, nrow, first, nleaves, prior), want, f"workspace of {prior:#x}")


def test_the_same_call_twice_gives_the_same_bits(dev):
    import torch
    for shape, lam in (((37, 333), 1.0), (BIG, BIG_LAMBDA)):
        a, b = (dev.poisson(shape, lambda_=lam, seed=SEED) for _ in range(2))
        for x, y in zip((a.col_ptr, a.row_idx, a.val), (b.col_ptr, b.row_idx, b.val)):
            assert torch.equal(x, y)
    assert torch.equal(dev.rpois(10 ** 6, 1.0, seed=SEED), dev.rpois(10 ** 6, 1.0, seed=SEED))


@pytest.mark.parametrize("lam,nrow,first,nleaves,short", [(1.0, 2 ** 31, 0, 1, False), (1.0, -1, 0, 1, False), (1.0, 5, 0, -1, False),
                                                          (1.0, 5, -1, 3, False), (1.0, 2 ** 31 - 1, 2 ** 33, 2 ** 33, False),
                                                          (1.0, 37, 0, 333, True), (4.5, 37, 0, 333, False),
                                                          (-1.0, 37, 0, 333, False), (float("nan"), 37, 0, 333, False)])
def test_a_status_leaves_the_outputs_untouched(dev, lam, nrow, first, nleaves, short):
    import torch
    from sparsearray_amd._hip import init
    lib = init()
    need = lib.svt_dev_poisson_ws_bytes(37 * 333)
    arena = Arena([need, 8 * 334, 4 * 1000, 4 * 1000, 4 * 1000])
    ptr = [arena.part(k).data_ptr() for k in range(5)]
    nnz = ctypes.c_int64(-7)
    ws_bytes = need - 1 if short else need
    args = (lam, SEED, nrow, first, nleaves)
    assert lib.svt_dev_poisson_count(*args, ptr[1], ctypes.byref(nnz), ptr[0], ws_bytes, _stream()) < 0
    assert lib.svt_last_error() != b""
    assert lib.svt_dev_poisson_fill(*args, ptr[1], ptr[2], ptr[3], ptr[0], ws_bytes, _stream()) < 0
    if not short:
        assert lib.svt_dev_rpois(lam if lam != 1.0 else 4.5, SEED, 0, 1000, ptr[4], _stream()) < 0
    torch.cuda.synchronize()
    assert nnz.value == -7 and arena.untouched()


def test_lambda_too_big_is_said_in_the_reference_words(dev):
    from sparsearray_amd import SparseArrayError
    with pytest.raises(SparseArrayError, match="'lambda' too big\\?"):
        dev.poisson((37, 333), lambda_=4.5)
    with pytest.raises(SparseArrayError, match="'lambda' too big\\?"):
        dev.rpois(10, 4.5)
    assert dev.poisson_ticks(4.0).size == 31


# ---------------------------------------------------------------------------
# the law, independent of the restatement
# ---------------------------------------------------------------------------
def test_counts_obey_the_poisson_law(dev):
    """2^22 cells at lambda = 1 under seed 20240607, for which the restatement passes the same check on the CPU
    (tests/test_zzzzzzzzzzzz_poisson_cpu.py): for every k with n p_k >= 25 the count of cells equal to k lies within
    6 sqrt(n p_k (1 - p_k)) of n p_k; p_k from lgamma, not from the ticks."""
    assert (pc.LAW_SEED, pc.LAW_N, pc.LAW_LAMBDA) == (20240607, 2 ** 22, 1.0)
    vals = dev.rpois(pc.LAW_N, pc.LAW_LAMBDA, seed=pc.LAW_SEED).cpu().numpy()
    assert pc.law_violations(vals) == []
    # and the sparse form of the same cells: the stored values are the nonzero ones
    R = dev.poisson((2 ** 11, 2 ** 11), lambda_=pc.LAW_LAMBDA, seed=pc.LAW_SEED)
    assert np.array_equal(np.bincount(R.val.cpu().numpy())[1:], np.bincount(vals)[1:])


# ---------------------------------------------------------------------------
# host level
# ---------------------------------------------------------------------------
def test_session_array_is_the_device_array(hip, dev):
    dim = (37, 111, 3)
    dn = [[f"r{i}" for i in range(37)], None, ["a", "b", "c"]]
    x = hip.poissonSparseArray(dim, lambda_=1.0, dimnames=dn, seed=SEED)
    assert x.type == "integer" and tuple(x.dim) == dim and x.dimnames == dn
    cp, ri, vv = x.to_csc()
    want = pc.expected(SEED, 1.0, 37, 333)
    same_arrays((np.asarray(cp, dtype=np.int64), np.asarray(ri, dtype=np.int32), np.asarray(vv, dtype=np.int32)), want)
    same_arrays(arrays(dev.poisson(dim, lambda_=1.0, seed=SEED)), want)
    d = pc.dense(SEED, 1.0, 37, 333)
    sums = np.asarray(hip.colSums(x), dtype=np.float64)
    assert sums.shape == (111, 3) and np.array_equal(sums.reshape(-1, order="F"), d.sum(axis=0).astype(np.float64))
    assert np.array_equal(x.to_dense().reshape(37, 333, order="F"), d)


def test_session_matrix_density_and_rpois(hip, dev):
    from sparsearray_amd import SparseArrayError
    m = hip.poissonSparseMatrix(37, 333, density=0.05, seed=2 ** 64 - 1)
    same_arrays(tuple(np.asarray(a) for a in m.to_csc()), pc.expected(2 ** 64 - 1, float(-np.log(1 - 0.05)), 37, 333))
    assert hip.poissonSparseArray((5, 0, 3)).nzcount() == 0 and hip.poissonSparseArray((0,)).nzcount() == 0
    got = hip.simple_rpois(5000, 1.0, seed=SEED)
    assert got.dtype == np.int32 and np.array_equal(got, dev.rpois(5000, 1.0, seed=SEED).cpu().numpy())
    assert hip.simple_rpois(0, 1.0).size == 0
    with pytest.raises(SparseArrayError, match="'lambda' too big\\?"):
        hip.poissonSparseArray((37, 333), lambda_=4.5)
    with pytest.raises(SparseArrayError, match="'lambda' too big\\?"):
        hip.simple_rpois(10, 4.5)
