"""colMads() / rowMads() on the device (kernels_median.hip: MadRule on the counting and the select kernel of the medians
and quantiles) against the plain definition on the dense column and against the host statement of
sparsearray_amd/api.py, at tolerance 0: every side evaluates the same IEEE operations."""
import numpy as np
import pytest

from helpers import assert_equal, assert_identical, random_csc
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, SparseArrayError, is_NA_real
from test_mads_cpu import check_argument_errors, check_mads_on_cases, dense_colmads
from test_medians import last_digit_columns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("na_rm", [False, True])
def test_hip_mads_are_the_dense_rule(hip, na_rm):
    check_mads_on_cases(hip, na_rm, "hip")


@pytest.mark.parametrize("na_rm", [False, True])
def test_hip_mads_against_host_statement(hip, oracle, na_rm):
    check_mads_on_cases(hip, na_rm, "hip vs oracle", reference=oracle)


def _mad_select_operand(type_):
    """5000-row columns (several sweeps of the 256-thread workgroup) of every fill class, and a center for each.  With
    the given centers: more than 1024 equal deviations (x in {c - 1.5, c + 1.5}: msel_select gives up and rank k + 1
    takes the extra counting pass), deviations that differ only in low mantissa bits, the block of the zeros'
    deviation |c| in the middle of the deviations, at their bottom (c = 0, or every x beyond 2c) and at their top (every
    x inside (0, 2c)), 1e200-scale values, +-Inf, NA / NaN.  Without them: nonzero medians with few zeros, short columns
    among many zeros (answered from the median's counts), columns with median 0 but fewer than half zeros (not so).
    Doubles also: the columns of test_medians.last_digit_columns with the centers 0.5, 0 and 2 -- the deviations
    0.5 + k 2^-52, 1 + k 2^-52 and 1 - k 2^-52 are exact and differ in their last bits only, about five copies of each:
    msel_select gives up after its last digit pass with a handful of candidates, and rank k + 1 is one step above."""
    rng = np.random.default_rng(71)
    nrow = 5000
    scale = 1000 if type_ == "integer" else 1
    cols, cen = [], []
    for j in range(72):
        col = np.zeros(nrow)
        fill = [1.0, 0.97, 0.8, 0.6, 0.51, 0.3][j % 6]
        m = rng.random(nrow) < fill
        kind = (j // 6) % 6
        if kind == 0:                                                           # block in the middle
            c = 2.0
            v = rng.normal(size=nrow) * 3 + c
        elif kind == 1:                                                         # more than 1024 equal deviations
            c = [2.5, -0.5][j % 2]
            v = c + rng.choice([-1.5, 1.5], nrow)
        elif kind == 2:                                                         # low mantissa bits of the deviation
            c = 3.0
            v = c + (1.0 + rng.integers(0, 1 << 20, nrow) * 2.0 ** -50) * rng.choice([-1.0, 1.0], nrow)
        elif kind == 3:                                                         # block at the top / at the bottom
            c = [1.0, 0.0, -1.0][j % 3]
            v = rng.uniform(0.2, 1.8, nrow) * (c if c else 1.0) if j % 2 else c + 4.0 + np.abs(rng.normal(size=nrow))
        elif kind == 4:                                                         # 1e200 scale
            c = [1e200, -3e199][j % 2]
            v = rng.normal(size=nrow) * 1e200
        else:                                                                   # duplicates on both sides of c
            c = 1.0
            v = rng.integers(-3, 6, nrow).astype(np.float64)
        if type_ == "integer":
            if kind not in (2, 4):
                c, v = c * scale, v * scale                                    # (kind 1: x - c = +-1500 exactly)
            v = np.round(v).clip(-2e9, 2e9)                                    # (kind 4: the centers stay far outside)
        col[m] = v[m]
        cols.append(col)
        cen.append(c)
    a = np.stack(cols, axis=1)
    short = np.zeros((nrow, 10))
    short[:3, 0] = [5, 6, 7]                                                    # median 0, nearly all zeros
    short[:40, 1] = -np.arange(1, 41)
    short[: nrow // 2 - 1, 2] = 2.0                                             # median 0, zeros a bare majority
    short[: nrow // 2, 3] = 2.0                                                 # exactly half: median 1, no shortcut
    short[: nrow // 2 + 1, 4] = 2.0                                             # median 2, b = 2 = every deviation
    short[:2000, 5] = -1.0 - rng.random(2000); short[2000:4000, 5] = 1.0 + rng.random(2000)   # median 0, 1000 zeros
    short[:2400, 6] = -3.0; short[2400:4800, 6] = 3.0                           # median 0, 200 zeros, M = 3
    short[:2500, 7] = -1.0; short[2500:, 7] = 1.0                               # median (-1 + 1) / 2 = 0, no zero
    short[:, 8] = np.arange(nrow) - 100.0                                       # all distinct
    short[:1500, 9] = 4.0; short[1500:1600, 9] = np.arange(100) + 5.0
    a = np.concatenate([a, short], axis=1)
    cen += [0.0, 0.0, 2.0, 1.0, 2.0, 0.5, 3.0, -1.0, 2400.0, 4.0]
    if type_ == "double":
        a[17, 3] = np.inf; a[18, 3] = -np.inf; a[5, 9] = np.nan; a[6, 10] = NA_real; a[:40, 11] = np.nan
        a[7, 20] = np.inf; a[9, 27] = -np.inf
        inf = np.zeros((nrow, 4))
        inf[: nrow // 2, 0] = -np.inf; inf[nrow // 2:, 0] = np.inf             # median NaN: NA
        inf[:1250, 1] = -np.inf; inf[1250:3000, 1] = rng.normal(size=1750); inf[3000:, 1] = np.inf
        inf[:100, 2] = np.inf; inf[100:3000, 2] = np.abs(rng.normal(size=2900)) + 1
        inf[:3000, 3] = np.inf                                                 # median +Inf: its own deviation is NaN
        a = np.concatenate([a, last_digit_columns(nrow), inf], axis=1)
        cen += [0.5, 0.0, 2.0] + [0.0, np.inf, 1.5, -np.inf]
        return SVT_SparseArray.from_dense(np.asfortranarray(a), "double"), a, np.array(cen)
    ai = a.astype(np.int32)
    ai[5, 9] = NA_integer; ai[:40, 11] = NA_integer
    dense = ai.astype(np.float64); dense[ai == NA_integer] = np.nan
    return SVT_SparseArray.from_dense(np.asfortranarray(ai), "integer"), dense, np.array(cen)


@pytest.fixture(scope="module", params=["double", "integer"])
def mad_operand(request):
    x, dense, cen = _mad_select_operand(request.param)
    want = {(given, na_rm): dense_colmads(dense, cen if given else None, 1.4826, na_rm)
            for given in (False, True) for na_rm in (False, True)}
    return request.param, x, dense, cen, want


def test_hip_colmads_select_against_dense_rule(hip, mad_operand):
    type_, x, dense, cen, want = mad_operand
    for (given, na_rm), w in want.items():
        got = hip.colMads(x, center=cen if given else None, na_rm=na_rm)
        assert_equal(got, w, tol=0, strict_na=True, what=f"{type_} given={given} na_rm={na_rm}")
    # the operand has what its docstring says: undecided columns, NA results, zero and nonzero results
    w = want[(False, False)]
    assert is_NA_real(w).any() and (w == 0.0).any() and (w[~np.isnan(w)] > 0.0).sum() > 40


def test_hip_colmads_given_medians_is_colmads(hip, mad_operand):
    """colMads(x, center = colMedians(x)) is colMads(x) bit for bit: the center array inside the workspace holds what
    colMedians returns, and the answers taken from the median's counts are those of the full pass."""
    type_, x, dense, cen, want = mad_operand
    for na_rm in (False, True):
        med = hip.colMedians(x, na_rm=na_rm)
        for k in (1.4826, 1.0):
            assert_identical(hip.colMads(x, center=med, constant=k, na_rm=na_rm), hip.colMads(x, constant=k, na_rm=na_rm),
                             what=f"{type_} na_rm={na_rm} constant={k}")


def test_hip_colmads_about_zero_is_the_median_of_abs(hip, mad_operand):
    """colMads(x, center = 0, constant = 1) is colMedians(|x|) bit for bit, |x| built on the host; on the columns
    without missing values."""
    type_, x, dense, cen, want = mad_operand
    keep = ~np.isnan(dense).any(axis=0)
    d = dense[:, keep]
    if type_ == "integer":
        xs = SVT_SparseArray.from_dense(np.asfortranarray(d.astype(np.int32)), "integer")
        xa = SVT_SparseArray.from_dense(np.asfortranarray(np.abs(d).astype(np.int32)), "integer")
    else:
        xs = SVT_SparseArray.from_dense(np.asfortranarray(d), "double")
        xa = SVT_SparseArray.from_dense(np.asfortranarray(np.abs(d)), "double")
    assert_identical(hip.colMads(xs, center=0, constant=1), hip.colMedians(xa), what=type_)


def test_hip_rowmads_on_select_operand(hip, mad_operand):
    """Rows of t(x) are these columns: the transposition on the device, then the same kernels."""
    type_, x, dense, cen, want = mad_operand
    clean = np.where(np.isnan(dense), 0.0, dense)
    xt = SVT_SparseArray.from_dense(np.asfortranarray(clean.T), "double")
    assert_equal(hip.rowMads(xt), dense_colmads(clean, None, 1.4826, False), tol=0, strict_na=True, what="rowMads")
    assert_equal(hip.rowMads(xt, center=cen, constant=1.0), dense_colmads(clean, cen, 1.0, False), tol=0,
                 strict_na=True, what="rowMads, given centers")


@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_colmads_tall(hip, type_):
    """300 000-row columns: many sweeps of one workgroup, all six digit passes with survivors."""
    rng = np.random.default_rng(72)
    tall = rng.normal(size=(300_000, 3)) + 0.75
    tall[:, 1] = np.round(tall[:, 1], 1)
    tall[rng.random(tall.shape) < 0.2] = 0.0
    td = tall if type_ == "double" else np.round(tall * 100)
    xt = SVT_SparseArray.from_dense(np.asfortranarray(td if type_ == "double" else td.astype(np.int32)), type_)
    assert_equal(hip.colMads(xt), dense_colmads(td, None, 1.4826, False), tol=0, strict_na=True, what="tall")
    cen = np.array([0.5, -1.0, 70.0])
    assert_equal(hip.colMads(xt, center=cen), dense_colmads(td, cen, 1.4826, False), tol=0, strict_na=True,
                 what="tall, given centers")


def _resident(nrow, ncol):
    from sparsearray_amd.device import DeviceCSC
    cp, ri, v = random_csc(nrow, ncol, 0.6, seed=53)                # dense enough for selects
    dense = np.zeros((nrow, ncol))
    for j in range(ncol):
        dense[ri[cp[j]:cp[j + 1]], j] = v[cp[j]:cp[j + 1]]
    return DeviceCSC.from_host(nrow, cp, ri, v), dense


def test_device_colmads_resident(hip):
    import torch
    from sparsearray_amd.device import _lib, colmads
    nrow, ncol = 3000, 40
    A, dense = _resident(nrow, ncol)
    cen = np.linspace(-0.5, 0.5, ncol)
    dcen = torch.as_tensor(cen, device="cuda")
    nbytes = _lib().svt_dev_colmads_ws_bytes(A.nnz, A.ncol)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for center, host_center in ((None, None), (dcen, cen)):
        want = dense_colmads(dense, host_center, 1.4826, False)
        out1 = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
        out2 = torch.full((ncol,), -2.0, dtype=torch.float64, device="cuda")
        assert colmads(A, center=center, out=out1, ws=ws) is out1
        colmads(A, center=center, out=out2, ws=ws)
        g1, g2 = out1.cpu().numpy(), out2.cpu().numpy()
        assert np.array_equal(g1.view(np.int64), g2.view(np.int64))
        assert_equal(g1, want, tol=0, strict_na=True, what="device colmads")
        assert_equal(colmads(A, center=center, constant=-2.0).cpu().numpy(),
                     dense_colmads(dense, host_center, -2.0, False), tol=0, strict_na=True)
    with pytest.raises(SparseArrayError, match="workspace too small"):
        colmads(A, out=out1, ws=ws[:nbytes - 1])
    with pytest.raises(SparseArrayError, match="one element per column"):
        colmads(A, center=dcen[:ncol - 1].contiguous())


@pytest.mark.parametrize("ncol", [1, 3, 40])
def test_device_colmads_stays_inside_its_workspace(hip, ncol):
    """colmads carves two sets of per-column arrays and the centers out of a caller's workspace of exactly the advertised
    size, at an odd address: right results, and not a byte touched before or after it."""
    import torch
    from sparsearray_amd.device import _lib, colmads
    A, dense = _resident(3000, ncol)
    nbytes = _lib().svt_dev_colmads_ws_bytes(A.nnz, ncol)
    assert nbytes == ncol * 64 + 1024
    cen = np.linspace(-0.5, 0.5, ncol)
    dcen = torch.as_tensor(cen, device="cuda")
    for center, host_center in ((None, None), (dcen, cen)):
        pad = 519
        arena = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = arena[pad:pad + nbytes]
        assert_equal(colmads(A, center=center, ws=ws).cpu().numpy(), dense_colmads(dense, host_center, 1.4826, False),
                     tol=0, strict_na=True, what=f"ncol={ncol}")
        assert bool((arena[:pad] == 0xA5).all()) and bool((arena[pad + nbytes:] == 0xA5).all())
        with pytest.raises(SparseArrayError, match="workspace too small"):
            colmads(A, center=center, ws=ws[:nbytes - 1])


def test_hip_mads_extents_and_errors(hip):
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    for cen in (None, 1.0, np.array([1.0, 2.0, 3.0])):
        m = hip.colMads(x0, center=cen)
        assert m.shape == (3,) and is_NA_real(m).all()
    assert hip.rowMads(x0).shape == (0,)
    x1 = SVT_SparseArray((4, 0), "double", [])
    assert hip.colMads(x1).shape == (0,)
    for cen in (None, 1.0, np.arange(4.0)):
        r = hip.rowMads(x1, center=cen)
        assert r.shape == (4,) and is_NA_real(r).all()
    check_argument_errors(hip)
    # the library's own checks (what a caller of the C ABI meets)
    x = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3, 4)), "double")
    x3 = SVT_SparseArray((2, 2, 2), "double", [None] * 4)
    na = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3)), "double", na_background=True)
    with pytest.raises(SparseArrayError, match=r"the colMads\(\) method for SparseArray objects only supports 2D"):
        hip.SparseArray_Call("C_colMads_SVT", x3, None, 1.4826, False)
    with pytest.raises(SparseArrayError, match=r"the rowMads\(\) method for SparseArray objects only supports 2D"):
        hip.SparseArray_Call("C_rowMads_SVT", x3, None, 1.4826, False)
    for entry in ("C_colMads_SVT", "C_rowMads_SVT"):
        with pytest.raises(SparseArrayError, match=r"colMads\(\) is not supported on NaArray objects"):
            hip.SparseArray_Call(entry, na, None, 1.4826, False)
    with pytest.raises(SparseArrayError, match="one element per column"):
        hip.SparseArray_Call("C_colMads_SVT", x, np.zeros(3), 1.4826, False)
    with pytest.raises(SparseArrayError, match="one element per row"):
        hip.SparseArray_Call("C_rowMads_SVT", x, np.zeros(4), 1.4826, False)
    assert_equal(hip.SparseArray_Call("C_colMads_SVT", x, np.zeros(4), 1.0, False), [0.0, 0.0, 0.0, 0.0], tol=0)
    assert_equal(hip.SparseArray_Call("C_rowMads_SVT", x, None, 1.0, False), [0.0, 0.0, 0.0], tol=0)
