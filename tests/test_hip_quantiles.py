"""colQuantiles() / rowQuantiles() / colIQRs() on the device (kernels_median.hip: one counting pass, one select launch
for the (column, prob) pairs it could not decide) against the plain definition on the dense column and against the
host statement of sparsearray_amd/api.py, at tolerance 0: every side evaluates the same IEEE operations."""
import numpy as np
import pytest

from helpers import assert_equal, assert_identical, random_csc
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, SparseArrayError, is_NA_real
from test_medians import _dense_colmedians, last_digit_columns
from test_quantiles_cpu import (PROBS_SETS, as_float, check_session_on_cases, dense_colquantiles, dense_iqrs,
                                quantile_cases)

pytestmark = pytest.mark.gpu

# (the last four: at and on either side of the two middle ranks of a 5000-value column, see last_digit_columns)
SELECT_PROBS = (0, 0.01, 0.25, 1 / 3, 0.5, 0.75, 0.99, 1, 2499 / 4999, 2500 / 4999, 0.49995, 0.50005)


@pytest.mark.parametrize("na_rm", [False, True])
def test_hip_quantiles_are_the_dense_rule(hip, na_rm):
    check_session_on_cases(hip, na_rm, "hip")


@pytest.mark.parametrize("na_rm", [False, True])
def test_hip_quantiles_against_host_statement(hip, oracle, na_rm):
    for name, a, type_ in quantile_cases():
        x = SVT_SparseArray.from_dense(np.asfortranarray(a), type_)
        for probs in PROBS_SETS:
            assert_equal(hip.colQuantiles(x, probs, na_rm=na_rm), oracle.colQuantiles(x, probs, na_rm=na_rm),
                         tol=0, strict_na=True, what=f"{name} {probs}")
            assert_equal(hip.rowQuantiles(x, probs, na_rm=na_rm), oracle.rowQuantiles(x, probs, na_rm=na_rm),
                         tol=0, strict_na=True, what=f"{name} rows {probs}")
        f = as_float(a, type_)
        assert_equal(hip.colIQRs(x, na_rm=na_rm), dense_iqrs(f, na_rm), tol=0, strict_na=True, what=name)
        assert_equal(hip.rowIQRs(x, na_rm=na_rm), dense_iqrs(f.T, na_rm), tol=0, strict_na=True, what=name + " rows")


def test_hip_quantiles_extents_and_errors(hip):
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    q = hip.colQuantiles(x0)
    assert q.shape == (3, 5) and is_NA_real(q).all()
    assert hip.rowQuantiles(x0).shape == (0, 5)
    x1 = SVT_SparseArray((4, 0), "double", [])
    assert hip.colQuantiles(x1, (0.1, 0.2)).shape == (0, 2)
    r = hip.rowQuantiles(x1, (0.1, 0.2))
    assert r.shape == (4, 2) and is_NA_real(r).all()
    x = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3)), "double")
    assert hip.colQuantiles(x, ()).shape == (3, 0)
    assert hip.rowQuantiles(x, ()).shape == (3, 0)
    with pytest.raises(SparseArrayError, match=r"the colQuantiles\(\) method for SparseArray objects only supports 2D"):
        hip.colQuantiles(SVT_SparseArray((2, 2, 2), "double", [None] * 4))
    with pytest.raises(SparseArrayError, match=r"colQuantiles\(\) is not supported on NaArray objects"):
        hip.colQuantiles(SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3)), "double", na_background=True))
    with pytest.raises(SparseArrayError, match="only type = 7 is supported"):
        hip.colQuantiles(x, type=5)
    with pytest.raises(SparseArrayError, match=r"'probs' outside \[0,1\]"):
        hip.colQuantiles(x, (0.5, 1.5))
    # the library's own checks (what a caller of the C ABI meets)
    for bad in (1.5, -0.1, np.nan):
        with pytest.raises(SparseArrayError, match=r"'probs' outside \[0,1\]"):
            hip.SparseArray_Call("C_colQuantiles_SVT", x, np.array([0.5, bad]), False)
    with pytest.raises(SparseArrayError, match=r"the rowQuantiles\(\) method for SparseArray objects only supports 2D"):
        hip.SparseArray_Call("C_rowQuantiles_SVT", SVT_SparseArray((2, 2, 2), "double", [None] * 4),
                             np.array([0.5]), False)


def _select_operand(type_):
    """5000-row columns of every fill class (several sweeps of the 256-thread workgroup), see
    test_hip_colmedians_radix_select_against_numpy: normal values, heavy duplicates (more than 1024 equal keys in a
    column: msel_select gives up and rank k + 1 takes the extra counting pass), values that differ only in low
    mantissa bits, negative majorities, 1e200-scale values, +-Inf as interpolation neighbours, NA / NaN, and short
    columns among many zeros; and (doubles) keys that differ in their last ten bits only, about five copies of each:
    msel_select gives up after its last digit pass with a handful of candidates, and rank k + 1 is one ulp above."""
    rng = np.random.default_rng(67)
    nrow = 5000
    cols = []
    for j in range(72):
        col = np.zeros(nrow)
        fill = [1.0, 0.97, 0.8, 0.6, 0.51, 0.3][j % 6]
        m = rng.random(nrow) < fill
        kind = (j // 6) % 6
        if kind == 0:
            v = rng.normal(size=nrow)
        elif kind == 1:
            v = rng.integers(-3, 4, nrow).astype(np.float64)                    # duplicates
        elif kind == 2:
            v = 1.0 + rng.integers(0, 1 << 20, nrow) * 2.0 ** -52               # same exponent, low mantissa bits
        elif kind == 3:
            v = -np.abs(rng.normal(size=nrow)) - (j % 3)                         # negative majority
        elif kind == 4:
            v = np.abs(rng.normal(size=nrow)) * 1e200 * (1 if j % 2 else -1)
        else:
            v = rng.choice([-1.5, 2.5], nrow)                                   # more than 1024 equal keys, both signs
        if type_ == "integer":
            v = np.round(v * (1000 if kind != 2 else 1)).clip(-2e9, 2e9)
        col[m] = v[m]
        cols.append(col)
    a = np.stack(cols, axis=1)
    short = np.zeros((nrow, 8))                                                # few stored values among many zeros
    short[:3, 0] = [5, 6, 7]
    short[:nrow // 2 + 1, 1] = 2.0
    short[: nrow // 2, 2] = -2.0; short[nrow // 2:, 2] = 3.0
    short[:, 3] = np.arange(nrow) - 100.0
    short[:, 4] = np.where(np.arange(nrow) % 2 == 0, -1.0, 1.0)
    short[:, 5] = 7.0                                                          # one key, 5000 times
    short[:40, 6] = -np.arange(1, 41)
    short[:1500, 7] = 4.0; short[1500:1600, 7] = np.arange(100) + 5.0          # rank k in 1500 equal keys, k + 1 above
    a = np.concatenate([a, short], axis=1)
    if type_ == "double":
        a[17, 3] = np.inf; a[18, 3] = -np.inf; a[5, 9] = np.nan; a[6, 10] = NA_real; a[:40, 11] = np.nan
        inf = np.zeros((nrow, 3))
        inf[: nrow // 2, 0] = -np.inf; inf[nrow // 2:, 0] = np.inf             # the median's neighbours: -Inf, +Inf
        inf[:1250, 1] = -np.inf; inf[1250:3000, 1] = rng.normal(size=1750); inf[3000:, 1] = np.inf
        inf[:100, 2] = np.inf; inf[100:3000, 2] = np.abs(rng.normal(size=2900)) + 1
        a = np.concatenate([a, last_digit_columns(nrow), inf], axis=1)
        return SVT_SparseArray.from_dense(np.asfortranarray(a), "double"), a
    ai = a.astype(np.int32)
    ai[5, 9] = NA_integer; ai[:40, 11] = NA_integer
    dense = ai.astype(np.float64); dense[ai == NA_integer] = np.nan
    return SVT_SparseArray.from_dense(np.asfortranarray(ai), "integer"), dense


@pytest.fixture(scope="module", params=["double", "integer"])
def select_operand(request):
    x, dense = _select_operand(request.param)
    want = {na_rm: dense_colquantiles(dense, SELECT_PROBS, na_rm) for na_rm in (False, True)}
    return request.param, x, dense, want


def test_hip_colquantiles_select_against_dense_rule(hip, select_operand):
    type_, x, dense, want = select_operand
    for na_rm in (False, True):
        got = hip.colQuantiles(x, SELECT_PROBS, na_rm=na_rm)
        assert_equal(got, want[na_rm], tol=0, strict_na=True, what=f"{type_} na_rm={na_rm}")
    if type_ == "double":
        j = dense.shape[1] - 3                          # half -Inf, half +Inf: NaN at 0.5, not NA
        mid = hip.colQuantiles(x, (0.5,))[j, 0]
        assert np.isnan(mid) and not is_NA_real(mid)
    # unsorted and repeated probs keep their order
    probs = (0.99, 0.25, 0.25, 0.5, 0.01)
    idx = [SELECT_PROBS.index(p) for p in probs]
    assert_equal(hip.colQuantiles(x, probs, na_rm=True), want[True][:, idx], tol=0, strict_na=True, what="order")


def test_hip_colmedians_is_the_half_quantile(hip, select_operand):
    """The median rule and the quantile rule run the same select: identical bits on this operand."""
    type_, x, dense, want = select_operand
    for na_rm in (False, True):
        med = hip.colMedians(x, na_rm=na_rm)
        assert_identical(med, hip.colQuantiles(x, (0.5,), na_rm=na_rm)[:, 0], what=f"{type_} na_rm={na_rm}")
        assert_equal(med, want[na_rm][:, SELECT_PROBS.index(0.5)], tol=0, strict_na=True)


def test_hip_iqrs_and_rows_on_select_operand(hip, select_operand):
    type_, x, dense, want = select_operand
    q = want[True][:, [SELECT_PROBS.index(0.25), SELECT_PROBS.index(0.75)]]
    with np.errstate(all="ignore"):
        d = q[:, 1] - q[:, 0]
    d[is_NA_real(q[:, 0]) | is_NA_real(q[:, 1])] = NA_real
    assert_equal(hip.colIQRs(x, na_rm=True), d, tol=0, strict_na=True, what="colIQRs")
    # rows of t(x) are these columns: the transposition on the device, then the same kernels
    xt = SVT_SparseArray.from_dense(np.asfortranarray(np.where(np.isnan(dense), 0.0, dense).T), "double")
    clean = np.where(np.isnan(dense), 0.0, dense)
    assert_equal(hip.rowQuantiles(xt, (0.25, 0.5, 0.99)), dense_colquantiles(clean, (0.25, 0.5, 0.99), False),
                 tol=0, strict_na=True, what="rowQuantiles")


@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_colquantiles_tall(hip, type_):
    """300 000-row columns: many sweeps of one workgroup, all six digit passes with survivors."""
    rng = np.random.default_rng(68)
    tall = rng.normal(size=(300_000, 3))
    tall[:, 1] = np.round(tall[:, 1], 1)
    tall[rng.random(tall.shape) < 0.2] = 0.0
    td = tall if type_ == "double" else np.round(tall * 100)
    xt = SVT_SparseArray.from_dense(np.asfortranarray(td if type_ == "double" else td.astype(np.int32)), type_)
    assert_equal(hip.colQuantiles(xt), dense_colquantiles(td, (0, 0.25, 0.5, 0.75, 1), False), tol=0,
                 strict_na=True, what="tall")


def test_device_colquantiles_resident(hip):
    import torch
    from sparsearray_amd.device import DeviceCSC, _lib, colquantiles
    nrow, ncol = 3000, 40
    cp, ri, v = random_csc(nrow, ncol, 0.6, seed=52)            # dense enough for selects
    A = DeviceCSC.from_host(nrow, cp, ri, v)
    probs = (0.25, 0.5, 0.75, 0.1)
    dense = np.zeros((nrow, ncol))
    for j in range(ncol):
        dense[ri[cp[j]:cp[j + 1]], j] = v[cp[j]:cp[j + 1]]
    want = dense_colquantiles(dense, probs, False)
    nbytes = _lib().svt_dev_colquantiles_ws_bytes(A.nnz, A.ncol, len(probs))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out1 = torch.full((len(probs), ncol), -1.0, dtype=torch.float64, device="cuda")
    out2 = torch.full((len(probs), ncol), -2.0, dtype=torch.float64, device="cuda")
    assert colquantiles(A, probs, out=out1, ws=ws) is out1
    colquantiles(A, probs, out=out2, ws=ws)
    g1, g2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert np.array_equal(g1.view(np.int64), g2.view(np.int64))
    assert_equal(g1.T, want, tol=0, strict_na=True, what="device colquantiles")
    assert_equal(colquantiles(A, probs).cpu().numpy().T, want, tol=0, strict_na=True)
    with pytest.raises(SparseArrayError, match="workspace too small"):
        colquantiles(A, probs, out=out1, ws=ws[:nbytes - 1])
    with pytest.raises(SparseArrayError, match=r"'probs' outside \[0,1\]"):
        colquantiles(A, (0.5, 2.0))


@pytest.mark.parametrize("ncol", [1, 3, 40])
def test_device_order_stats_stay_inside_their_workspace(hip, ncol):
    """colmedians and colquantiles carve their per-column arrays out of a caller's workspace of exactly the advertised
    size, at an odd address: right results, and not a byte touched before or after it."""
    import torch
    from sparsearray_amd.device import DeviceCSC, _lib, colmedians, colquantiles
    nrow = 3000
    cp, ri, v = random_csc(nrow, ncol, 0.6, seed=52)
    A = DeviceCSC.from_host(nrow, cp, ri, v)
    dense = np.zeros((nrow, ncol))
    for j in range(ncol):
        dense[ri[cp[j]:cp[j + 1]], j] = v[cp[j]:cp[j + 1]]
    probs = (0.25, 0.5, 0.75, 0.1)
    runs = (
        (_lib().svt_dev_colmedians_ws_bytes(A.nnz, ncol), ncol * 28 + 1024, lambda ws: colmedians(A, ws=ws),
         _dense_colmedians(dense, False)),
        (_lib().svt_dev_colquantiles_ws_bytes(A.nnz, ncol, len(probs)), ncol * 44 + 1024,
         lambda ws: colquantiles(A, probs, ws=ws).T, dense_colquantiles(dense, probs, False)),
    )
    for nbytes, advertised, run, want in runs:
        assert nbytes == advertised
        pad = 519
        arena = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = arena[pad:pad + nbytes]
        assert_equal(run(ws).cpu().numpy(), want, tol=0, strict_na=True, what=f"ncol={ncol}")
        assert bool((arena[:pad] == 0xA5).all()) and bool((arena[pad + nbytes:] == 0xA5).all())
        with pytest.raises(SparseArrayError, match="workspace too small"):
            run(ws[:nbytes - 1])
