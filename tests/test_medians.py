"""colMedians() / rowMedians(): the reference computes them in R, one leaf at a time
(R/SparseArray-matrixStats.R:690-815).  The oracle restates that R code (oracle/oracle.py);
both it and the HIP path are checked against the plain definition, median of the dense column
(with R's rule: any NA/NaN -> NA unless na.rm)."""
import numpy as np
import pytest

from helpers import assert_equal
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, is_NA_real
from test_quantiles_cpu import dense_colquantiles


def _dense_colmedians(a, na_rm):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape[1])
    for j in range(a.shape[1]):
        col = a[:, j]
        miss = np.isnan(col)
        if miss.any() and not na_rm:
            out[j] = NA_real
            continue
        col = col[~miss]
        out[j] = NA_real if col.size == 0 else np.median(col)
    return out


dense_colmedians = _dense_colmedians                  # (the rule under its public name: tests/chain_cases.py)


def last_digit_columns(nrow=5000, seed=69):
    """Full columns of ``nrow`` (even) values 1 + k * 2^-52 with k < 1024: every key shares its upper 54 bits with more
    than 1024 others, so the select's bin never gets small before its last digit pass and it gives up with a handful
    of candidates (msel_select, ``shift == 0``); rank k + 1 then comes from the caller's counting pass, with the next
    key ONE ulp above.  Column 0: half the values below k = 512 and half from it on, 511 and 512 among them -- the two
    middle ranks are adjacent distinct keys; column 1: k uniform; column 2: the two middle ranks inside seven copies of
    one key."""
    rng = np.random.default_rng(seed)
    half = nrow // 2
    assert nrow % 2 == 0 and half > 1024
    k0 = np.concatenate([rng.integers(0, 512, half), rng.integers(512, 1024, half)])
    k0[0], k0[half] = 511, 512
    k1 = rng.integers(0, 1024, nrow)
    k2 = np.concatenate([rng.integers(0, 300, half - 3), np.full(7, 300), rng.integers(301, 1024, half - 4)])
    cols = np.stack([1.0 + rng.permutation(k) * 2.0 ** -52 for k in (k0, k1, k2)], axis=1)
    s = np.sort(cols, axis=0)
    assert s[half - 1, 0] == 1.0 + 511 * 2.0 ** -52 and s[half, 0] == 1.0 + 512 * 2.0 ** -52
    assert s[half - 1, 2] == s[half, 2] == 1.0 + 300 * 2.0 ** -52
    assert all(np.unique(cols[:, j], return_counts=True)[1].max() < 40 for j in range(3))
    return cols


def _cases():
    rng = np.random.default_rng(5)
    cases = []
    # man/SparseArray-matrixStats.Rd:183-187 (the 2D example object)
    m0 = np.zeros((6, 4), dtype=np.int32)
    m0.reshape(-1, order="F")[np.array([1, 2, 8, 10, 15, 16, 17, 24]) - 1] = np.arange(1, 9) * 10
    m0 = m0.reshape((6, 4), order="F") if m0.flags.f_contiguous else np.asfortranarray(m0)
    m0 = np.asfortranarray(m0)
    m0[4, 1] = NA_integer
    cases.append(("man page m0", m0, "integer"))
    for nrow in (1, 2, 7, 8):
        a = np.round(rng.normal(size=(nrow, 40)), 1)
        a[rng.random(a.shape) < 0.5] = 0.0
        cases.append((f"small {nrow}", a, "double"))
    a = np.round(rng.normal(size=(101, 60)), 2)
    a[rng.random(a.shape) < 0.6] = 0.0
    a[:, 0] = 0.0                                   # empty leaf
    a[:, 1] = np.abs(a[:, 1]) + 1                   # all positive
    a[:, 2] = -np.abs(a[:, 2]) - 1                  # all negative
    a[:51, 3] = 5.0; a[51:, 3] = 0.0                # bare majority of positives, odd n
    a[3, 4] = np.nan
    a[5, 5] = NA_real
    a[7, 6] = np.inf
    a[:, 7] = np.nan                                # nothing left under na.rm
    a[9, 8] = -np.inf
    cases.append(("mixed 101", a, "double"))
    b = a[:100].copy()                              # even n: means of two middle values
    b[:50, 9] = 2.0; b[50:, 9] = 0.0                # exactly half positive
    b[:50, 10] = -2.0; b[50:, 10] = 0.0             # exactly half negative
    b[:50, 11] = -2.0; b[50:, 11] = 3.0             # half / half, no zeros
    cases.append(("mixed 100", b, "double"))
    c = rng.integers(-5, 6, (64, 30)).astype(np.int32)
    c[rng.random(c.shape) < 0.5] = 0
    c[2, 3] = NA_integer
    cases.append(("int 64", c, "integer"))
    return cases


def _as_float(a, type_):
    f = np.asarray(a, dtype=np.float64).copy()
    if type_ == "integer":
        f[np.asarray(a) == NA_integer] = np.nan
    return f


@pytest.mark.parametrize("na_rm", [False, True])
def test_oracle_colmedians_is_the_dense_median(oracle, na_rm):
    for name, a, type_ in _cases():
        x = SVT_SparseArray.from_dense(np.asfortranarray(a), type_)
        want = _dense_colmedians(_as_float(a, type_), na_rm)
        assert_equal(oracle.colMedians(x, na_rm=na_rm), want, tol=1e-15, strict_na=True, what=name)
        want_r = _dense_colmedians(_as_float(a, type_).T, na_rm)
        assert_equal(oracle.rowMedians(x, na_rm=na_rm), want_r, tol=1e-15, strict_na=True, what=name + " rows")
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    assert is_NA_real(oracle.colMedians(x0)).all()
    with pytest.raises(Exception, match="only supports 2D"):
        oracle.colMedians(SVT_SparseArray((2, 2, 2), "double", [None] * 4))


def _check_median_keeps_its_own_finish(session):
    """The median of an even column is (lo + hi) * 0.5, the quantile at 0.5 is 0.5 * lo + 0.5 * hi: the first
    overflows where the second does not, and they round a subnormal pair differently.  Every column has four stored
    values (no zeros): on the device all three go through the select kernel."""
    big = np.array([1.5e308, 1.6e308, 1e308, 1.7e308])
    a = np.stack([big, np.array([5e-324, 1e-323, -1.0, 3.0]), -big], axis=1)
    half = dense_colquantiles(a, (0.5,), False)[:, 0]
    x = SVT_SparseArray.from_dense(np.asfortranarray(a), "double")
    xt = SVT_SparseArray.from_dense(np.asfortranarray(a.T), "double")
    with np.errstate(over="ignore"):                    # (the overflow is the point)
        med = np.array([np.median(a[:, j]) for j in range(3)])
        assert np.array_equal(med, [np.inf, 1e-323, -np.inf])
        assert (med != half).all()
        assert_equal(session.colMedians(x), med, tol=0, strict_na=True, what="colMedians")
        assert_equal(session.rowMedians(xt), med, tol=0, strict_na=True, what="rowMedians")
    assert_equal(session.colQuantiles(x, (0.5,))[:, 0], half, tol=0, strict_na=True, what="colQuantiles(0.5)")


def test_oracle_median_keeps_its_own_finish(oracle):
    _check_median_keeps_its_own_finish(oracle)


@pytest.mark.gpu
def test_hip_median_keeps_its_own_finish(hip):
    _check_median_keeps_its_own_finish(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("na_rm", [False, True])
def test_hip_colmedians(hip, oracle, na_rm):
    for name, a, type_ in _cases():
        x = SVT_SparseArray.from_dense(np.asfortranarray(a), type_)
        assert_equal(hip.colMedians(x, na_rm=na_rm), oracle.colMedians(x, na_rm=na_rm),
                     tol=1e-15, strict_na=True, what=name)
        assert_equal(hip.rowMedians(x, na_rm=na_rm), oracle.rowMedians(x, na_rm=na_rm),
                     tol=1e-15, strict_na=True, what=name + " rows")
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    assert is_NA_real(hip.colMedians(x0)).all()
    with pytest.raises(Exception, match="only supports 2D"):
        hip.colMedians(SVT_SparseArray((2, 2, 2), "double", [None] * 4))


@pytest.mark.gpu
def test_hip_colmedians_long_columns(hip):
    rng = np.random.default_rng(6)
    a = np.round(rng.normal(size=(40_001, 120)), 3)
    a[rng.random(a.shape) < 0.7] = 0.0
    a[:, 5] = np.abs(a[:, 5]) + 0.5
    a[11, 7] = np.nan
    x = SVT_SparseArray.from_dense(np.asfortranarray(a), "double")
    for na_rm in (False, True):
        assert_equal(hip.colMedians(x, na_rm=na_rm), _dense_colmedians(a, na_rm), tol=1e-15, strict_na=True)


@pytest.mark.gpu
@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_colmedians_radix_select_against_numpy(hip, type_):
    """The per-column radix select (round 5, kernels_median.hip) against the plain definition on columns where the
    median is an order statistic of the stored values: dense-ish columns of every length class (shorter than one
    sweep of the workgroup, ragged, several sweeps), heavy duplicates (the second middle value is the same key),
    values that differ only in their low bits (the last digits of the select decide), mostly negative / mostly
    positive columns, +-Inf, and NA / NaN entries under na.rm (R/SparseArray-matrixStats.R:690-784)."""
    rng = np.random.default_rng(66)
    cols = []
    nrow = 5000
    for j in range(96):
        col = np.zeros(nrow)
        fill = [1.0, 0.97, 0.8, 0.6, 0.51, 0.3][j % 6]
        m = rng.random(nrow) < fill
        kind = (j // 6) % 5
        if kind == 0:
            v = rng.normal(size=nrow)
        elif kind == 1:
            v = rng.integers(-3, 4, nrow).astype(np.float64)                    # duplicates
        elif kind == 2:
            v = 1.0 + rng.integers(0, 1 << 20, nrow) * 2.0 ** -52               # same exponent, low mantissa bits
        elif kind == 3:
            v = -np.abs(rng.normal(size=nrow)) - (j % 3)                         # negative majority
        else:
            v = np.abs(rng.normal(size=nrow)) * 1e200 * (1 if j % 2 else -1)
        if type_ == "integer":
            v = np.round(v * (1000 if kind != 2 else 1)).clip(-2e9, 2e9)
        col[m] = v[m]
        cols.append(col)
    a = np.stack(cols, axis=1)
    short = np.zeros((nrow, 6))                                                # few stored values among many zeros
    short[:3, 0] = [5, 6, 7]
    short[:nrow // 2 + 1, 1] = 2.0
    short[: nrow // 2, 2] = -2.0; short[nrow // 2:, 2] = 3.0
    short[:, 3] = np.arange(nrow) - 100.0
    short[:, 4] = np.where(np.arange(nrow) % 2 == 0, -1.0, 1.0)
    short[:, 5] = 7.0
    a = np.concatenate([a, short], axis=1)
    if type_ == "double":
        a[17, 3] = np.inf; a[18, 3] = -np.inf; a[5, 9] = np.nan; a[6, 10] = NA_real; a[:40, 11] = np.nan
        a = np.concatenate([a, last_digit_columns(nrow)], axis=1)              # the select's last digit decides nothing
        x = SVT_SparseArray.from_dense(np.asfortranarray(a), "double")
        dense = a
    else:
        ai = a.astype(np.int32)
        ai[5, 9] = NA_integer; ai[:40, 11] = NA_integer
        x = SVT_SparseArray.from_dense(np.asfortranarray(ai), "integer")
        dense = ai.astype(np.float64); dense[ai == NA_integer] = np.nan
    for na_rm in (False, True):
        got = hip.colMedians(x, na_rm=na_rm)
        want = _dense_colmedians(dense, na_rm)
        assert_equal(got, want, tol=0, strict_na=True, what=f"{type_} na_rm={na_rm}")
    # a tall column: many sweeps of one workgroup, all six digit passes with survivors
    tall = rng.normal(size=(300_000, 3))
    tall[:, 1] = np.round(tall[:, 1], 1)
    tall[rng.random(tall.shape) < 0.2] = 0.0
    xt = SVT_SparseArray.from_dense(np.asfortranarray(tall if type_ == "double" else np.round(tall * 100).astype(np.int32)), type_)
    td = tall if type_ == "double" else np.round(tall * 100)
    assert_equal(hip.colMedians(xt), _dense_colmedians(td, False), tol=0, strict_na=True, what="tall")
