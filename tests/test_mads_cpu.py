"""colMads() / rowMads(): the reference has no method; the rule is stats::mad without low / high on each column's nrow
values, the implicit zeros included (include/svt_hip.h, svt_colMads_SVT).  Here the host statement of
oracle/rules.py (what the oracle session runs: an entry point of its dispatcher) is checked against the plain
definition on the sorted dense column, at tolerance 0: both sides evaluate the same IEEE operations."""
import numpy as np
import pytest

from helpers import assert_equal
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, SparseArrayError, is_NA_real
from test_quantiles_cpu import as_float, quantile_cases

DEFAULT = 1.4826
CONSTANTS = (1.0, 0.0, -2.5)                            # next to the default


def _median(x):
    """The median's own rule on a sorted vector: the middle value, or (lo + hi) * 0.5."""
    n = x.size
    lo = x[(n - 1) >> 1]
    return lo if n & 1 else (lo + x[n >> 1]) * 0.5


def dense_colmads(a, center, constant, na_rm):
    """stats::mad(low = FALSE, high = FALSE) of every column of the dense matrix ``a`` (NaN = missing), in five steps:
    the median's NA rule; c = the given center or the median; c NA / NaN gives NA; t = |x - c|, any NaN gives NA; the
    result is constant * median(t)."""
    a = np.asarray(a, dtype=np.float64)
    ncol = a.shape[1]
    if center is not None:
        center = np.broadcast_to(np.asarray(center, dtype=np.float64), (ncol,))
    out = np.empty(ncol)
    with np.errstate(all="ignore"):
        for j in range(ncol):
            col = a[:, j]
            miss = np.isnan(col)
            if miss.any() and not na_rm:                # 1.
                out[j] = NA_real
                continue
            x = col[~miss]
            if x.size == 0:
                out[j] = NA_real
                continue
            c = _median(np.sort(x)) if center is None else center[j]     # 2.
            if np.isnan(c):                             # 3.
                out[j] = NA_real
                continue
            t = np.abs(x - c)                           # 4.
            if np.isnan(t).any():
                out[j] = NA_real
                continue
            out[j] = np.float64(constant) * _median(np.sort(t))          # 5.
    return out


def mad_cases():
    """MAD's own operands, next to the case families of the quantiles."""
    rng = np.random.default_rng(11)
    inf = np.inf
    cases = []
    for nrow in (7, 8):                                 # odd and even n; negative and half-integer medians
        a = np.zeros((nrow, 12))
        a[:, 0] = -np.arange(1, nrow + 1)               # all negative
        a[:, 1] = np.arange(nrow) - 2.0
        a[: nrow // 2 + 1, 2] = -3.0                    # bare majority of one negative value
        a[:, 3] = np.arange(nrow) * 0.5 - 1.25
        a[:4, 4] = [1, 2, 1, 2]                         # (even n: median 0.5)
        a[:, 5] = rng.integers(-4, 5, nrow)
        a[:, 6] = rng.integers(-4, 5, nrow) + 0.5
        # symmetric about the center 2: the deviations are equal in pairs
        a[:6, 7] = [2 - 3, 2 - 1, 2 + 1, 2 + 3, 2 - 0.5, 2 + 0.5]
        a[:, 8] = 2.0 + np.resize([-1.5, 1.5], nrow)
        # stored values equal to 2c (median 2 resp. center 2): t == b, they join the block
        a[:5, 9] = [2, 2, 2, 4, 4]
        a[:, 10] = np.resize([4.0, 0.0, 1.0, 4.0, 3.0], nrow)
        a[:, 11] = np.resize([-1.0, 1.0], nrow)          # median 0 (even n) without a stored zero
        cases.append((f"mad {nrow}", a, "double"))
    b = np.round(rng.normal(size=(40, 9)) * 3 + 1)
    b[rng.random(b.shape) < 0.4] = 0
    b = b.astype(np.int32)
    b[3, 1] = NA_integer
    b[:, 2] = NA_integer                                # nothing left under na.rm
    b[:30, 3] = NA_integer
    b[:, 4] = 2 * (np.arange(40) % 3)                   # 0, 2, 4: values at 2c for the center 1 and the median 2
    cases.append(("mad int 40 with NA", b, "integer"))
    c = np.zeros((5, 6))                                # infinities with and without a center that is one
    c[:, 0] = [inf, 1, 2, 3, 4]
    c[:, 1] = [-inf, 1, 2, 3, 4]
    c[:, 2] = [inf, inf, inf, 1, 0]                     # median +Inf: the deviation of +Inf is NaN
    c[:, 3] = [-inf, -inf, -inf, 1, 0]
    c[:, 4] = [1, 2, 3, 0, 0]
    c[:, 5] = [inf, -inf, np.nan, 1, 0]
    cases.append(("mad infinities", c, "double"))
    d = np.zeros((4, 2))
    d[:, 0] = [-inf, -inf, inf, inf]                    # median NaN (not NA): the result is NA
    d[:, 1] = [inf, -inf, 0, 0]
    cases.append(("mad infinite median", d, "double"))
    return cases


def all_cases():
    return quantile_cases() + mad_cases()


def center_specs(n):
    """(label, center) for a result of n entries: None, scalars (0.0, -0.0, inside, far outside, NaN, NA, +-Inf) and
    vectors, one of which mixes NaN, NA and both infinities among ordinary centers."""
    ramp = np.linspace(-2.0, 4.0, n) if n else np.zeros(0)
    mixed = np.resize(np.array([np.inf, -np.inf, np.nan, NA_real, 0.5, -0.0, 2.0]), n)
    return [("none", None), ("0.0", 0.0), ("-0.0", -0.0), ("1.5", 1.5), ("2", 2), ("1e6", 1e6), ("-1e300", -1e300),
            ("NaN", np.nan), ("NA", NA_real), ("+Inf", np.inf), ("-Inf", -np.inf), ("ramp", ramp),
            ("mixed", mixed), ("mixed reversed", mixed[::-1].copy())]


def check_mads_on_cases(session, na_rm, what, reference=None):
    """colMads / rowMads of ``session`` on every case with every center at the default constant, and with the other
    constants without a center and with a vector of centers; against dense_colmads, or against ``reference``'s."""
    for name, a, type_ in all_cases():
        x = SVT_SparseArray.from_dense(np.asfortranarray(a), type_)
        f = as_float(a, type_)
        for axis, fn, dense in ((1, "colMads", f), (0, "rowMads", f.T)):
            n = a.shape[axis]
            specs = center_specs(n)
            runs = [(lab, cen, DEFAULT) for lab, cen in specs]
            runs += [(lab, cen, k) for k in CONSTANTS for lab, cen in (specs[0], specs[11])]
            for lab, cen, k in runs:
                got = getattr(session, fn)(x, center=cen, constant=k, na_rm=na_rm)
                assert got.shape == (n,)
                if reference is None:
                    want = dense_colmads(dense, cen, k, na_rm)
                else:
                    want = getattr(reference, fn)(x, center=cen, constant=k, na_rm=na_rm)
                assert_equal(got, want, tol=0, strict_na=True, what=f"{what} {fn} {name} center={lab} constant={k}")


@pytest.mark.parametrize("na_rm", [False, True])
def test_host_statement_is_the_dense_rule(oracle, na_rm):
    check_mads_on_cases(oracle, na_rm, "oracle")


def test_defaults(oracle):
    _, a, type_ = mad_cases()[0]
    x = SVT_SparseArray.from_dense(np.asfortranarray(a), type_)
    assert_equal(oracle.colMads(x), dense_colmads(a, None, 1.4826, False), tol=0, strict_na=True)
    assert_equal(oracle.rowMads(x), dense_colmads(a.T, None, 1.4826, False), tol=0, strict_na=True)


def test_known_values(oracle):
    """Worked by hand: c(1, 2, 3, 4, 100) has median 3 and deviations 2, 1, 0, 1, 97, median 1; c(0, 0, 1, 2) has median
    0.5 and deviations 0.5, 0.5, 0.5, 1.5, median 0.5; a column whose median is +Inf is NA; a given NaN center is NA."""
    a = np.zeros((5, 3))
    a[:, 0] = [1, 2, 3, 4, 100]
    a[:, 1] = [np.inf, np.inf, np.inf, 1, 0]
    a[:, 2] = [0, 0, 0, 1, 2]
    x = SVT_SparseArray.from_dense(np.asfortranarray(a), "double")
    got = oracle.colMads(x)
    assert got[0] == 1.4826 * 1.0 and is_NA_real(got[1]) and got[2] == 0.0
    assert list(oracle.colMads(x, constant=1)[[0, 2]]) == [1.0, 0.0]
    assert list(oracle.colMads(x, center=0, constant=1)) == [3.0, np.inf, 0.0]
    assert is_NA_real(oracle.colMads(x, center=np.nan)).all()
    b = np.array([[0.0], [0.0], [1.0], [2.0]])
    assert oracle.colMads(SVT_SparseArray.from_dense(np.asfortranarray(b), "double"), constant=1)[0] == 0.5


def test_zero_extents(oracle):
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    for cen in (None, 1.0, np.array([1.0, 2.0, 3.0])):
        m = oracle.colMads(x0, center=cen)
        assert m.shape == (3,) and is_NA_real(m).all()
    assert oracle.rowMads(x0).shape == (0,)
    assert oracle.rowMads(x0, center=np.zeros(0)).shape == (0,)
    x1 = SVT_SparseArray((4, 0), "double", [])
    assert oracle.colMads(x1).shape == (0,)
    for cen in (None, 1.0, np.arange(4.0)):
        r = oracle.rowMads(x1, center=cen)
        assert r.shape == (4,) and is_NA_real(r).all()


def check_argument_errors(session):
    x = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3, 4)), "double")
    x3 = SVT_SparseArray((2, 2, 2), "double", [None] * 4)
    with pytest.raises(SparseArrayError, match=r"the colMads\(\) method for SparseArray objects only supports 2D"):
        session.colMads(x3)
    with pytest.raises(SparseArrayError, match=r"the rowMads\(\) method for SparseArray objects only supports 2D"):
        session.rowMads(x3)
    na = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3)), "double", na_background=True)
    for fn in (session.colMads, session.rowMads):
        with pytest.raises(SparseArrayError, match=r"colMads\(\) is not supported on NaArray objects"):
            fn(na)
        with pytest.raises(SparseArrayError, match="'na.rm' must be TRUE or FALSE"):
            fn(x, na_rm=1)
    per_col = "'center' must be NULL, a single number, or a vector with one element per column"
    per_row = "'center' must be NULL, a single number, or a vector with one element per row"
    for bad in (np.zeros(3), np.zeros(5), np.zeros(0), np.zeros((4, 1)), "a"):
        with pytest.raises(SparseArrayError, match=per_col):
            session.colMads(x, center=bad)
    for bad in (np.zeros(4), np.zeros(2), np.zeros((1, 3)), "median"):
        with pytest.raises(SparseArrayError, match=per_row):
            session.rowMads(x, center=bad)
    assert session.colMads(x, center=np.zeros(4)).shape == (4,)
    assert session.rowMads(x, center=[0.0, 1.0, 2.0]).shape == (3,)


def test_argument_checks(oracle):
    check_argument_errors(oracle)
