"""The reference itself against the exact result: every case of stats_cases.py through the CPU oracle, held to the
rounding bounds of exact_stats.py (no exclusions: a bound the sequential reference misses is a wrong bound); mutants
that the 1e-6 parity bar lets through and these bounds must not; and the exact helper on hand-computed columns."""
from fractions import Fraction

import numpy as np
import pytest

import exact_stats as ex
import stats_cases as sc
from sparsearray_amd import NA_real

COLUMN_PARAMS = [(n, p) for n in sc.COLUMN_FORMS for p in sc.COLUMN_PALETTES[n]]
ROW_PARAMS = [(n, p) for n in sc.ROW_ROUTES for p in sc.ROW_PALETTES[n]]


@pytest.mark.parametrize("name,palette", COLUMN_PARAMS)
def test_oracle_column_forms(oracle, name, palette):
    c = sc.column_case(name, palette)
    sc.assert_column_form(c)
    sc.run_column_case(oracle, c)
    sc.run_summary_case(oracle, c)
    if c.inner == 1 and c.type == "double" and not c.planted and palette != "e":
        sc.run_dgc_case(oracle, c)


@pytest.mark.parametrize("name,palette", ROW_PARAMS)
def test_oracle_row_routes(oracle, name, palette):
    c = sc.row_case(name, palette)
    sc.assert_row_forms(c)
    sc.run_row_case(oracle, c)


@pytest.mark.parametrize("nrow", [300, 2000])
def test_oracle_offset_and_product_palettes(oracle, nrow):
    """Full columns: 1e8 + N(0,1), where a one-pass variance has no correct digit and the two-pass form keeps the bound;
    1e3 + N(0,1) for the expanded row form; products of +-(1 + t)."""
    c = sc.full_case(nrow, "b_col")
    for op in ("sum", "mean", "var1", "sd1", "centered_X2_sum"):
        center = c.center if op == "centered_X2_sum" else None
        sc.check_stat(op, oracle._colStats(op, c.x, False, center, 1), c.cells[False], None, None, center=center,
                      what=f"full{nrow} b_col")
    sc.run_dgc_case(oracle, c)
    r = sc.full_case(nrow, "b_row")
    t = r.x.t()                                             # rows of t(x) = the columns of x
    cells = r.cells[False]
    sc.check_stat("var1", oracle.rowVars(t), cells, None, None, rows=True, what=f"full{nrow} b_row")
    sc.check_stat("sd1", oracle.rowSds(t), cells, None, None, rows=True, what=f"full{nrow} b_row")
    cen = np.full(8, r.center)
    sc.check_stat("centered_X2_sum", oracle._rowStats("centered_X2_sum", t, False, cen, 1), cells, None, None,
                  center=cen, rows=True, what=f"full{nrow} b_row")
    g = sc.full_case(nrow, "g")
    sc.check_stat("prod", oracle.colProds(g.x), g.cells[False], None, None, what=f"full{nrow} g")
    sc.check_stat("prod", oracle.rowProds(g.x.t()), g.cells[False], None, None, what=f"full{nrow} g rows")
    sc.check_stat("prod", np.asarray(oracle.prod(sc.full_case(nrow // 10, "g").x)).reshape(1),
                  _whole(sc.full_case(nrow // 10, "g")), None, None, what="prod()")


def _whole(c):
    return ex.Cells(c.val, np.zeros(len(c.val), np.int64), 1, len(c.val))


def test_oracle_overflowing_sums(oracle):
    """All-positive values near 2**1023: every order gives +Inf for a sum of two or more; the centred statistics of such
    a column are Inf - Inf."""
    c = sc.full_case(300, "overflow")
    assert np.all(np.asarray(oracle.colSums(c.x)) == np.inf)
    assert np.all(np.asarray(oracle.colMeans(c.x)) == np.inf)
    with np.errstate(all="ignore"):
        assert np.all(np.isnan(oracle.colVars(c.x))) and np.all(np.isnan(oracle.colSds(c.x)))
        assert np.all(np.asarray(oracle.rowSums(c.x)) == np.inf)


@pytest.mark.parametrize("ngroup", [3, 1000])
@pytest.mark.parametrize("palette", ["a", "c_up", "c_down", "d"])
def test_oracle_rowsum_colsum(oracle, palette, ngroup):
    sc.run_groupsum_case(oracle, sc.groupsum_case(palette, ngroup))


# ---------------------------------------------------------------------------
# the bounds have teeth
# ---------------------------------------------------------------------------
def _columns(c):
    cp = c.col_ptr[::c.inner]
    return [c.val[cp[g]:cp[g + 1]] for g in range(c.nseg)]


@pytest.mark.parametrize("palette", ["a", "d"])
@pytest.mark.parametrize("name", ["lanes16", "thread"])
def test_mutants_fail(name, palette):
    """Four wrong kernels, each within 1e-6 of the reference on most inputs: an accumulator in float32, a sum that drops
    its smallest element, a variance without the implicit zeros' term c * c * Z, a minimum that forgets the implicit
    zero.  None may pass."""
    c = sc.column_case(name, palette)
    cells = c.cells[True]                                   # (na_rm: the planted values are out of the way)
    cols = [v[~np.isnan(v)] for v in _columns(c)]
    import math
    right = np.array([math.fsum(v) for v in cols])
    assert ex.check_sum(right, cells).ok

    f32 = np.array([float(np.sum(v.astype(np.float32), dtype=np.float32)) if len(v) else 0.0 for v in cols])
    assert not ex.check_sum(f32, cells).ok, "a float32 accumulator passes"

    dropped = np.array([math.fsum(np.delete(v, np.argmin(np.abs(v)))) if len(v) else 0.0 for v in cols])
    assert not ex.check_sum(dropped, cells).ok, "a sum without its smallest element passes"

    N = cells.N.astype(np.float64)
    mu = right / N
    with np.errstate(all="ignore"):
        no_zero_term = np.array([math.fsum((v - m) ** 2) for v, m in zip(cols, mu)]) / (N - 1.0)
        full = no_zero_term + mu * mu * cells.Z / (N - 1.0)
    assert ex.check_col_centered(full, cells, op="var1").ok
    assert not ex.check_col_centered(no_zero_term, cells, op="var1").ok, "a variance without c * c * zeros passes"

    if name == "thread":        # (columns of one to three values: some are all positive; of 40 values, hardly any)
        no_zero_min = np.array([v.min() if len(v) else 0.0 for v in cols])
        with pytest.raises(AssertionError):
            ex.check_identical(no_zero_min, ex.exact_minmax(cells, True), "min")


# ---------------------------------------------------------------------------
# the exact helper on columns worked out by hand
# ---------------------------------------------------------------------------
def test_exact_helper_by_hand():
    """Three columns of 5 rows: (1, 2, 4), (0.1, -0.1, 2**-60), and one with an NA.
    (1, 2, 4, 0, 0): S = 7, A = 7, Q = 21, T = 21 - 49 / 5 = 56 / 5, var = 14 / 5.
    (0.1, -0.1, 2**-60): S = 2**-60 exactly, A = 2 * double(0.1) + 2**-60.
    (3, NA): na_rm off -> NA; na_rm on -> n = 1, N = 4, S = 3, T = 9 - 9 / 4 = 27 / 4."""
    cp = np.array([0, 3, 6, 8])
    val = np.array([1.0, 2.0, 4.0, 0.1, -0.1, 2.0 ** -60, 3.0, NA_real])
    assert ex.ExactVec.from_float(np.array([0.1, 5e-324, -1.5])).to_fractions() == \
        [Fraction(0.1), Fraction(5e-324), Fraction(-3, 2)]
    for na_rm in (False, True):
        c = ex.column_cells(cp, val, 5, na_rm=na_rm)
        S, A, Q = c.S.to_fractions(), c.A.to_fractions(), c.Q.to_fractions()
        assert (S[0], A[0], Q[0]) == (7, 7, 21) and list(c.n[:2]) == [3, 3] and list(c.Z) == [2, 2, 3]
        assert S[1] == Fraction(2) ** -60 and A[1] == 2 * Fraction(0.1) + Fraction(2) ** -60
        assert list(c.poisoned) == [False, False, not na_rm] and list(c.N) == [5, 5, 4 if na_rm else 5]
        assert (S[2], Q[2], c.n[2], c.r[2]) == (3, 9, 1, 1)
        var = np.array([14 / 5, 0.0, 0.0])
        v = ex.check_col_centered(np.where(c.poisoned, np.nan, var), c, op="var1")
        assert not v.ok                                     # columns 1 and 2 are not 0 ...
        var[1] = float((Q[1] - S[1] ** 2 / 5) / 4)
        var[2] = float(Fraction(27, 4) / 3) if na_rm else np.nan
        assert ex.check_col_centered(var, c, op="var1").ok
        assert ex.check_col_centered(np.sqrt(var), c, op="sd1").ok
        sums = np.array([7.0, 2.0 ** -60, np.nan if not na_rm else 3.0])
        assert ex.check_sum(sums, c).ok and ex.check_sum(sums, c).worst == 0.0
        off = sums.copy()
        off[0] = 7.0 + 2.0 ** -50                           # one ulp, 8.9e-16 <= gamma(2) * 7 = 1.55e-15
        assert ex.check_sum(off, c).ok
        off[0] = 7.0 + 2.0 ** -49                           # two: 1.78e-15
        assert not ex.check_sum(off, c).ok
        off[0] = 7.0
        off[1] = 2.0 ** -60 + 2.0 ** -55                    # err 2.8e-17 <= gamma(2) * 0.2 = 4.4e-17
        assert ex.check_sum(off, c).ok and 0.5 < ex.check_sum(off, c).worst < 1.0
        assert list(ex.exact_minmax(c, True)[:2]) == [0.0, -0.1] and list(ex.exact_minmax(c, False)[:2]) == [4.0, 0.1]
        assert list(ex.exact_count_nas(c)) == [0, 0, 1]
    g = ex.gamma(np.array([2])).to_fractions()[0]
    assert g == Fraction(2, 2 ** 53 - 2)
