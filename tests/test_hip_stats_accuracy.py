"""The statistics kernels against the exact result: the cases of stats_cases.py (skewed column lengths for every launch
form of the column statistics, one shape per route of the row statistics, the value palettes) through the host entry
points and through the device level, held to the rounding bounds of exact_stats.py.  test_stats_accuracy_cpu.py holds
the CPU reference to the same bounds and shows what they reject; the 1e-6 bar of the oracle-parity tests is a
different, much wider rule."""
import numpy as np
import pytest

import exact_stats as ex
import stats_cases as sc

pytestmark = pytest.mark.gpu

COLUMN_PARAMS = [(n, p) for n in sc.COLUMN_FORMS for p in sc.COLUMN_PALETTES[n]]
ROW_PARAMS = [(n, p) for n in sc.ROW_ROUTES for p in sc.ROW_PALETTES[n]]


def device_colstat(c):
    """colstats() of the case as a resident operand: f(op, na_rm, center) -> (host array, warn word set)."""
    from sparsearray_amd import device
    A = device.DeviceCSC.from_host(c.nrow, c.col_ptr, c.row_idx, c.val)
    assert device.colstats_form(A, c.inner)[0] == c.form

    def f(op, na_rm, center):
        out, warn = device.colstats(A, op, na_rm, float("nan") if center is None else float(center), c.inner)
        return out.cpu().numpy(), bool(warn.cpu().numpy().any())
    return f


def device_rowstat(c):
    """rowstats() of the case as a resident operand; None where the device level does not serve the operation (more
    than 65535 output columns: the six operations of the reference only)."""
    import torch
    from sparsearray_amd import device
    from sparsearray_amd.api import SparseArrayUnsupported
    A = device.DeviceCSC.from_host(c.nrow, c.col_ptr, c.row_idx, c.val)

    def f(op, na_rm, center):
        cen = None if center is None else torch.as_tensor(np.ascontiguousarray(center), device="cuda")
        try:
            out, _ = device.rowstats(A, op, na_rm, cen, c.inner)
        except SparseArrayUnsupported:
            assert c.inner > 65535 and op in ("mean", "var1", "sd1", "range", "prod")
            return None
        return out.cpu().numpy().reshape(-1)
    return f


@pytest.mark.parametrize("name,palette", COLUMN_PARAMS)
def test_column_forms(hip, name, palette):
    """Every column statistic, the whole-array summaries and the dgCMatrix column statistics of one skewed case: host
    entry points, then svt_dev_colstats on the resident operand."""
    c = sc.column_case(name, palette)
    sc.assert_column_form(c)
    sc.run_column_case(hip, c)
    sc.run_summary_case(hip, c)
    if c.inner == 1 and c.type == "double" and not c.planted and palette != "e":
        sc.run_dgc_case(hip, c)
    if not c.na_bg:                  # (a resident NaArray operand cannot be stated at the device level)
        sc.run_column_case(None, c, colstat=device_colstat(c))


@pytest.mark.parametrize("name,palette", ROW_PARAMS)
def test_row_routes(hip, name, palette):
    c = sc.row_case(name, palette)
    sc.assert_row_forms(c)
    sc.run_row_case(hip, c)
    sc.run_row_case(None, c, rowstat=device_rowstat(c))


@pytest.mark.parametrize("nrow", [300, 2000])
def test_offset_and_product_palettes(hip, nrow):
    """Full columns of 1e8 + N(0,1) through the two-pass column variance, of 1e3 + N(0,1) through the expanded row form,
    and products of +-(1 + t)."""
    c = sc.full_case(nrow, "b_col")
    for op in ("sum", "mean", "var1", "sd1", "centered_X2_sum"):
        center = c.center if op == "centered_X2_sum" else None
        sc.check_stat(op, hip._colStats(op, c.x, False, center, 1), c.cells[False], None, None, center=center,
                      what=f"full{nrow} b_col")
    sc.run_dgc_case(hip, c)
    r = sc.full_case(nrow, "b_row")
    t = r.x.t()                                             # rows of t(x) = the columns of x
    cells = r.cells[False]
    sc.check_stat("var1", hip.rowVars(t), cells, None, None, rows=True, what=f"full{nrow} b_row")
    sc.check_stat("sd1", hip.rowSds(t), cells, None, None, rows=True, what=f"full{nrow} b_row")
    cen = np.full(8, r.center)
    sc.check_stat("centered_X2_sum", hip._rowStats("centered_X2_sum", t, False, cen, 1), cells, None, None,
                  center=cen, rows=True, what=f"full{nrow} b_row")
    g = sc.full_case(nrow, "g")
    sc.check_stat("prod", hip.colProds(g.x), g.cells[False], None, None, what=f"full{nrow} g")
    sc.check_stat("prod", hip.rowProds(g.x.t()), g.cells[False], None, None, what=f"full{nrow} g rows")
    small = sc.full_case(nrow // 10, "g")
    sc.check_stat("prod", np.asarray(hip.prod(small.x)).reshape(1),
                  ex.Cells(small.val, np.zeros(len(small.val), np.int64), 1, len(small.val)), None, None, what="prod()")


@pytest.mark.parametrize("name", ["full", "lanes16"])
def test_overflowing_sums_by_class(hip, oracle, name):
    """All-positive values near 2**1023: a sum of two or more is +Inf in every order, and var / sd make Inf - Inf of it.
    No bound applies: the class of every result (finite value, +-Inf, NaN) is the reference's."""
    c = sc.full_case(300, "overflow") if name == "full" else sc.column_case("lanes16", "overflow")
    for op in ("colSums", "colMeans", "colVars", "colSds", "rowSums"):
        with np.errstate(all="ignore"):
            got, want = np.asarray(getattr(hip, op)(c.x)), np.asarray(getattr(oracle, op)(c.x))
        assert np.array_equal(np.isnan(got), np.isnan(want)), op
        inf = np.isinf(want)
        assert np.array_equal(got[inf], want[inf]), op
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), op


@pytest.mark.parametrize("ngroup", [3, 1000])
@pytest.mark.parametrize("palette", ["a", "c_up", "c_down", "d"])
def test_rowsum_colsum(hip, palette, ngroup):
    sc.run_groupsum_case(hip, sc.groupsum_case(palette, ngroup))
