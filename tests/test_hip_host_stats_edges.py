"""The branches of the host-level statistics entry points (svt_hip.cpp, "Host level: stats") that no other test enters:
zero extents, the six-operation row entry past 65535 output columns, and which check answers when two would refuse.

Zero extents: all-zero operands, so every result is a fill, a zero, an infinity or a NaN -- no arithmetic happens and the
comparison with the oracle is exact (integers identical, doubles at tolerance 0 with the NA / NaN class).  The oracle
has no C_rowStatsFull_SVT; its row methods (rowRanges, rowVars, ...) are the yardstick for that entry point.

65536 output columns: the operand of test_hip_rowstats_native.py::test_more_than_65535_output_columns and its
tolerance (double sums formed in another order)."""
import ctypes
import warnings

import numpy as np
import pytest

from sparsearray_amd import NA_real, SparseArrayError, SVT_SparseArray
from sparsearray_amd.api import OPCODES
from sparsearray_amd.svt import make_view
from helpers import assert_equal, assert_identical

pytestmark = pytest.mark.gpu

ZERO_DIMS = [(3, 0), (0, 4), (3, 2, 0), (0, 2, 2), (3, 4, 0, 2)]
KINDS = ["double", "integer"]
SIX_OPS = ["countNAs", "anyNA", "min", "max", "sum", "centered_X2_sum"]
FULL_METHODS = {"countNAs": "rowCountNAs", "anyNA": "rowAnyNAs", "min": "rowMins", "max": "rowMaxs", "sum": "rowSums",
                "any": "rowAnys", "all": "rowAlls", "prod": "rowProds", "range": "rowRanges", "mean": "rowMeans",
                "var1": "rowVars", "sd1": "rowSds"}
COERCION = "NAs introduced by coercion"


def _zeros(dim, kind):
    return SVT_SparseArray.from_dense(np.zeros(dim, dtype=np.float64 if kind == "double" else np.int32, order="F"),
                                      type=kind)


def _same(got, want, what):
    """Result and shape as the oracle's: integers identical, doubles identical too (tolerance 0, NA / NaN class)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if want.dtype == np.float64:
        assert_equal(got, want, tol=0.0, atol=0.0, strict_na=True, what=what)
    else:
        assert_identical(got.astype(np.int32), want.astype(np.int32), what)


def _warned(fn):
    """(result of fn(), whether it gave the integer-coercion warning)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = fn()
    return res, any(COERCION in str(m.message) for m in w)


def _row_method(session, op, x, na_rm, dims):
    if op in ("countNAs", "anyNA"):                                  # (no na.rm argument)
        return getattr(session, FULL_METHODS[op])(x, dims=dims)
    return getattr(session, FULL_METHODS[op])(x, na_rm=na_rm, dims=dims)


def _center(x, dims):
    return np.full(x.dim[:dims], 0.5, order="F")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", ZERO_DIMS, ids=str)
def test_zero_extent_row_stats_six(hip, oracle, dim, kind):
    x = _zeros(dim, kind)
    for dims in range(1, x.ndim):
        for op in SIX_OPS:
            center = _center(x, dims) if op == "centered_X2_sum" else None
            for na_rm in (False, True):
                what = f"C_rowStats_SVT {op} {kind} {dim} dims={dims} na_rm={na_rm}"
                got, gwarn = hip._call("C_rowStats_SVT", x, op, na_rm, center, dims)
                want, wwarn = oracle._call("C_rowStats_SVT", x, op, na_rm, center, dims)
                _same(got, want, what)
                assert gwarn == wwarn, f"{what}: warn {gwarn} != {wwarn}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", ZERO_DIMS, ids=str)
def test_zero_extent_row_stats_full(hip, oracle, dim, kind):
    x = _zeros(dim, kind)
    for dims in range(1, x.ndim):
        for op in list(FULL_METHODS) + ["centered_X2_sum"]:
            for na_rm in (False, True):
                what = f"C_rowStatsFull_SVT {op} {kind} {dim} dims={dims} na_rm={na_rm}"
                if kind == "double" and op in ("any", "all"):        # refused for doubles, whatever the extents
                    with pytest.raises(SparseArrayError, match="does not support"):
                        hip._call("C_rowStatsFull_SVT", x, op, na_rm, None, dims)
                    with pytest.raises(SparseArrayError, match="does not support"):
                        _row_method(oracle, op, x, na_rm, dims)
                    continue
                if op == "centered_X2_sum":
                    center = _center(x, dims)
                    want, wwarn = _warned(lambda: oracle._rowStats(op, x, na_rm, center, dims))
                else:
                    center = None
                    want, wwarn = _warned(lambda: _row_method(oracle, op, x, na_rm, dims))
                flat, gwarn = hip._call("C_rowStatsFull_SVT", x, op, na_rm, center, dims)
                want = np.asarray(want)
                # the flat result: prod(dim[:dims]) cells column-major; "range": the minima, then as many maxima
                assert want.shape == tuple(x.dim[:dims]) + ((2,) if op == "range" else ()), what
                _same(flat, want.reshape(-1, order="F"), what)
                assert gwarn == wwarn, f"{what}: warn {gwarn} != {wwarn}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", ZERO_DIMS, ids=str)
def test_zero_extent_col_stats_and_summarize(hip, oracle, dim, kind):
    x = _zeros(dim, kind)
    for dims in range(1, x.ndim + 1):
        for op in ("sum", "min", "max", "var1", "countNAs"):
            for na_rm in (False, True):
                what = f"C_colStats_SVT {op} {kind} {dim} dims={dims} na_rm={na_rm}"
                got, gwarn = hip._call("C_colStats_SVT", x, op, na_rm, NA_real, dims)
                want, wwarn = oracle._call("C_colStats_SVT", x, op, na_rm, NA_real, dims)
                _same(got, want, what)
                assert gwarn == wwarn, f"{what}: warn {gwarn} != {wwarn}"
    for op in ("sum", "min", "range"):
        for na_rm in (False, True):
            what = f"summarize_SVT {op} {kind} {dim} na_rm={na_rm}"
            got, gwarn = _warned(lambda: hip.summarize_SVT(op, x, na_rm))
            want, wwarn = _warned(lambda: oracle.summarize_SVT(op, x, na_rm))
            _same(got, want, what)
            assert gwarn == wwarn, f"{what}: warn {gwarn} != {wwarn}"


def test_six_operations_past_65535_output_columns(hip, oracle):
    """svt_rowStats_SVT itself on the memory-atomic route.  `center` reaches centered_X2_sum and no other operation."""
    dim = (2, 65536, 1)
    rng = np.random.default_rng(65536)
    d = np.asfortranarray(np.where(rng.random(dim) < 0.5, rng.uniform(0.5, 2.0, dim), 0.0))
    d[1, 7, 0] = NA_real
    x = SVT_SparseArray.from_dense(d, type="double")
    center = np.asfortranarray(np.random.default_rng(2).uniform(0.0, 1.0, dim[:2]))
    want = {}
    for op in SIX_OPS:
        for na_rm in (False, True):
            want[op, na_rm] = oracle._call("C_rowStats_SVT", x, op, na_rm, center if op == "centered_X2_sum" else None, 2)
    for op, given in [(op, center if op == "centered_X2_sum" else None) for op in SIX_OPS] + [("sum", center)]:
        for na_rm in (False, True):
            what = f"{op} na_rm={na_rm} center={'yes' if given is not None else 'no'}"
            got, gwarn = hip._call("C_rowStats_SVT", x, op, na_rm, given, 2)
            exp, wwarn = want[op, na_rm]
            assert got.shape == exp.shape == dim[:2], what
            if exp.dtype == np.int32:
                assert_identical(got, exp, what)
            else:
                assert_equal(got, exp, tol=1e-9, atol=1e-9, strict_na=True, what=what)
            assert gwarn == wwarn, what


def _refused(lib, status, text):
    assert status == -1, status
    assert text in lib.svt_last_error().decode(), lib.svt_last_error()


def test_which_check_answers(hip):
    """Through the raw C ABI: each call below fails the named check, some a later one as well; the first one answers."""
    from sparsearray_amd import _hip
    lib = _hip.init()
    out = np.zeros(64, dtype=np.float64)
    warn = ctypes.c_int(0)
    d = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(3, 4))
    x2 = SVT_SparseArray.from_dense(d, type="double")
    v2 = make_view(x2)
    # dims = ndim, and an operation the entry point does not take
    _refused(lib, lib.svt_rowStats_SVT(ctypes.addressof(v2), OPCODES["prod"], 0, None, 2, out.ctypes.data,
                                       ctypes.byref(warn)), "'dims' must be")
    xna = SVT_SparseArray.from_dense(d, type="double", na_background=True)
    na = make_view(xna)
    center = np.zeros(3)
    _refused(lib, lib.svt_rowStats_SVT(ctypes.addressof(na), OPCODES["centered_X2_sum"], 0, center.ctypes.data, 1,
                                       out.ctypes.data, ctypes.byref(warn)), "not yet supported on NaArray")
    x3 = SVT_SparseArray.from_dense(np.asfortranarray(d.reshape(3, 2, 2, order="F")), type="double")
    v3 = make_view(x3)
    _refused(lib, lib.svt_rowMedians_SVT(ctypes.addressof(v3), 0, out.ctypes.data), "rowMedians")
    # a 3-D operand, and no such ties.method
    _refused(lib, lib.svt_rowRanks_SVT(ctypes.addressof(v3), 99, out.ctypes.data), "rowRanks")
    _refused(lib, lib.svt_colRanks_SVT(ctypes.addressof(v2), 99, 1, out.ctypes.data), "ties.method")
