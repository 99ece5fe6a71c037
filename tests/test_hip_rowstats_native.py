"""rowAnys / rowAlls / rowProds / rowMeans / rowVars / rowSds / rowRanges in one call each (svt_rowStatsFull_SVT,
svt_dev_rowstats; the any / all / prod / range rules of kernels_rowstats.hip and the fused mean / var1 / sd1 driver).

The yardstick is the oracle session: it has no such entry point, so it takes the route of the R methods (aperm() +
colStats, rowSums / rowCountNAs / centered_X2_sum composed on the host).

Operands: the smallest at which the LDS row-panel form can go wrong -- 5000 rows are three 2048-row panels, the last
one partial; 4500 x 6 x 5 gives inner > 1 (dims = 2) and nstrata > 1 both ways.  Forced cells: row 0 has no entry;
rows 1 to 4 are stored in every leaf (row 1 with an NA on request, row 3 with a stored zero for ints, row 4 with an
Inf for doubles); row 2049 is the first row of a panel; the last row has an NA.

Tolerances are those tests/test_hip_vs_oracle.py uses for the same quantities: tol = 1e-9, atol = 1e-9 for double
reductions formed in another order, strict NA / NaN class for ranges; integer work is bit-exact."""
import ctypes
import warnings

import numpy as np
import pytest

from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SVT_SparseArray, is_NA_real
from sparsearray_amd.api import OPCODES, Session
from sparsearray_amd.svt import make_view
from helpers import assert_equal, assert_identical

pytestmark = pytest.mark.gpu

GENERICS = ["rowAnys", "rowAlls", "rowProds", "rowMeans", "rowVars", "rowSds", "rowRanges"]
SHAPES = {"2d-0.3": ((5000, 37), 0.3, False), "2d-0.9": ((5000, 37), 0.9, True),
          "3d": ((4500, 6, 5), 0.4, True)}
_cache = {}


def _operand(shape, kind, lacunar, na_background=False):
    """(leaves built by hand: a stored zero and a lacunar leaf cannot come from a dense array)"""
    key = (shape, kind, lacunar, na_background)
    if key in _cache:
        return _cache[key]
    dim, density, row1_na = SHAPES[shape]
    nrow, nleaves = dim[0], int(np.prod(dim[1:]))
    rng = np.random.default_rng(sum(map(ord, shape + kind)))
    mask = rng.random((nrow, nleaves)) < density
    mask[0, :] = False
    mask[1:5, :] = True
    mask[2049, ::2] = True
    mask[11, 0], mask[11, 1] = True, False
    mask[[10, nrow - 1], 0] = True
    if kind == "double":
        V = rng.uniform(0.5, 2.0, (nrow, nleaves))
        V[4, 0] = np.inf                                     # in a fully covered row
        V[11, 0] = np.inf                                    # in a row that also has an implicit zero
        V[10, 0] = np.nan
        na = NA_real
    else:
        V = (rng.integers(1, 20, (nrow, nleaves)) if kind == "integer" else np.ones((nrow, nleaves))).astype(np.int32)
        V[3, 1] = 0                                          # a stored zero in a fully covered row
        V[2049, 0] = 0
        na = NA_integer
    V[nrow - 1, 0] = na
    if row1_na:
        V[1, 0] = na
    if lacunar:                                              # every third leaf all ones (no forced cell lives there)
        V[:, 2::3] = 1
    if na_background:                                        # the leaves of a NaArray hold the non-NA entries
        mask &= ~is_NA_real(V) if kind == "double" else V != NA_integer
    leaves = []
    for j in range(nleaves):
        offs = np.flatnonzero(mask[:, j]).astype(np.int32)
        vals = np.ascontiguousarray(V[offs, j])
        leaves.append((offs, None if lacunar and np.all(vals == 1) else vals))
    x = SVT_SparseArray(dim, kind, leaves, na_background=na_background)
    assert (not lacunar) or any(lf[1] is None for lf in leaves)
    _cache[key] = x
    return x


def _dims_of(shape):
    return [1] if shape.startswith("2d") else [1, 2]


@pytest.mark.parametrize("lacunar", [False, True])
@pytest.mark.parametrize("kind", ["integer", "logical"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_int_and_logical_operands(hip, oracle, shape, kind, lacunar):
    x = _operand(shape, kind, lacunar)
    for dims in _dims_of(shape):
        for na_rm in (False, True):
            what = f"{shape} {kind} dims={dims} na_rm={na_rm}"
            for fn in ("rowAnys", "rowAlls", "rowRanges"):
                assert_identical(getattr(hip, fn)(x, na_rm=na_rm, dims=dims),
                                 getattr(oracle, fn)(x, na_rm=na_rm, dims=dims), f"{fn} {what}")
            for fn in ("rowProds", "rowMeans", "rowVars", "rowSds"):
                assert_equal(getattr(hip, fn)(x, na_rm=na_rm, dims=dims),
                             getattr(oracle, fn)(x, na_rm=na_rm, dims=dims), tol=1e-9, atol=1e-9, what=f"{fn} {what}")


@pytest.mark.parametrize("lacunar", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_double_operands(hip, oracle, shape, lacunar):
    x = _operand(shape, "double", lacunar)
    for dims in _dims_of(shape):
        for na_rm in (False, True):
            what = f"{shape} dims={dims} na_rm={na_rm}"
            assert_equal(hip.rowRanges(x, na_rm=na_rm, dims=dims), oracle.rowRanges(x, na_rm=na_rm, dims=dims),
                         tol=1e-9, atol=1e-9, strict_na=True, what=f"rowRanges {what}")
            for fn in ("rowMeans", "rowVars", "rowSds", "rowProds"):
                assert_equal(getattr(hip, fn)(x, na_rm=na_rm, dims=dims),
                             getattr(oracle, fn)(x, na_rm=na_rm, dims=dims), tol=1e-9, atol=1e-9, what=f"{fn} {what}")


def test_double_any_all_still_refused(hip):
    x = _operand("2d-0.3", "double", False)
    for fn in ("rowAnys", "rowAlls"):
        with pytest.raises(SparseArrayError, match="does not support"):
            getattr(hip, fn)(x)


def test_rowprods_exact_whatever_the_order(hip, oracle):
    """Powers of two with either sign over 64 strata: every order of the multiplications gives the same bits."""
    rng = np.random.default_rng(64)
    nrow, ncol = 4100, 64
    mask = rng.random((nrow, ncol)) < 0.9
    mask[0, :] = False
    mask[1:3, :] = True
    V = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), (nrow, ncol))
    V[2, 5] = NA_real
    d = np.asfortranarray(np.where(mask, V, 0.0))
    x = SVT_SparseArray.from_dense(d, type="double")
    for na_rm in (False, True):
        assert_identical(hip.rowProds(x, na_rm=na_rm), oracle.rowProds(x, na_rm=na_rm), f"na_rm={na_rm}")
    full = np.flatnonzero(mask.all(axis=1) & ~np.isnan(V).any(axis=1))
    assert full.size > 0 and np.all(hip.rowProds(x)[full] != 0.0)


@pytest.mark.parametrize("shape,dims", [("2d-0.3", 1), ("3d", 2)])
def test_rowvars_with_a_center(hip, oracle, shape, dims):
    x = _operand(shape, "double", False)
    rng = np.random.default_rng(3)
    vec = rng.uniform(0.0, 1.0, x.dim[:dims])
    for center in (vec if dims > 1 else vec.reshape(-1), 0.75):
        for na_rm in (False, True):
            for fn in ("rowVars", "rowSds"):
                assert_equal(getattr(hip, fn)(x, na_rm=na_rm, center=center, dims=dims),
                             getattr(oracle, fn)(x, na_rm=na_rm, center=center, dims=dims),
                             tol=1e-9, atol=1e-9, what=f"{fn} {shape} na_rm={na_rm}")


@pytest.mark.parametrize("kind", ["integer", "double"])
def test_naarray_operand(hip, oracle, kind):
    x = _operand("2d-0.3", kind, False, na_background=True)
    x3 = _operand("3d", kind, False, na_background=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for y, dims in ((x, 1), (x3, 1), (x3, 2)):
            for na_rm in (False, True):
                got = hip.rowRanges(y, na_rm=na_rm, dims=dims)
                stacked = np.stack([hip.rowMins(y, na_rm=na_rm, dims=dims), hip.rowMaxs(y, na_rm=na_rm, dims=dims)],
                                   axis=-1)
                assert_identical(got, stacked, f"rowRanges NaArray {kind} dims={dims} na_rm={na_rm}")
                want = oracle.rowRanges(y, na_rm=na_rm, dims=dims)
                if kind == "double":
                    assert_equal(got, want, tol=1e-9, atol=1e-9, strict_na=True)
                else:
                    assert_identical(got, want)
    with pytest.raises(SparseArrayError, match="unable to find an inherited method"):
        hip.rowAnys(x)


class _Recorder:
    def __init__(self, inner):
        self._inner = inner
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append(name)
        return self._inner(name, *args)

    def __getattr__(self, name):
        return getattr(self._inner, name)


def test_one_call_per_generic(hip):
    rec = _Recorder(hip._call)
    s = Session(rec)
    for kind in ("integer", "double"):
        x = _operand("3d", kind, False)
        for fn in GENERICS:
            if kind == "double" and fn in ("rowAnys", "rowAlls"):
                continue
            for dims in (1, 2):
                for na_rm in (False, True):
                    rec.calls.clear()
                    getattr(s, fn)(x, na_rm=na_rm, dims=dims)
                    assert rec.calls == ["C_rowStatsFull_SVT"], (fn, kind, dims, na_rm, rec.calls)


def test_more_than_65535_output_columns(hip, oracle):
    """65536 output columns: the added operations answer "not supported here" (status > 0) at both levels and the
    generics fall back to the composition; the six operations of C_rowStats_SVT take the memory-atomic route."""
    from sparsearray_amd import device
    from sparsearray_amd.api import SparseArrayUnsupported
    dim = (2, 65536, 1)                                      # (the fewest leaves that give 65536 columns)
    rng = np.random.default_rng(65536)
    d = np.asfortranarray(np.where(rng.random(dim) < 0.5, rng.uniform(0.5, 2.0, dim), 0.0))
    d[1, 7, 0] = NA_real
    x = SVT_SparseArray.from_dense(d, type="double")
    rec = _Recorder(hip._call)
    s = Session(rec)
    for fn in ("rowProds", "rowRanges"):
        rec.calls.clear()
        got = getattr(s, fn)(x, dims=2)
        assert rec.calls[0] == "C_rowStatsFull_SVT" and rec.calls.count("C_rowStatsFull_SVT") == 1 and len(rec.calls) > 1
        assert_equal(got, getattr(oracle, fn)(x, dims=2), tol=1e-9, atol=1e-9, strict_na=fn == "rowRanges", what=fn)
    lib = _raw()
    view = make_view(x)
    out = np.zeros(2 * 2 * 65536, dtype=np.float64)          # (room for range)
    warn = ctypes.c_int(0)
    for op in ("prod", "range", "sd1"):
        assert lib.svt_rowStatsFull_SVT(ctypes.addressof(view), OPCODES[op], 0, None, 2, out.ctypes.data,
                                        ctypes.byref(warn)) == 1, op
    cp, ri, v = x.to_csc()
    A = device.DeviceCSC.from_host(2, cp, ri, v)
    for op in ("prod", "range", "mean"):
        with pytest.raises(SparseArrayUnsupported):
            device.rowstats(A, op, inner=65536)
    got, _ = device.rowstats(A, "max", inner=65536)
    assert_equal(got.cpu().numpy(), oracle.rowMaxs(x, dims=2), tol=1e-9, atol=1e-9, strict_na=True, what="max")


def _raw():
    from sparsearray_amd import _hip
    return _hip.init()


def test_raw_c_abi(hip):
    lib = _raw()
    assert hasattr(lib, "svt_rowStatsFull_SVT")
    x = _operand("2d-0.3", "double", False)
    view = make_view(x)
    out = np.zeros(2 * x.dim[0], dtype=np.float64)
    warn = ctypes.c_int(0)
    args = (None, 1, out.ctypes.data, ctypes.byref(warn))
    assert lib.svt_rowStatsFull_SVT(ctypes.addressof(view), OPCODES["prod"], 0, *args) == 0, lib.svt_last_error()
    assert_equal(out[:x.dim[0]], hip.rowProds(x), tol=1e-9, atol=1e-9)
    assert lib.svt_rowStatsFull_SVT(ctypes.addressof(view), OPCODES["any"], 0, *args) == -1
    assert "does not support" in lib.svt_last_error().decode()
    assert lib.svt_rowStats_SVT(ctypes.addressof(view), OPCODES["prod"], 0, *args) == -1
    assert "operation not supported" in lib.svt_last_error().decode()


ALL_OPS = ["countNAs", "anyNA", "min", "max", "sum", "centered_X2_sum", "any", "all", "prod", "range", "mean",
           "var1", "sd1"]


@pytest.mark.parametrize("shape,dims", [("2d-0.9", 1), ("3d", 2)])
@pytest.mark.parametrize("kind", ["integer", "double"])
def test_device_level_matches_the_host_entry_point(hip, shape, dims, kind):
    import torch
    from sparsearray_amd import device
    x = _operand(shape, kind, False)
    cp, ri, v = x.to_csc()
    A = device.DeviceCSC.from_host(x.dim[0], cp, ri, v)
    inner = int(np.prod(x.dim[1:dims]))
    n = inner * x.dim[0]
    center = np.random.default_rng(5).uniform(0.0, 1.0, n)
    dcenter = torch.as_tensor(center, device=A.val.device)
    for op in ALL_OPS:
        if kind == "double" and op in ("any", "all"):
            with pytest.raises(SparseArrayError, match="does not support"):
                device.rowstats(A, op, inner=inner)
            continue
        for na_rm in (False, True):
            for c, dc in ((None, None), (center, dcenter)) if op in ("centered_X2_sum", "var1", "sd1") else ((None, None),):
                got, warn = device.rowstats(A, op, na_rm=na_rm, center=dc, inner=inner)
                want, hwarn = hip._call("C_rowStatsFull_SVT", x, op, na_rm, c, dims)
                got = got.cpu().numpy().reshape(-1)
                what = f"{op} {kind} {shape} na_rm={na_rm} center={'yes' if c is not None else 'no'}"
                if want.dtype == np.int32:
                    assert_identical(got, want, what)
                else:
                    assert_equal(got, want, tol=1e-9, atol=1e-9, strict_na=True, what=what)
                assert bool(int(warn.item())) == hwarn, what


def test_second_call_finds_the_resident_operand(hip):
    x = _operand("3d", "double", True)
    try:
        hip.resident_set_limit(1 << 28)
        first = hip.rowProds(x, dims=2)
        base = hip.resident_stats()
        second = hip.rowVars(x, na_rm=True, dims=2)
        st = hip.resident_stats()
        assert st["hits"] == base["hits"] + 1 and st["misses"] == base["misses"]
        assert first.shape == second.shape == x.dim[:2]
    finally:
        hip.resident_set_limit(0)
        hip.resident_clear()
