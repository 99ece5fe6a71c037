"""sweep(x, MARGIN, STATS, FUN) on the GPU: the third kernel family of kernels_arith.hip through the count and fill calls
with the test's own guarded buffers, the compositions DeviceCSC.sweep, and the host entry points behind Session.sweep --
against the expectations of tests/sweep_cases.py (numpy broadcasting on the dense array, compared as bits).  No operand
has more than about three tiles of entries."""
import ctypes
import warnings

import numpy as np
import pytest

import arith_cases as ac
import compare_cases as cc
import subset_cases as sc
import sweep_cases as sw
from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SparseArrayUnsupported

torch = pytest.importorskip("torch")
from sparsearray_amd.device import arith_tile, sweep_form          # noqa: E402
pytestmark = pytest.mark.gpu

GUARD = 64          # guard words on either side of every output array
LGLSXP, INTSXP, REALSXP = 10, 13, 14
RTYPE = {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}


@pytest.fixture(scope="module")
def T(hip):
    return arith_tile()


def _device(nrow, csc, logical=False):
    from sparsearray_amd.device import DeviceCSC
    cp, ri, val = csc
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val), device="cuda"), logical=logical)


def _host(R):
    torch.cuda.synchronize()
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def _same(got, want, cls, what):
    """CSC triples: col_ptr and row_idx exactly, rows ascending in every column, values as bits by their class"""
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    starts = np.zeros(got[1].size, bool)
    starts[got[0][:-1][np.diff(got[0]) > 0]] = True
    assert np.all((np.diff(got[1]) > 0) | starts[1:]), f"{what}: rows do not ascend inside a column"
    e = ac.Expected("double" if want[2].dtype == np.float64 else "integer", want[2], cls, np.ones(want[2].shape, bool))
    ac.compare(got[2], np.ones(got[2].shape, bool), e, what)


class Guarded:
    """an output array between two bands of guard words"""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def body(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def intact(self):
        return bool((self.t[:GUARD] == self.fill).all()) and bool((self.t[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.t == self.fill).all())


class Raw:
    """One sweep through the count and fill calls with the test's own buffers: a poisoned workspace of the advertised
    size followed by a guard band, every output between guard words."""

    def __init__(self, x, op, stats, s_type, form, short=0, stats_len=None):
        from sparsearray_amd.api import ARITH_OPCODES, COMPARE_OPCODES
        from sparsearray_amd.device import _lib, _stream
        self.lib, self.stream, self.x = _lib(), _stream, x
        self.compare = op in COMPARE_OPCODES
        self.stats = torch.as_tensor(np.ascontiguousarray(stats), device="cuda")
        code = COMPARE_OPCODES[op] if self.compare else ARITH_OPCODES.get(op, op)
        self.args = (x.handle, code, self.stats.data_ptr(), RTYPE[s_type], self.stats.numel() if stats_len is None else stats_len,
                     *form)
        self.nb = self.lib.svt_dev_sweep_ws_bytes(x.ncol, x.nnz)
        self.ws = torch.full((self.nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cp = Guarded(x.ncol + 1, torch.int64, -77)
        self.nnz, self.bad, self.short = ctypes.c_int64(-5), ctypes.c_int64(-9), short
        self.ov = torch.zeros(1, dtype=torch.int32, device="cuda")

    def count(self):
        fn = self.lib.svt_dev_compare_sweep_count if self.compare else self.lib.svt_dev_arith_sweep_count
        rc = fn(*self.args, self.cp.ptr(), ctypes.byref(self.nnz), ctypes.byref(self.bad), self.ws.data_ptr(),
                self.nb - self.short, self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, dtype):
        n = max(self.nnz.value, 0)
        self.ri, self.vv = Guarded(n, torch.int32, -77), Guarded(n, dtype, 77)
        if self.compare:
            rc = self.lib.svt_dev_compare_sweep_fill(*self.args, self.cp.ptr(), self.ri.ptr(), self.vv.ptr(), self.ws.data_ptr(),
                                                     self.nb, self.stream())
        else:
            rc = self.lib.svt_dev_arith_sweep_fill(*self.args, self.cp.ptr(), self.ri.ptr(), self.vv.ptr(), self.ov.data_ptr(),
                                                   self.ws.data_ptr(), self.nb, self.stream())
        torch.cuda.synchronize()
        return rc

    def ws_guard_intact(self):
        return bool((self.ws[self.nb:] == 0xA5).all())

    def arrays(self):
        return self.cp.body(), self.ri.body(), self.vv.body()


def _run_raw(x, nrow, csc, dim, margin, op, stats, s_type, what):
    """count, fill, guards and the expectation; returns the arrays"""
    want, cls, t, over = sw.expect_csc(op, nrow, csc, dim, margin, stats, s_type)
    r = Raw(x, op, stats, s_type, sweep_form(dim, margin))
    assert r.count() == 0, (what, r.lib.svt_last_error())
    assert r.bad.value == -1 and r.nnz.value == want[1].size and np.array_equal(r.cp.body(), want[0]), f"{what}: count"
    assert r.cp.intact() and r.ws_guard_intact()
    assert r.fill(torch.float64 if t == "double" else torch.int32) == 0
    assert r.cp.intact() and r.ri.intact() and r.vv.intact() and r.ws_guard_intact(), what
    _same(r.arrays(), want, cls, what)
    assert bool(r.ov.item()) == over, f"{what}: the overflow word"
    return r.arrays(), want, cls, over


PLACEMENT = [(op, st) for op in ("*", "/") for st in ("integer", "double")]
PLACEMENT_INT = [(op, st) for op in ("%%", "%/%", "*") for st in ("integer", "double")]


# ---------------------------------------------------------------------------
# 1. placement, 2-D; 8. determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("type", ["double", "integer"])
@pytest.mark.parametrize("shape", ["placement", "nnz_0", "nnz_T", "ncol_1"])
def test_placement_two_dimensions(T, shape, type):
    """margins 1 and 2 with int32 and float64 vectors through count and fill, then the composition, then once more: the
    same bits"""
    nrow, csc = sw.device_operands(T)[f"{shape}_{type}"]
    x, dim = _device(nrow, csc), (nrow, csc[0].size - 1)
    for margin in (1, 2):
        for op, st in (PLACEMENT if type == "double" else PLACEMENT_INT):
            what = f"{shape} {type} margin {margin} {op} {st}"
            stats = sw.stats_for(op, sw.stats_length(dim, margin), st, seed=margin)
            got, want, cls, over = _run_raw(x, nrow, csc, dim, margin, op, stats, st, what)
            runs = []
            for _ in range(2):
                R = x.sweep(op, torch.as_tensor(stats, device="cuda"), margin)
                ov = R.ovflow
                runs.append(_host(R))
                assert bool(ov.item()) == over and R.nrow == nrow and R.ncol == dim[1] and R.Rtype != LGLSXP
            _same(runs[0], want, cls, f"{what}, composition")
            for a, b, c in zip(runs[0], runs[1], got):
                assert np.array_equal(sc.bits(a) if a.dtype == np.float64 else a, sc.bits(b) if b.dtype == np.float64 else b)
                assert np.array_equal(sc.bits(a) if a.dtype == np.float64 else a, sc.bits(c) if c.dtype == np.float64 else c)


@pytest.mark.parametrize("op", ["==", "!=", ">", ">=", "<", "<="])
def test_placement_compare(T, op):
    """the Compare rule on the same operand: logical results, values 1 or NA, both margins, both operand types"""
    for type in ("double", "integer"):
        nrow, csc = sw.device_operands(T)[f"placement_{type}"]
        x, dim = _device(nrow, csc), (nrow, csc[0].size - 1)
        for margin, st in ((1, "double"), (2, "integer")):
            stats = sw.stats_for(op, sw.stats_length(dim, margin), st, seed=margin)
            got, want, cls, _ = _run_raw(x, nrow, csc, dim, margin, op, stats, st, f"{type} margin {margin} {op}")
            assert set(np.unique(got[2]).tolist()) <= {1, int(NA_integer)} and (got[2] == NA_integer).any()
            R = x.sweep(op, stats, margin)
            assert R.Rtype == LGLSXP
            _same(_host(R), want, cls, f"{type} margin {margin} {op}, composition")


# ---------------------------------------------------------------------------
# 2. dropped results
# ---------------------------------------------------------------------------
def test_a_zero_element_empties_its_row_or_leaf_but_for_nan_and_inf(T):
    nrow, csc = sw.device_operands(T)["placement_double"]
    cp, ri, val = csc
    x, dim = _device(nrow, csc), (nrow, cp.size - 1)
    long_leaf = int(np.argmax(np.diff(cp)))
    col = np.repeat(np.arange(dim[1]), np.diff(cp))
    special = np.isnan(val) | np.isinf(val)
    assert special[col == long_leaf].any()
    busy_row = int(np.bincount(ri[special], minlength=nrow).argmax())
    for margin, k, mine in ((2, long_leaf, col == long_leaf), (1, busy_row, ri == busy_row)):
        stats = sw.stats_for("*", sw.stats_length(dim, margin), "double")
        stats[k] = 0.0
        got, want, cls, _ = _run_raw(x, nrow, csc, dim, margin, "*", stats, "double", f"zero at {k} of margin {margin}")
        gcol = np.repeat(np.arange(dim[1]), np.diff(got[0]))
        left = (gcol == k) if margin == 2 else (got[1] == k)
        assert left.sum() == (mine & special).sum() > 0 and np.all(np.isnan(got[2][left]))
        assert np.array_equal(got[1][left], ri[mine & special])


def test_underflow_to_zero_drops_entries(T):
    nrow, (cp, ri, val) = sw.device_operands(T)["nnz_T_double"]
    val = np.where(np.arange(val.size) % 3 == 0, 1e-10, 1e10)         # 1e-10 * 1e-320 * 2500 is below half a denormal
    x, dim = _device(nrow, (cp, ri, val)), (nrow, cp.size - 1)
    stats = 1e-320 * (1.0 + np.arange(nrow))
    got, want, _, _ = _run_raw(x, nrow, (cp, ri, val), dim, 1, "*", stats, "double", "1e-320")
    assert got[1].size == int((np.arange(val.size) % 3 != 0).sum()) < val.size


def test_integer_overflow_gives_na_and_raises_the_word(T):
    nrow, csc = sw.device_operands(T)["placement_integer"]
    x, dim = _device(nrow, csc), (nrow, csc[0].size - 1)
    stats = (3_000_000 + np.arange(dim[1])).astype(np.int32)
    got, want, _, over = _run_raw(x, nrow, csc, dim, 2, "*", stats, "integer", "overflow")
    assert over and (got[2] == NA_integer).sum() > (csc[2] == NA_integer).sum() and (got[2] != NA_integer).any()
    R = x.sweep("*", stats, 2)
    torch.cuda.synchronize()
    assert bool(R.ovflow.item())


# ---------------------------------------------------------------------------
# 3. N-d
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["*", ">"])
@pytest.mark.parametrize("margin", sw.MARGINS_4D)
def test_four_dimensions(T, margin, op):
    for type, st in (("double", "double"), ("integer", "integer"), ("integer", "double")):
        nrow, csc = sw.dense_4d(type)
        x = _device(nrow, csc)
        stats = sw.stats_for(op, sw.stats_length(sw.DIM_4D, margin), st)
        want, cls, t, over = sw.expect_csc(op, nrow, csc, sw.DIM_4D, margin, stats, st)
        extents = [sw.DIM_4D[k - 1] for k in sw.as_margin(margin)]
        given = torch.as_tensor(stats.reshape(extents, order="F"), device="cuda")        # the array R would hand over
        _same(_host(x.sweep(op, given, margin, dim=sw.DIM_4D)), want, cls, f"{type} {st} margin {margin} {op}")
        _run_raw(x, nrow, csc, sw.DIM_4D, margin, op, stats, st, f"{type} {st} margin {margin} {op}, raw")


# ---------------------------------------------------------------------------
# 4. agreement with the scalar map
# ---------------------------------------------------------------------------
def _bits(a):
    return sc.bits(a) if a.dtype == np.float64 else a


def test_a_constant_vector_gives_the_scalar_maps_bits(T):
    constants = {"*": 2.5, "/": 3.0, "^": 2.5, "%%": 7.0, "%/%": 7.0, "==": 3.0, "!=": 0.0, "<=": -1.0, ">=": 1.0, "<": 0.0, ">": 0.0}
    for type in ("double", "integer"):
        nrow, csc = sw.device_operands(T)[f"placement_{type}"]
        x, ncol = _device(nrow, csc), csc[0].size - 1
        for op, s in constants.items():
            for margin, n in ((1, nrow), (2, ncol)):
                for st in ("double", "integer"):
                    scalar = s if st == "double" else int(s)
                    stats = np.full(n, scalar, dtype=np.float64 if st == "double" else np.int32)
                    A = _host(x.sweep(op, stats, margin))
                    B = _host(x.compare(op, scalar) if op in cc.COMPARE_OPS else x.arith(op, scalar))
                    for a, b in zip(A, B):
                        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (type, op, margin, st)


def test_pow_with_an_exponent_per_leaf_is_the_scalar_map_leaf_by_leaf(T):
    """both call svt_rule_pow on the same inputs, so no ulps bound is needed: leaf j of the sweep is x ^ s_j bit for bit"""
    base = np.array(ac.ULPS_INPUTS["^"], dtype=np.float64)
    n, exps = base.size, [float(e) for e, _ in ac.POW_EXPONENTS]
    cp = np.arange(len(exps) + 1, dtype=np.int64) * n
    ri = np.tile(np.arange(n, dtype=np.int32), len(exps))
    x = _device(n, (cp, ri, np.tile(base, len(exps))))
    one = _device(n, (cp[:2], ri[:n], base))
    got = _host(x.sweep("^", np.array(exps), 2))
    for j, e in enumerate(exps):
        w = _host(one.arith("^", e))
        lo, hi = got[0][j], got[0][j + 1]
        assert np.array_equal(got[1][lo:hi], w[1]) and np.array_equal(sc.bits(got[2][lo:hi]), sc.bits(w[2])), e


# ---------------------------------------------------------------------------
# 5. validity
# ---------------------------------------------------------------------------
BAD_ELEMENTS = [("*", "double", np.nan), ("*", "double", NA_real), ("*", "double", np.inf), ("*", "double", -np.inf),
                ("*", "integer", NA_integer), ("/", "double", 0.0), ("/", "double", np.nan), ("/", "integer", 0),
                ("%%", "double", -0.0), ("%%", "integer", NA_integer), ("%/%", "double", 0.0), ("%/%", "integer", 0),
                ("^", "double", 0.0), ("^", "double", -2.0), ("^", "double", np.nan), ("^", "integer", -1),
                (">", "double", -1.0), (">", "double", np.nan), (">=", "integer", 0), ("==", "double", 0.0),
                ("!=", "integer", 4), ("<", "double", 0.5), ("<=", "integer", 0), ("<=", "logical", NA_integer)]


@pytest.mark.parametrize("k", range(len(BAD_ELEMENTS)))
def test_an_element_that_would_fill_the_result_is_refused_on_the_device(T, k):
    op, st, value = BAD_ELEMENTS[k]
    nrow, csc = sw.device_operands(T)["nnz_T_integer" if st == "logical" else "nnz_T_double"]
    x = _device(nrow, csc, logical=st == "logical")
    dim = (nrow, csc[0].size - 1)
    for margin, (first, second) in ((1, (1700, 803)), (2, (3, 1))):
        stats = sw.stats_for(op, sw.stats_length(dim, margin), "integer" if st == "logical" else st)
        stats[[first, second]] = value
        r = Raw(x, op, stats, st, sweep_form(dim, margin))
        assert r.count() < 0 and r.bad.value == min(first, second), (r.bad.value, r.lib.svt_last_error())
        assert f"element {min(first, second)} ".encode() in r.lib.svt_last_error()
        assert r.cp.untouched() and r.nnz.value == -5 and r.ws_guard_intact()
        with pytest.raises(SparseArrayError, match=rf"stats\[{min(first, second)}\] = .*does not keep the result sparse"):
            x.sweep(op, torch.as_tensor(stats, device="cuda"), margin, logical=st == "logical")
    torch.cuda.synchronize()


def test_the_smallest_offender_of_a_long_vector(T):
    """a vector longer than one pass of the checking grid, on an operand of many empty leaves"""
    ncol = 300_001
    x = _device(5, (np.zeros(ncol + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    stats = np.arange(1.0, ncol + 1.0)
    r = Raw(x, "/", stats, "double", sweep_form((5, ncol), 2))
    assert r.count() == 0 and r.nnz.value == 0 and not r.cp.body().any()
    stats[[299_999, 280_017, 290_000]] = 0.0
    r = Raw(x, "/", stats, "double", sweep_form((5, ncol), 2))
    assert r.count() < 0 and r.bad.value == 280_017 and r.cp.untouched()


def test_statuses_leave_the_outputs_untouched(T):
    """< 0: a vector of another length, integers that do not divide the leaves, a workspace one byte short, + and -, an
    unknown opcode, a logical operand under Arith, a logical vector under Arith; > 0: na_background"""
    nrow, csc = sw.device_operands(T)["nnz_T_double"]
    x, ncol = _device(nrow, csc), csc[0].size - 1
    lgl = _device(nrow, (csc[0], csc[1], np.ones(csc[1].size, np.int32)), logical=True)
    s_row, s_col = np.ones(nrow), np.ones(ncol)
    negative = [(Raw(x, "*", s_row, "double", (0, 1, ncol)), "length"), (Raw(x, "*", s_col, "double", (1, 1, 1)), "length"),
                (Raw(x, "*", s_col, "double", (0, 1, ncol), stats_len=ncol - 1), "length"),
                (Raw(x, "*", np.ones(3), "double", (0, 1, 3)), "do not divide"), (Raw(x, "*", s_col, "double", (0, 0, ncol)), "geometry"),
                (Raw(x, "*", np.ones(2 * ncol), "double", (0, 1, 2 * ncol)), "do not divide"),
                (Raw(x, "*", s_col, "double", (2, 1, ncol)), "geometry"),
                (Raw(x, "*", s_col, "double", (0, 1, ncol), short=1), "workspace too small"),
                (Raw(x, "+", s_col, "double", (0, 1, ncol)), "result wouldn't be sparse in general"),
                (Raw(x, "-", s_col, "double", (0, 1, ncol)), "result wouldn't be sparse in general"),
                (Raw(x, 0, s_col, "double", (0, 1, ncol)), "unknown operation"), (Raw(x, 8, s_col, "double", (0, 1, ncol)), "unknown operation"),
                (Raw(lgl, "*", s_col, "double", (0, 1, ncol)), "logical"),
                (Raw(x, "*", s_col.astype(np.int32), "logical", (0, 1, ncol)), "unknown operation")]
    for r, msg in negative:
        assert r.count() < 0 and msg.encode() in r.lib.svt_last_error(), (msg, r.lib.svt_last_error())
        assert r.cp.untouched() and r.nnz.value == -5 and bool((r.ws == 0xA5).all())
    na = _device(nrow, csc)
    off = 4 + 4 + 3 * 8 + 3 * 8              # struct svt_dev_csc: Rtype, owned, three extents, three pointers, na_background
    ctypes.cast(na._h, ctypes.POINTER(ctypes.c_int32))[off // 4] = 1
    for op in ("*", ">"):
        r = Raw(na, op, s_col, "double", (0, 1, ncol))
        assert r.count() > 0 and b"NaArray" in r.lib.svt_last_error()
        assert r.cp.untouched() and r.nnz.value == -5 and bool((r.ws == 0xA5).all())
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        na.sweep("*", s_col, 2)
    for margin, msg in (((1, 3), "margin"), (3, "margin")):
        with pytest.raises(SparseArrayError, match=msg):
            x.sweep("*", s_col, margin)
    with pytest.raises(SparseArrayError, match="result wouldn't be sparse in general"):
        x.sweep("+", s_col, 2)
    with pytest.raises(SparseArrayError, match="length"):
        x.sweep("*", s_row, 2)
    # the stream is sound after all of it
    assert _host(x.sweep("*", s_col, 2))[1].size == int((csc[2] != 0).sum())


# ---------------------------------------------------------------------------
# 6. host entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sw.SESSION_NAMES)
def test_session_shared_case(hip, name):
    _, xn, margin, op, st = sw.SESSION_BY_NAME[name]
    x, stats = sw.session_stats(name)
    want = sw.expect_session(op, x, stats, st, margin)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = hip.sweep(x, margin, stats, op)
    if op in cc.COMPARE_OPS:
        cc.check_result(res, x, want, name)
        assert not w
    else:
        ac.check_result(res, x, want, name)
        assert [str(m.message) for m in w] == (["NAs produced by integer overflow"] if want.overflow else []), name
    assert res.dimnames == x.dimnames


def test_session_refusals_and_dimnames(hip):
    d = cc.operand("d1")
    with pytest.raises(SparseArrayError, match=r"length\(STATS\) is 41 but prod\(dim\(x\)\[MARGIN\]\) is 29"):
        hip.sweep(d, 2, np.ones(41), "/")
    with pytest.raises(SparseArrayError, match=r"c\(1, 3\) is not supported"):
        hip.sweep(cc.operand("d3d"), (1, 3), np.ones(36), "*")
    with pytest.raises(SparseArrayError, match=r"STATS\[4\] == 0"):
        hip.sweep(d, 2, np.where(np.arange(29) == 3, 0.0, 2.0), "/")
    named = type(d)(d.dim, d.type, d.leaves, dimnames=[[f"g{i}" for i in range(41)], None])
    res = hip.sweep(named, 1, np.arange(1.0, 42.0), "*")
    assert res.dimnames == named.dimnames


def test_the_library_names_the_element_the_session_did_not_see(hip):
    """the host entry point itself, past the Session's checks: the device finds the element and hands back its index"""
    from sparsearray_amd._dispatch import CAbiDispatcher
    d = cc.operand("d1")
    stats = np.arange(1.0, 30.0)
    stats[[20, 11]] = 0.0
    with pytest.raises(SparseArrayError, match="element 11 of the vector does not keep the result sparse"):
        hip._call("C_sweep_SVT", d, stats, "double", (2,), "/")
    with pytest.raises(SparseArrayError, match="strictly increasing run of consecutive dimensions"):
        hip._call("C_sweep_SVT", cc.operand("d3d"), np.ones(36), "double", (1, 3), "*")
    assert isinstance(hip._call, CAbiDispatcher)


# ---------------------------------------------------------------------------
# 7. the chain, all resident
# ---------------------------------------------------------------------------
def _counts(empty_col=None):
    rng = np.random.default_rng(77)
    dense = np.where(rng.random((300, 50)) < 0.15, rng.integers(1, 40, size=(300, 50)), 0).astype(np.float64)
    dense[0, :] = 1.0                                                  # no column is empty
    if empty_col is not None:
        dense[:, empty_col] = 0.0
    cp = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=0))]).astype(np.int64)
    ri = np.nonzero(dense.T)[1].astype(np.int32)
    return dense, (cp, ri, dense.T[dense.T != 0])


def test_normalisation_chain_stays_on_the_device(T):
    from sparsearray_amd.device import colstats
    dense, csc = _counts()
    s = dense.sum(axis=0)
    assert np.all(s > 0) and np.all(s < 2 ** 53) and np.all(dense == np.round(dense))      # the sums are exact in double
    x = _device(300, csc)
    sums, _ = colstats(x, "sum")
    assert sums.is_cuda and sums.dtype == torch.float64
    R = x.sweep("/", sums, 2).arith("*", 1e4)
    got = _host(R)
    want = dense / s[None, :] * 1e4
    assert np.array_equal(got[0], csc[0]) and np.array_equal(got[1], csc[1])
    assert np.array_equal(sc.bits(got[2]), sc.bits(want.T[dense.T != 0]))
    # the same chain on an operand with one empty column: its sum is 0 and the division is refused, naming the column
    dense, csc = _counts(empty_col=17)
    x = _device(300, csc)
    with pytest.raises(SparseArrayError, match=r"stats\[17\] = 0\.0"):
        x.sweep("/", colstats(x, "sum")[0], 2)
