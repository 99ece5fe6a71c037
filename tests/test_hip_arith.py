"""Arith, unary minus and Math on the GPU (kernels_arith.hip; include/svt_hip.h, svt_dev_arith_* and svt_Arith_* /
svt_unary_minus_* / svt_Math_*): the shared cases of tests/arith_cases.py through the host entry points, and the two
kernel families at the device level on operands placed around the tile T = svt_dev_arith_tile().  The expectation and
the way values are compared (bits; the NaN classes; ulps for log1p, expm1 and ^) are stated in tests/arith_cases.py.
No operand holds more than about 3 T nonzeros."""
import ctypes
import warnings

import numpy as np
import pytest

import arith_cases as ac
import subset_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64          # guard words on either side of every output array
# The largest distance from the correctly rounded value seen on gfx950 for the inputs of arith_cases.ULPS_INPUTS
# (profiles/elementwise_accuracy.txt), rounded up to a whole ulp: the inputs are fixed and the kernels deterministic.
MAX_ULPS = {"log1p": 0, "expm1": 1, "^": 1}


def _arith(hip, op, x, y, expect_overflow):
    """hip.arith with the overflow warning asserted: raised exactly when the expectation overflows"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = hip.arith(op, x, y)
    msgs = [str(m.message) for m in w]
    assert msgs == (["NAs produced by integer overflow"] if expect_overflow else []), msgs
    return res


# ---------------------------------------------------------------------------
# shared cases, host entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,op", ac.MERGE_PARAMS)
def test_merge_shared_case(hip, name, op):
    _, xn, yn, _ = ac.MERGE_BY_NAME[name]
    x, y = ac.operand(xn), ac.operand(yn)
    want = ac.expect_merge(op, x, y)
    ac.check_result(_arith(hip, op, x, y, want.overflow), x, want, f"{name} {op}")
    if name == "identical_operands" and op == "-":
        assert not want.stored.any()
    if name == "only_nan_and_inf_survive_an_implicit_zero":
        assert want.stored.any() and not np.isfinite(want.dense[want.stored]).any()
    if name == "int_overflow":
        assert want.overflow and (want.dense[want.stored] == ac.INT_MIN).any()


@pytest.mark.parametrize("name", ac.SCALAR_NAMES)
def test_scalar_shared_case(hip, name):
    _, xn, op, s, st = ac.SCALAR_BY_NAME[name]
    x = ac.operand(xn)
    want = ac.expect_scalar(op, x, s, st)
    s = int(s) if st == "integer" else float(s)
    ac.check_result(_arith(hip, op, x, s, want.overflow), x, want, name, MAX_ULPS["^"])
    if op == "*":                                          # a scalar on the left of *: the same call
        ac.check_result(_arith(hip, op, s, x, want.overflow), x, want, name + ", scalar on the left")
    if name.startswith("times_0") and "no_specials" not in name:
        kept = want.dense[want.stored]
        assert kept.size and (np.all(~np.isfinite(kept)) if want.type == "double" else np.all(kept == ac.INT_MIN))
    if name == "times_0_no_specials":
        assert not want.stored.any()
    if name == "times_1e-320_underflow":
        assert 0 < want.stored.sum() < ac.dense_nd(x)[1].sum()


@pytest.mark.parametrize("xn", ac.NEG_OPERANDS)
def test_unary_minus_shared_case(hip, xn):
    x = ac.operand(xn)
    ac.check_result(hip.unary_minus(x), x, ac.expect_neg(x), f"-{xn}")


@pytest.mark.parametrize("op", [o for o in ac.MATH_OPS if o not in ac.ULPS_MATH])
@pytest.mark.parametrize("xn", ac.MATH_OPERANDS)
def test_math_shared_case(hip, xn, op):
    x = ac.operand(xn)
    ac.check_result(hip.math(op, x), x, ac.expect_math(op, x), f"{op}({xn})")


@pytest.mark.parametrize("fn", ["log1p", "expm1", "^"])
def test_device_math_library_within_the_measured_ulps(hip, fn):
    """log1p, expm1 and ^ on the fixed inputs against the correctly rounded values: the bound is the largest distance
    measured on the GPU (profiles/elementwise_accuracy.txt), a whole number of ulps"""
    x = ac.ulps_operand(fn)
    worst = 0
    if fn == "^":
        for s, st in ac.POW_EXPONENTS:
            s = int(s) if st == "integer" else float(s)
            d = ac.check_result(hip.arith("^", x, s), x, ac.expect_scalar("^", x, s, "double"), f"^ {s}", max_ulps=2 ** 62)
            print(f"x ^ {s}: {d} ulps")
            worst = max(worst, d)
    else:
        for xn in (None,) + ac.MATH_OPERANDS:
            y = x if xn is None else ac.operand(xn)
            worst = max(worst, ac.check_result(hip.math(fn, y), y, ac.expect_math(fn, y), f"{fn}({xn})", max_ulps=2 ** 62))
    print(f"{fn}: largest distance {worst} ulps")
    assert worst <= MAX_ULPS[fn], f"{fn}: {worst} ulps, the measured bound is {MAX_ULPS[fn]}"


def test_unsupported_and_refused_operations(hip):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    d, i = ac.operand("d1"), ac.operand("i1")
    call = hip._call
    for op in ("sin", "asin", "sinh", "asinh", "sinpi", "tan", "atan", "tanh", "atanh", "tanpi", "round", "signif"):
        with pytest.raises(SparseArrayUnsupported, match="not supported here"):
            hip.math(op, d)
    na = sc.operand("na_double")[0]
    plain = sc.build(na.dim, "double", np.ones(na.dim, bool))
    for f in (lambda: hip.arith("+", na, plain), lambda: hip.arith("+", plain, na), lambda: hip.arith("*", na, 2.0),
              lambda: hip.unary_minus(na), lambda: hip.math("sqrt", na)):
        with pytest.raises(SparseArrayUnsupported, match="NaArray"):
            f()
    # the entry points themselves (not the Session's checks): < 0
    lgl = sc.operand("logical")[0]
    for f, msg in ((lambda: call.C_Arith_SVT1_SVT2(d, ac.operand("d_ncol0"), "+"), "non-conformable"),
                   (lambda: call.C_Arith_SVT1_SVT2(d, d, "/"), "unknown operation"),
                   (lambda: call.C_Arith_SVT1_v2(d, 2.0, "double", "+"), "unknown operation"),
                   (lambda: call.C_Arith_SVT1_v2(lgl, 2.0, "double", "*"), "logical"),
                   (lambda: call.C_unary_minus_SVT(lgl), "logical"),
                   (lambda: call.C_Math_SVT(i, "sqrt", 0.0), "double"),
                   (lambda: call.C_Math_SVT(d, "log", 0.0), "unknown operation")):
        with pytest.raises(SparseArrayError, match=msg) as e:
            f()
        assert not isinstance(e.value, SparseArrayUnsupported)


def test_resident_cache_counts_one_miss_per_operand(hip):
    x, y = ac.operand("d1"), ac.operand("i2")
    hip.resident_clear()
    hip.resident_set_limit(1 << 22)
    try:
        before = hip.resident_stats()
        hip.arith("+", x, y)
        assert hip.resident_stats()["misses"] == before["misses"] + 2
        ac.check_result(hip.arith("-", x, y), x, ac.expect_merge("-", x, y), "resident x - y")
        ac.check_result(hip.arith("-", x, x), x, ac.expect_merge("-", x, x), "resident x - x")
        ac.check_result(hip.math("sqrt", x), x, ac.expect_math("sqrt", x), "resident sqrt")
        ac.check_result(hip.arith("*", y, 3), y, ac.expect_scalar("*", y, 3, "integer"), "resident y * 3")
        after = hip.resident_stats()
        assert after["misses"] == before["misses"] + 2 and after["hits"] == before["hits"] + 6
    finally:
        hip.resident_set_limit(0)
        hip.resident_clear()


# ---------------------------------------------------------------------------
# device level, around the tile
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile(hip):
    from sparsearray_amd.device import arith_tile
    return arith_tile()


def _device(nrow, csc):
    from sparsearray_amd.device import DeviceCSC
    cp, ri, val = csc
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val), device="cuda"))


def _same(got, want, cls, what):
    """CSC triples: col_ptr and row_idx exactly, rows ascending in every column, values by their class"""
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
    """One operation of either family through the count and fill calls with the test's own buffers: a workspace of the
    advertised size followed by a guard band, every output between guard words.  y None: the map (kind, op, s, s_Rtype)."""

    def __init__(self, x, y, op, kind=0, s=0.0, s_Rtype=0, short=0):
        from sparsearray_amd.device import _lib, _stream
        self.lib, self.stream, self.x, self.y, self.op, self.map_args = _lib(), _stream, x, y, op, (kind, op, float(s), s_Rtype)
        self.nb = (self.lib.svt_dev_arith_map_ws_bytes(x.ncol, x.nnz) if y is None else
                   self.lib.svt_dev_arith_merge_ws_bytes(x.ncol, x.nnz, y.nnz))
        self.ws = torch.full((self.nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cp = Guarded(x.ncol + 1, torch.int64, -77)
        self.nnz = ctypes.c_int64(-5)
        self.short = short
        self.ov = torch.zeros(1, dtype=torch.int32, device="cuda")

    def count(self):
        if self.y is None:
            rc = self.lib.svt_dev_arith_map_count(self.x.handle, *self.map_args, self.cp.ptr(), ctypes.byref(self.nnz),
                                                  self.ws.data_ptr(), self.nb - self.short, self.stream())
        else:
            rc = self.lib.svt_dev_arith_merge_count(self.x.handle, self.y.handle, self.op, self.cp.ptr(), ctypes.byref(self.nnz),
                                                    self.ws.data_ptr(), self.nb - self.short, self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, dtype, short=0):
        n = max(self.nnz.value, 0)
        self.ri, self.vv = Guarded(n, torch.int32, -77), Guarded(n, dtype, 77)
        if self.y is None:
            rc = self.lib.svt_dev_arith_map_fill(self.x.handle, *self.map_args, self.cp.ptr(), self.ri.ptr(), self.vv.ptr(),
                                                 self.ov.data_ptr(), self.ws.data_ptr(), self.nb - short, self.stream())
        else:
            rc = self.lib.svt_dev_arith_merge_fill(self.x.handle, self.y.handle, self.op, self.cp.ptr(), self.ri.ptr(),
                                                   self.vv.ptr(), self.ov.data_ptr(), self.ws.data_ptr(), self.nb - short,
                                                   self.stream())
        torch.cuda.synchronize()
        return rc

    def ws_guard_intact(self):
        return bool((self.ws[self.nb:] == 0xA5).all())

    def arrays(self):
        return self.cp.body(), self.ri.body(), self.vv.body()


@pytest.mark.parametrize("name", ac.DEVICE_NAMES)
def test_merge_around_the_tile(tile, name):
    """count's out_col_ptr and nnz, then the filled arrays, rows ascending, every guard word intact; the composition
    DeviceCSC.arith gives the same arrays"""
    from sparsearray_amd.api import ARITH_OPCODES
    c = ac.device_cases(tile)[name]
    want = c.want
    x, y = _device(c.nrow, c.x), _device(c.nrow, c.y)
    r = Raw(x, y, ARITH_OPCODES[c.op])
    assert r.count() == 0
    assert r.nnz.value == want[1].size and np.array_equal(r.cp.body(), want[0]), f"{name}: count"
    assert r.cp.intact() and r.ws_guard_intact()
    assert r.fill(torch.float64 if want[2].dtype == np.float64 else torch.int32) == 0
    assert r.cp.intact() and r.ri.intact() and r.vv.intact() and r.ws_guard_intact()
    _same(r.arrays(), want, c.cls, name)
    assert bool(r.ov.item()) == c.overflow
    R = x.arith(c.op, y)
    ov = R.ovflow
    torch.cuda.synchronize()
    got = (R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy())
    _same(got, want, c.cls, f"{name}, composition")
    assert np.array_equal(sc.bits(got[2]), sc.bits(r.arrays()[2])) and bool(ov.item()) == c.overflow
    assert R.nrow == c.nrow and R.ncol == c.ncol


@pytest.mark.parametrize("name", ["one_column_holds_everything", "100000_empty_columns", "straddling_pairs_columns",
                                  "merged_length_+0_from_T", "merged_length_+1_from_T", "all_match_int", "empty_both"])
def test_map_around_the_tile(tile, name):
    """the map family on the x operands of the merge cases: x * 0.5, -x, abs(x), and a predicate that drops entries
    (x %/% 50: the small magnitudes become zero) -- counts, arrays, guards"""
    from sparsearray_amd.api import ARITH_OPCODES, MATH_OPCODES
    from sparsearray_amd.device import ARITH_MATH, ARITH_NEG, ARITH_SCALAR
    from sparsearray_amd.svt import INTSXP, REALSXP
    c = ac.device_cases(tile)[name]
    cp, ri, val = c.x
    x = _device(c.nrow, c.x)
    is_int = val.dtype == np.int32
    ops = [(ARITH_NEG, 0, 0.0, 0, ac.Expected("integer" if is_int else "double", -val, None, np.ones(val.shape, bool))),
           (ARITH_SCALAR, ARITH_OPCODES["%/%"], 50, INTSXP if is_int else REALSXP,
            ac.Expected("integer" if is_int else "double", np.floor_divide(val, 50) if is_int else np.floor(val / 50.0), None,
                        np.ones(val.shape, bool)))]
    if not is_int:
        ops += [(ARITH_SCALAR, ARITH_OPCODES["*"], 0.5, REALSXP, ac.Expected("double", val * 0.5, None, np.ones(val.shape, bool))),
                (ARITH_MATH, MATH_OPCODES["abs"], 0.0, 0, ac.Expected("double", np.abs(val), None, np.ones(val.shape, bool)))]
    for kind, op, s, st, e in ops:
        keep = e.stored
        col = np.repeat(np.arange(c.ncol), np.diff(cp))
        want_cp = np.zeros(c.ncol + 1, np.int64)
        np.cumsum(np.bincount(col[keep], minlength=c.ncol), out=want_cp[1:])
        r = Raw(x, None, op, kind, s, st)
        assert r.count() == 0
        assert r.nnz.value == int(keep.sum()) and np.array_equal(r.cp.body(), want_cp), f"{name}: count of kind {kind}"
        assert r.fill(torch.int32 if is_int else torch.float64) == 0
        assert r.cp.intact() and r.ri.intact() and r.vv.intact() and r.ws_guard_intact()
        got = r.arrays()
        assert np.array_equal(got[1], ri[keep]) and np.array_equal(sc.bits(got[2]), sc.bits(e.dense[keep])), f"{name}: kind {kind}"
    if name == "one_column_holds_everything":
        assert 0 < int(ops[1][4].stored.sum()) < val.size          # the predicate dropped some entries and kept others


def test_same_call_twice_gives_the_same_bits(tile):
    c = ac.device_cases(tile)["one_column_holds_everything"]
    x, y = _device(c.nrow, c.x), _device(c.nrow, c.y)
    runs = []
    for _ in range(2):
        R = x.arith("*", y).math("log1p").arith("/", 3.0)
        torch.cuda.synchronize()
        runs.append((R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy().view(np.uint64)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_map_route_leaves_the_subset_route_counts_alone(tile):
    from sparsearray_amd.device import subset_route_counts
    c = ac.device_cases(tile)["all_match"]
    x, y = _device(c.nrow, c.x), _device(c.nrow, c.y)
    subset_route_counts(reset=True)
    x.neg(); x.math("sqrt"); x.arith("*", 2.0); x.arith("+", y)
    torch.cuda.synchronize()
    assert subset_route_counts() == {"column_gather": 0, "row_filter": 0, "general_rows": 0}


def test_statuses_leave_the_outputs_untouched(tile):
    """< 0: extents that differ, a workspace one byte short (count and fill), a logical operand, an unknown opcode or
    kind, Math on integers; > 0: na_background, the Math functions not offered.  Nothing is written outside ws."""
    from sparsearray_amd.api import ARITH_OPCODES, MATH_OPCODES
    from sparsearray_amd.device import ARITH_MATH, ARITH_MERGE, ARITH_NEG, ARITH_SCALAR, DeviceCSC, _lib
    from sparsearray_amd.svt import REALSXP
    lib = _lib()
    c = ac.device_cases(tile)["all_match"]
    x, y = _device(c.nrow, c.x), _device(c.nrow, c.y)
    cp, ri, val = c.x
    other_nrow = _device(c.nrow + 1, c.y)
    other_ncol = _device(c.nrow, (np.append(c.y[0], c.y[0][-1]), c.y[1], c.y[2]))
    lgl = DeviceCSC(c.nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                    torch.ones(ri.size, dtype=torch.int32, device="cuda"), logical=True)
    xi = _device(c.nrow, (cp, ri, np.ones(ri.size, np.int32)))
    add, mult = ARITH_OPCODES["+"], ARITH_OPCODES["*"]
    negative = [(Raw(x, other_nrow, add), "non-conformable"), (Raw(x, other_ncol, add), "non-conformable"),
                (Raw(x, y, add, short=1), "workspace too small"), (Raw(x, None, mult, ARITH_SCALAR, 2.0, REALSXP, short=1),
                                                                   "workspace too small"),
                (Raw(x, lgl, add), "logical"), (Raw(lgl, y, add), "logical"), (Raw(lgl, None, 0, ARITH_NEG), "logical"),
                (Raw(x, y, ARITH_OPCODES["/"]), "unknown operation"), (Raw(x, y, 0), "unknown operation"),
                (Raw(x, y, 99), "unknown operation"), (Raw(x, None, add, ARITH_SCALAR, 2.0, REALSXP), "unknown operation"),
                (Raw(x, None, mult, ARITH_MERGE, 2.0, REALSXP), "unknown operation"), (Raw(x, None, 1, 9), "unknown operation"),
                (Raw(x, None, 0, ARITH_MATH), "unknown operation"), (Raw(x, None, 21, ARITH_MATH), "unknown operation"),
                (Raw(xi, None, MATH_OPCODES["sqrt"], ARITH_MATH), "double")]
    for r, msg in negative:
        assert r.count() < 0 and msg.encode() in lib.svt_last_error(), (msg, lib.svt_last_error())
        assert r.cp.untouched() and r.nnz.value == -5 and bool((r.ws == 0xA5).all())
    r = Raw(x, y, add)
    assert r.count() == 0
    assert r.fill(torch.float64, short=1) < 0 and b"workspace too small" in lib.svt_last_error()
    assert r.ri.untouched() and r.vv.untouched()
    # > 0: "not supported here"
    na = _device(c.nrow, c.x)
    off = 4 + 4 + 3 * 8 + 3 * 8              # struct svt_dev_csc: Rtype, owned, three extents, three pointers, na_background
    ctypes.cast(na._h, ctypes.POINTER(ctypes.c_int32))[off // 4] = 1
    positive = [(Raw(na, y, add), "NaArray"), (Raw(x, na, add), "NaArray"), (Raw(na, None, 0, ARITH_NEG), "NaArray"),
                (Raw(x, None, MATH_OPCODES["sin"], ARITH_MATH), "not supported here"),
                (Raw(x, None, MATH_OPCODES["round"], ARITH_MATH), "not supported here")]
    for r, msg in positive:
        assert r.count() > 0 and msg.encode() in lib.svt_last_error(), (msg, lib.svt_last_error())
        assert r.cp.untouched() and r.nnz.value == -5 and bool((r.ws == 0xA5).all())
    # the stream is sound after all of it
    r = Raw(x, y, add)
    assert r.count() == 0 and r.fill(torch.float64) == 0
    _same(r.arrays(), c.want, c.cls, "after the statuses")
