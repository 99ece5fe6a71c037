"""Compare and Logic on the GPU (the Compare and Logic rules of kernels_arith.hip; include/svt_hip.h, svt_dev_compare_* /
svt_dev_logic_* and svt_Compare_* / svt_Logic_*): the shared cases of tests/compare_cases.py through the host entry
points, and the kernels at the device level on the placements of arith_cases.device_cases(T) around the tile
T = svt_dev_arith_tile().  The expectation is numpy's on the dense arrays (tests/compare_cases.py); every comparison is
bit for bit.  No operand holds more than 3 T + 100 entries."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import compare_cases as cc
import subset_cases as sc
from helpers import Arena

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NA = int(cc.NA)


# ---------------------------------------------------------------------------
# shared cases, host entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ac.MERGE_CASES])
def test_compare_merge_shared_case(hip, name):
    """x != y, x < y, x > y over an operand pair of arith_cases.MERGE_CASES"""
    _, xn, yn, _ = ac.MERGE_BY_NAME[name]
    x, y = cc.operand(xn), cc.operand(yn)
    for op in cc.MERGE_OPS:
        want = cc.expect_compare_merge(op, x, y)
        cc.check_result(hip.compare(op, x, y), x, want, f"{name} {op}")
        if name == "identical_operands" and op == "!=":
            assert not want.stored[~np.isnan(ac.as_double(ac.dense_nd(x)[0]))].any()
        if name.startswith("specials") and op == "!=":
            assert (want.dense[want.stored] == NA).any() and (want.dense[want.stored] == 1).any()


@pytest.mark.parametrize("name", cc.SCALAR_NAMES)
def test_compare_scalar_shared_case(hip, name):
    _, xn, op, s, st = cc.SCALAR_BY_NAME[name]
    x = cc.operand(xn)
    want = cc.expect_compare_scalar(op, x, s, st)
    s = bool(s) if st == "logical" else int(s) if st == "integer" else float(s)
    cc.check_result(hip.compare(op, x, s), x, want, name)
    flipped = {"<=": ">=", ">=": "<=", "<": ">", ">": "<"}.get(op, op)
    cc.check_result(hip.compare(flipped, s, x), x, want, name + ", scalar on the left")
    if name == "stored_zeros_gt_0":
        dense, stored = ac.dense_nd(x)
        assert (stored & (dense == 0) & np.signbit(dense)).any() and not want.stored[dense == 0].any()
        assert want.stored[dense == 5e-324].all()
    if name.endswith("gt_inf") or name.endswith("lt_minus_inf"):
        assert np.all(want.dense[want.stored] == NA)
    if name == "i1_gt_2.5":
        dense = ac.dense_nd(x)[0]
        assert np.array_equal(want.stored, dense >= 3)


@pytest.mark.parametrize("op", cc.LOGIC_OPS)
@pytest.mark.parametrize("name", [c[0] for c in cc.LOGIC_CASES])
def test_logic_shared_case(hip, name, op):
    _, xn, yn = {c[0]: c for c in cc.LOGIC_CASES}[name]
    x, y = cc.operand(xn), cc.operand(yn)
    want = cc.expect_logic(op, x, y)
    cc.check_result(hip.logic(op, x, y), x, want, f"{name} {op}")
    if name == "na_and_false_both_sides":
        dx, sx = ac.dense_nd(x)
        dy, sy = ac.dense_nd(y)
        for a in (1, 0, NA):                              # every combination of stored values meets somewhere
            for b in (1, 0, NA):
                assert (sx & sy & (dx == a) & (dy == b)).any(), (a, b)


def test_unsupported_and_refused_operations(hip):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    d, lg = cc.operand("d1"), cc.operand("l1")
    call = hip._call
    na = sc.operand("na_double")[0]
    plain = sc.build(na.dim, "double", np.ones(na.dim, bool))
    for f in (lambda: hip.compare("!=", na, plain), lambda: hip.compare("<", plain, na), lambda: hip.compare(">", na, 0)):
        with pytest.raises(SparseArrayUnsupported, match="NaArray"):
            f()
    # the entry points themselves (not the Session's checks): < 0
    for f, msg in ((lambda: call.C_Compare_SVT1_SVT2(d, ac.operand("d_ncol0"), "!="), "non-conformable"),
                   (lambda: call.C_Compare_SVT1_SVT2(d, d, "=="), "result wouldn't be sparse"),
                   (lambda: call.C_Compare_SVT1_SVT2(d, d, "<="), "result wouldn't be sparse"),
                   (lambda: call.C_Compare_SVT1_v2(d, 0.0, "double", "=="), "result wouldn't be sparse"),
                   (lambda: call.C_Compare_SVT1_v2(d, 1.0, "double", "<"), "result wouldn't be sparse"),
                   (lambda: call.C_Compare_SVT1_v2(d, float("nan"), "double", ">"), "result wouldn't be sparse"),
                   (lambda: call.C_Compare_SVT1_v2(d, float(NA), "integer", ">"), "result wouldn't be sparse"),
                   (lambda: call.C_Logic_SVT1_SVT2(lg, ac.operand("i1"), "&"), "logical"),
                   (lambda: call.C_Logic_SVT1_SVT2(lg, sc.operand("logical")[0], "|"), "non-conformable")):
        with pytest.raises(SparseArrayError, match=msg) as e:
            f()
        assert not isinstance(e.value, SparseArrayUnsupported)
    # the Arith entry points refuse a logical operand as before
    with pytest.raises(SparseArrayError, match="logical"):
        call.C_Arith_SVT1_v2(lg, 2.0, "double", "*")


def test_resident_cache_serves_the_operands(hip):
    x, y = cc.operand("d1"), cc.operand("i2")
    hip.resident_clear()
    hip.resident_set_limit(1 << 22)
    try:
        before = hip.resident_stats()
        cc.check_result(hip.compare("!=", x, y), x, cc.expect_compare_merge("!=", x, y), "resident x != y")
        cc.check_result(hip.compare(">", x, 0), x, cc.expect_compare_scalar(">", x, 0, "integer"), "resident x > 0")
        after = hip.resident_stats()
        assert after["misses"] == before["misses"] + 2 and after["hits"] == before["hits"] + 1
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


def _device(nrow, csc, logical=False):
    from sparsearray_amd.device import DeviceCSC
    cp, ri, val = csc
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val), device="cuda"), logical=logical)


def _operands(c, values):
    """the two device operands of a placement under a value kind, and their host arrays"""
    kx, vx, ky, vy = cc.device_operands(c, values)
    x, y = ac._csc(kx, vx, c.nrow, c.ncol), ac._csc(ky, vy, c.nrow, c.ncol)
    return _device(c.nrow, x, values == "logical"), _device(c.nrow, y, values == "logical"), (kx, vx, ky, vy), x


class Raw:
    """One operation through the count and fill calls with the test's own buffers, every one a part of a 0xA5 arena with
    guard bands (tests/helpers.py): the workspace of exactly the advertised size and out_col_ptr for the count, then
    out_row_idx and out_val of exactly the counted size for the fill.  family: "compare_merge", "logic_merge" or
    "compare_map" (y None; s, s_Rtype)."""

    def __init__(self, family, x, y, op, s=0.0, s_Rtype=0, short=0, ws_fill=0xA5):
        from sparsearray_amd.device import _lib, _stream
        self.lib, self.stream, self.family, self.x, self.y, self.op = _lib(), _stream, family, x, y, op
        self.head = (x.handle, op, float(s), s_Rtype) if y is None else (x.handle, y.handle, op)
        self.nb = (self.lib.svt_dev_arith_map_ws_bytes(x.ncol, x.nnz) if y is None else
                   self.lib.svt_dev_arith_merge_ws_bytes(x.ncol, x.nnz, y.nnz))
        self.a = Arena([self.nb, (x.ncol + 1) * 8])
        self.a.part(0).fill_(ws_fill)
        self.nnz, self.short, self.b = ctypes.c_int64(-5), short, None

    def count(self):
        rc = getattr(self.lib, f"svt_dev_{self.family}_count")(*self.head, self.a.part(1).data_ptr(), ctypes.byref(self.nnz),
                                                              self.a.part(0).data_ptr(), self.nb - self.short, self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, short=0):
        n = max(self.nnz.value, 0)
        self.b = Arena([n * 4, n * 4])
        rc = getattr(self.lib, f"svt_dev_{self.family}_fill")(*self.head, self.a.part(1).data_ptr(), self.b.part(0).data_ptr(),
                                                             self.b.part(1).data_ptr(), self.a.part(0).data_ptr(),
                                                             self.nb - short, self.stream())
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        return self.a.guards_intact() and (self.b is None or self.b.guards_intact())

    def outputs_untouched(self):
        """out_col_ptr, every guard band and (when the fill was tried) the fill's outputs still hold 0xA5"""
        o, n = self.a.parts[1]
        return (self.guards_intact() and bool((self.a.mem[o:o + n] == 0xA5).all()) and self.nnz.value == -5
                and (self.b is None or self.b.untouched()))

    def arrays(self):
        return (self.a.part(1, torch.int64).cpu().numpy(), self.b.part(0, torch.int32).cpu().numpy(),
                self.b.part(1, torch.int32).cpu().numpy())

    def run(self, what):
        assert self.count() == 0, (what, self.lib.svt_last_error())
        assert self.guards_intact(), f"{what}: a guard band was written by the count"
        assert self.fill() == 0, (what, self.lib.svt_last_error())
        assert self.guards_intact(), f"{what}: a guard band was written by the fill"
        return self.arrays()


def _same(got, want, what):
    """CSC triples exactly: col_ptr, row_idx (ascending inside every column), int32 values 1 / NA"""
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    starts = np.zeros(got[1].size, bool)
    starts[got[0][:-1][np.diff(got[0]) > 0]] = True
    assert np.all((np.diff(got[1]) > 0) | starts[1:]), f"{what}: rows do not ascend inside a column"
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), f"{what}: values"
    assert np.all((got[2] == 1) | (got[2] == NA)), f"{what}: a value that is not TRUE or NA"


def _triple(R):
    torch.cuda.synchronize()
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


@pytest.mark.parametrize("name", ac.DEVICE_NAMES)
def test_merge_around_the_tile(tile, name):
    """every placement under != and < with double, integer and mixed values, and under & and | with values from
    {1, 0, NA}: count's out_col_ptr and nnz, the filled arrays, rows ascending, every guard band intact; the
    compositions DeviceCSC.compare / .logic give the same arrays"""
    from sparsearray_amd.api import COMPARE_OPCODES, LOGIC_OPCODES
    from sparsearray_amd.svt import LGLSXP
    c = ac.device_cases(tile)[name]
    for values in ("double", "integer", "mixed"):
        x, y, host, _ = _operands(c, values)
        for op in ("!=", "<"):
            what = f"{name}, {values} values, {op}"
            want = cc.device_expect("compare", op, *host, c.nrow, c.ncol)
            r = Raw("compare_merge", x, y, COMPARE_OPCODES[op])
            got = r.run(what)
            assert r.nnz.value == want[1].size, f"{what}: count"
            _same(got, want, what)
        R = x.compare("<", y)
        _same(_triple(R), want, f"{name}, {values} values, composition")
        assert R.Rtype == LGLSXP and R.nrow == c.nrow and R.ncol == c.ncol
    x, y, host, _ = _operands(c, "logical")
    for op in cc.LOGIC_OPS:
        what = f"{name}, {op}"
        want = cc.device_expect("logic", op, *host, c.nrow, c.ncol)
        r = Raw("logic_merge", x, y, LOGIC_OPCODES[op])
        got = r.run(what)
        assert r.nnz.value == want[1].size, f"{what}: count"
        _same(got, want, what)
    _same(_triple(x.logic("|", y)), want, f"{name}, | by the composition")
    if name == "straddling_pairs_cancel":                   # (proved without a GPU in tests/test_z_compare_cpu.py)
        kx, vx, ky, vy = cc.device_operands(c, "double")
        assert cc.device_expect("compare", "!=", kx, vx, ky, vy, c.nrow, c.ncol)[0][-1] == kx.size - 2


@pytest.mark.parametrize("name", ["one_column_holds_everything", "100000_empty_columns", "straddling_pairs_columns",
                                  "merged_length_+0_from_T", "merged_length_+1_from_T", "merged_length_2T", "all_match_int",
                                  "empty_both"])
def test_map_around_the_tile(tile, name):
    """the map on the x parts, double and integer values: a scalar that keeps everything (the result's col_ptr and
    row_idx are x's, every value is 1), one that keeps nothing, one that keeps about half; the composition agrees"""
    from sparsearray_amd.api import COMPARE_OPCODES
    from sparsearray_amd.svt import INTSXP, REALSXP
    c = ac.device_cases(tile)[name]
    for values in ("double", "integer"):
        x, _, _, (cp, ri, val) = _operands(c, values)
        assert not (val == 0).any()
        for op, s, st, keeps in (("!=", 0, "integer", "all"), (">", 1e9, "double", "none"), (">", 0, "integer", "half"),
                                 ("<=", -50.5, "double", "some")):
            what = f"{name}, {values} values, x {op} {s}"
            want = cc.map_expect(op, cp, ri, val, s, st, c.ncol)
            r = Raw("compare_map", x, None, COMPARE_OPCODES[op], s, INTSXP if st == "integer" else REALSXP)
            got = r.run(what)
            assert r.nnz.value == want[1].size, f"{what}: count"
            _same(got, want, what)
            if keeps == "all":
                assert np.array_equal(got[0], cp) and np.array_equal(got[1], ri) and np.all(got[2] == 1) and got[2].size == val.size
            if keeps == "none":
                assert got[1].size == 0 and not got[0].any()
            if keeps == "half" and val.size > 100:
                assert val.size // 4 < got[1].size < 3 * val.size // 4
        _same(_triple(x.compare("<=", -50.5)), want, f"{name}, {values} values, composition")
    lg = _device(c.nrow, (cp, ri, cc.logical_values(ri.size, 7)), logical=True)
    want = cc.map_expect("==", cp, ri, cc.logical_values(ri.size, 7), True, "logical", c.ncol)
    _same(_triple(lg.compare("==", True)), want, f"{name}, logical x == TRUE")


def test_same_call_twice_gives_the_same_bits(tile):
    c = ac.device_cases(tile)["one_column_holds_everything"]
    x, y, _, _ = _operands(c, "double")
    runs = []
    for _ in range(2):
        R = x.compare("!=", y).logic("&", x.compare(">", 0))
        runs.append(_triple(R) + _triple(x.compare("<", y)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("family", ["compare_merge", "logic_merge", "compare_map"])
def test_result_does_not_depend_on_what_the_workspace_held(tile, family):
    """0x00, 0xA5, 0xFF and the workspace another operation left behind give the same arrays; nothing is written
    outside the advertised bytes (the arena's guard bands, asserted by every run)"""
    from sparsearray_amd.api import COMPARE_OPCODES, LOGIC_OPCODES
    from sparsearray_amd.svt import REALSXP
    c = ac.device_cases(tile)["straddling_pairs_columns"]
    x, y, host, xh = _operands(c, "logical" if family == "logic_merge" else "double")
    if family == "compare_merge":
        make = lambda **k: Raw(family, x, y, COMPARE_OPCODES["<"], **k)                         # noqa: E731
        want = cc.device_expect("compare", "<", *host, c.nrow, c.ncol)
    elif family == "logic_merge":
        make = lambda **k: Raw(family, x, y, LOGIC_OPCODES["&"], **k)                            # noqa: E731
        want = cc.device_expect("logic", "&", *host, c.nrow, c.ncol)
    else:
        make = lambda **k: Raw(family, x, None, COMPARE_OPCODES[">"], 0.0, REALSXP, **k)        # noqa: E731
        want = cc.map_expect(">", *xh, 0.0, "double", c.ncol)
    for fill in (0x00, 0xA5, 0xFF):
        _same(make(ws_fill=fill).run(f"{family}, workspace of {fill:#x}"), want, f"{family}, workspace of {fill:#x}")
    r = make()
    r.run(family)
    other = ac.device_cases(tile)["all_match"]                                   # another operation in the same arena
    ox, oy, ohost, _ = _operands(other, "double")
    if r.nb >= r.lib.svt_dev_arith_merge_ws_bytes(ox.ncol, ox.nnz, oy.nnz):
        assert r.lib.svt_dev_compare_merge_count(ox.handle, oy.handle, COMPARE_OPCODES["!="],
                                                 torch.empty(ox.ncol + 1, dtype=torch.int64, device="cuda").data_ptr(),
                                                 ctypes.byref(ctypes.c_int64(0)), r.a.part(0).data_ptr(), r.nb, r.stream()) == 0
    _same(r.run(f"{family}, a used workspace"), want, f"{family}, a used workspace")


def test_statuses_leave_the_outputs_untouched(tile):
    """< 0: extents that differ, a workspace one byte short (count and fill), an unknown opcode, merge Compare with an op
    other than != < >, a map Compare whose scalar does not make 0 op s FALSE, Logic on operands that are not logical,
    a scalar type outside logical / integer / double; > 0: na_background.  Each leaves out_col_ptr, *out_nnz and every
    guard band as they were; none launches anything."""
    from sparsearray_amd.api import COMPARE_OPCODES as C, LOGIC_OPCODES as L
    from sparsearray_amd.device import _lib
    from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP
    lib = _lib()
    c = ac.device_cases(tile)["all_match"]
    x, y, _, _ = _operands(c, "double")
    xi, _, _, _ = _operands(c, "integer")
    lx, ly, _, _ = _operands(c, "logical")
    other_nrow = _device(c.nrow + 1, c.y)
    other_ncol = _device(c.nrow, (np.append(c.y[0], c.y[0][-1]), c.y[1], c.y[2]))
    l_other_nrow = _device(c.nrow + 1, (c.y[0], c.y[1], np.ones(c.y[1].size, np.int32)), logical=True)
    nan, na_int = float("nan"), float(NA)
    sparse = "result wouldn't be sparse"
    negative = ([(Raw("compare_merge", x, other_nrow, C["!="]), "non-conformable"),
                 (Raw("compare_merge", x, other_ncol, C["<"]), "non-conformable"),
                 (Raw("logic_merge", lx, l_other_nrow, L["&"]), "non-conformable"),
                 (Raw("compare_merge", x, y, C["!="], short=1), "workspace too small"),
                 (Raw("logic_merge", lx, ly, L["|"], short=1), "workspace too small"),
                 (Raw("compare_map", x, None, C[">"], 0.0, REALSXP, short=1), "workspace too small"),
                 (Raw("compare_merge", x, y, 0), "unknown operation"), (Raw("compare_merge", x, y, 7), "unknown operation"),
                 (Raw("compare_map", x, None, 0, 1.0, REALSXP), "unknown operation"),
                 (Raw("compare_map", x, None, 99, 1.0, REALSXP), "unknown operation"),
                 (Raw("logic_merge", lx, ly, 0), "unknown operation"), (Raw("logic_merge", lx, ly, 3), "unknown operation"),
                 (Raw("logic_merge", x, ly, L["&"]), "logical"), (Raw("logic_merge", lx, xi, L["|"]), "logical"),
                 (Raw("logic_merge", xi, xi, L["&"]), "logical"),
                 (Raw("compare_map", x, None, C[">"], 0.0, 16), "scalar must be of type"),
                 (Raw("compare_map", x, None, C[">"], 0.0, 0), "scalar must be of type")] +
                [(Raw("compare_merge", x, y, C[op]), sparse) for op in ("==", "<=", ">=")] +
                [(Raw("compare_map", a, None, C[op], s, st), sparse) for a in (x, xi, lx) for op, s, st in
                 (("==", 0.0, REALSXP), (">=", 0.0, REALSXP), ("<", 1.0, REALSXP), ("<=", 0, INTSXP), (">=", -1, INTSXP),
                  ("!=", 2.5, REALSXP), (">", -1e-300, REALSXP), ("<", float("inf"), REALSXP), (">", nan, REALSXP),
                  ("!=", nan, REALSXP), ("==", nan, REALSXP), (">", na_int, INTSXP), ("!=", na_int, LGLSXP), ("==", 0, LGLSXP),
                  ("!=", 1, LGLSXP))])
    for r, msg in negative:
        assert r.count() < 0 and msg.encode() in lib.svt_last_error(), (msg, lib.svt_last_error())
        assert r.outputs_untouched() and r.a.untouched(), msg
        r.nnz.value = 3                                     # the fill of the same call refuses as well
        assert r.fill(short=r.short) < 0 and r.b.untouched(), msg
    # (-2^31 as a DOUBLE scalar is a number, not NA: x < -2147483648.0 is an ordinary comparison)
    assert Raw("compare_map", x, None, C["<"], na_int, REALSXP).count() == 0
    r = Raw("compare_merge", x, y, C["!="])
    assert r.count() == 0
    assert r.fill(short=1) < 0 and b"workspace too small" in lib.svt_last_error() and r.b.untouched()
    # > 0: "not supported here"
    na = _device(c.nrow, c.x)
    off = 4 + 4 + 3 * 8 + 3 * 8              # struct svt_dev_csc: Rtype, owned, three extents, three pointers, na_background
    ctypes.cast(na._h, ctypes.POINTER(ctypes.c_int32))[off // 4] = 1
    lna = _device(c.nrow, (c.x[0], c.x[1], np.ones(c.x[1].size, np.int32)), logical=True)
    ctypes.cast(lna._h, ctypes.POINTER(ctypes.c_int32))[off // 4] = 1
    for r in (Raw("compare_merge", na, y, C["!="]), Raw("compare_merge", x, na, C["<"]),
              Raw("compare_map", na, None, C[">"], 0.0, REALSXP), Raw("logic_merge", lna, ly, L["&"]),
              Raw("logic_merge", lx, lna, L["|"])):
        assert r.count() > 0 and b"NaArray" in lib.svt_last_error(), lib.svt_last_error()
        assert r.outputs_untouched() and r.a.untouched()
    # the compositions answer the same way, and the stream is sound after all of it
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    for f, kind in ((lambda: x.compare("==", y), SparseArrayError), (lambda: x.compare(">=", 0), SparseArrayError),
                    (lambda: x.logic("&", y), SparseArrayError), (lambda: na.compare(">", 0), SparseArrayUnsupported)):
        with pytest.raises(kind) as e:
            f()
        assert isinstance(e.value, SparseArrayUnsupported) == (kind is SparseArrayUnsupported)
    _, _, host, _ = _operands(c, "double")
    _same(Raw("compare_merge", x, y, C["!="]).run("after the statuses"), cc.device_expect("compare", "!=", *host, c.nrow, c.ncol),
          "after the statuses")


# ---------------------------------------------------------------------------
# chained: the logical operands made on the device feed the statistics, Logic, t() and subset
# ---------------------------------------------------------------------------
def test_chained_device_made_operands(tile):
    from sparsearray_amd.device import colstats, rowstats
    from sparsearray_amd.svt import LGLSXP
    nrow, ncol = 97, 64
    rng = np.random.default_rng(77)
    ka = np.sort(rng.choice(nrow * ncol, size=tile + 300, replace=False))
    kb = np.sort(np.concatenate([rng.choice(ka, size=tile // 2, replace=False),
                                 rng.choice(np.setdiff1d(np.arange(nrow * ncol), ka), size=tile // 2, replace=False)]))
    va = ac._vals(ka.size, 78)
    vb = ac._vals(kb.size, 79)
    equal = np.isin(kb, ka) & (np.arange(kb.size) % 2 == 0)                  # some of the shared positions hold equal values
    vb[equal] = va[np.searchsorted(ka, kb[equal])]
    A, B = _device(nrow, ac._csc(ka, va, nrow, ncol)), _device(nrow, ac._csc(kb, vb, nrow, ncol))
    dA, dB = np.zeros(nrow * ncol), np.zeros(nrow * ncol)
    dA[ka], dB[kb] = va, vb
    dA, dB = dA.reshape(ncol, nrow).T, dB.reshape(ncol, nrow).T              # nrow x ncol
    pos = A.compare(">", 0)
    sums, _ = colstats(pos, "sum")
    rsums, _ = rowstats(pos, "sum")
    torch.cuda.synchronize()
    assert np.array_equal(sums.cpu().numpy(), (dA > 0).sum(axis=0)) and np.array_equal(rsums.cpu().numpy(), (dA > 0).sum(axis=1))
    assert 0 < int((dA > 0).sum()) < ka.size
    both = A.compare("!=", B).logic("&", pos)
    want = (dA != dB) & (dA > 0)
    assert 0 < int(want.sum()) < int((dA > 0).sum()) and (dA == dB)[dA != 0].any()

    def dense(R, shape):
        cp, ri, val = _triple(R)
        assert R.Rtype == LGLSXP and np.all(val == 1)
        out = np.zeros(shape, bool)
        out[ri, np.repeat(np.arange(shape[1]), np.diff(cp))] = True
        return out

    assert np.array_equal(dense(both, (nrow, ncol)), want)
    assert np.array_equal(dense(both.t(), (ncol, nrow)), want.T)
    rows, cols = [5, 1, 1, 90, 17, 44], list(range(ncol - 1, 0, -3))
    assert np.array_equal(dense(both.subset(rows, cols), (len(rows), len(cols))), want[np.ix_(rows, cols)])
    assert np.array_equal(colstats(both.t(), "sum")[0].cpu().numpy(), want.sum(axis=1))
