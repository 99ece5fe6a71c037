"""pmin() / pmax() and is.na() / is.nan() / is.infinite() on the GPU: the two new rules on the merge, map and sweep
families of kernels_arith.hip through the count and fill calls with the test's own guarded buffers, the compositions of
DeviceCSC, the reference's own chain composed from the existing device methods, and the host entry points behind
Session -- every result compared bit for bit (col_ptr, row_idx and the values as integers) with the numpy expectations
of tests/pminmax_cases.py.  No operand has more than about three tiles of entries."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import pminmax_cases as pc
import sweep_cases as sw
from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SVT_SparseArray

torch = pytest.importorskip("torch")
from sparsearray_amd.device import arith_tile, sweep_form          # noqa: E402
pytestmark = pytest.mark.gpu

GUARD = 64          # guard words on either side of every output array
LGLSXP, INTSXP, REALSXP = 10, 13, 14
RTYPE = {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}
PAIRS = [(tx, ty) for tx in pc.TYPES for ty in pc.TYPES]
VARIANTS = [(op, na_rm) for op in pc.OPS for na_rm in (False, True)]


@pytest.fixture(scope="module")
def T(hip):
    return arith_tile()


def _code(op, na_rm):
    from sparsearray_amd.api import PMINMAX_NA_RM, PMINMAX_OPCODES
    return PMINMAX_OPCODES[op] | (PMINMAX_NA_RM if na_rm else 0)


def _device(nrow, csc, t):
    from sparsearray_amd.device import DeviceCSC
    cp, ri, val = csc
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val, dtype=pc.np_dtype(t)), device="cuda"), logical=t == "logical")


def _pair(nrow, ncol, kx, vx, tx, ky, vy, ty):
    return _device(nrow, ac._csc(kx, vx, nrow, ncol), tx), _device(nrow, ac._csc(ky, vy, nrow, ncol), ty)


def _host(R):
    torch.cuda.synchronize()
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


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
    """One operation through its count and fill calls with the test's own buffers: a poisoned workspace of the advertised
    size followed by a guard band, every output between guard words.  ``family``: "pminmax_merge", "pminmax_map",
    "pminmax_sweep" or "isfun_map"; ``args``: what the two calls take before the outputs."""

    def __init__(self, family, args, ncol, nb, keep=()):
        from sparsearray_amd.device import _lib, _stream
        self.lib, self.stream, self.keep = _lib(), _stream, keep
        self.count_fn, self.fill_fn = getattr(self.lib, f"svt_dev_{family}_count"), getattr(self.lib, f"svt_dev_{family}_fill")
        self.family, self.sweep, self.args, self.nb = family, family == "pminmax_sweep", args, nb
        self.ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cp = Guarded(ncol + 1, torch.int64, -77)
        self.nnz, self.bad = ctypes.c_int64(-5), ctypes.c_int64(-9)

    def count(self, short=0):
        bad = (ctypes.byref(self.bad),) if self.sweep else ()
        rc = self.count_fn(*self.args, self.cp.ptr(), ctypes.byref(self.nnz), *bad, self.ws.data_ptr(), self.nb - short, self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, dtype, short=0):
        n = max(self.nnz.value, 0)
        self.ri, self.vv = Guarded(n, torch.int32, -77), Guarded(n, dtype, 77)
        rc = self.fill_fn(*self.args, self.cp.ptr(), self.ri.ptr(), self.vv.ptr(), self.ws.data_ptr(), self.nb - short, self.stream())
        torch.cuda.synchronize()
        return rc

    def ws_guard_intact(self):
        return bool((self.ws[self.nb:] == 0xA5).all())

    def ws_untouched(self):
        return bool((self.ws == 0xA5).all())

    def arrays(self):
        return self.cp.body(), self.ri.body(), self.vv.body()

    def run(self, want, t, what):
        """count, fill, the guards and the expectation; returns the arrays"""
        assert self.count() == 0, (what, self.lib.svt_last_error())
        assert self.nnz.value == want[1].size and np.array_equal(self.cp.body(), want[0]), f"{what}: count"
        assert self.cp.intact() and self.ws_guard_intact() and (not self.sweep or self.bad.value == -1)
        assert self.fill(torch.float64 if t == "double" else torch.int32) == 0, (what, self.lib.svt_last_error())
        assert self.cp.intact() and self.ri.intact() and self.vv.intact() and self.ws_guard_intact(), what
        pc.same(self.arrays(), want, what)
        return self.arrays()


def _raw_merge(x, y, op, na_rm):
    from sparsearray_amd.device import _lib
    return Raw("pminmax_merge", (x.handle, y.handle, _code(op, na_rm)), x.ncol, _lib().svt_dev_arith_merge_ws_bytes(x.ncol, x.nnz, y.nnz))


def _raw_map(x, op, na_rm, s, s_type):
    from sparsearray_amd.device import _lib
    return Raw("pminmax_map", (x.handle, _code(op, na_rm), float(s), RTYPE[s_type]), x.ncol, _lib().svt_dev_arith_map_ws_bytes(x.ncol, x.nnz))


def _raw_sweep(x, op, na_rm, stats, s_type, form):
    from sparsearray_amd.device import _lib
    st = torch.as_tensor(np.ascontiguousarray(stats), device="cuda")
    return Raw("pminmax_sweep", (x.handle, _code(op, na_rm), st.data_ptr(), RTYPE[s_type], st.numel(), *form), x.ncol,
               _lib().svt_dev_sweep_ws_bytes(x.ncol, x.nnz), keep=(st,))


def _raw_isfun(x, fn):
    from sparsearray_amd.api import ISFUN_OPCODES
    from sparsearray_amd.device import _lib
    return Raw("isfun_map", (x.handle, ISFUN_OPCODES.get(fn, fn)), x.ncol, _lib().svt_dev_arith_map_ws_bytes(x.ncol, x.nnz))


def _scalar(s, s_type):
    return bool(s) if s_type == "logical" else int(s) if s_type == "integer" else float(s)


# ---------------------------------------------------------------------------
# 1. the value table: every (x, y) combination a cell, implicit zeros on either side
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tx,ty", PAIRS)
def test_value_table_merge(T, tx, ty):
    nrow, ncol, kx, vx, ky, vy = pc.table_pair(tx, ty)
    x, y = _pair(nrow, ncol, kx, vx, tx, ky, vy, ty)
    for op, na_rm in VARIANTS:
        want, t = pc.expect_merge(op, na_rm, nrow, ncol, kx, vx, tx, ky, vy, ty)
        what = f"{op}({tx}, {ty}, na_rm={na_rm})"
        _raw_merge(x, y, op, na_rm).run(want, t, what)
        R = getattr(x, op)(y, na_rm=na_rm)
        assert R.Rtype == RTYPE[t] and (R.nrow, R.ncol) == (nrow, ncol)
        pc.same(_host(R), want, what + ", composition")


@pytest.mark.parametrize("tx,ty", PAIRS)
def test_value_table_scalar_map(T, tx, ty):
    """every table value of x against every scalar of the table that keeps the result sparse"""
    X = pc.TABLE[tx]
    csc = (np.array([0, X.size, X.size], np.int64), np.arange(X.size, dtype=np.int32), X)
    x = _device(X.size, csc, tx)
    for op, na_rm in VARIANTS:
        for s in pc.TABLE[ty]:
            if not pc.keeps_sparse(op, s, ty):
                continue
            want, t = pc.expect_map(op, na_rm, csc, tx, s, ty)
            what = f"{op}({tx}, {s!r} {ty}, na_rm={na_rm})"
            _raw_map(x, op, na_rm, s, ty).run(want, t, what)
            R = getattr(x, op)(_scalar(s, ty), na_rm=na_rm)
            assert R.Rtype == RTYPE[t]
            pc.same(_host(R), want, what + ", composition")


# ---------------------------------------------------------------------------
# 2. placement; two runs give the same bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tx,ty", [("double", "double"), ("integer", "integer"), ("integer", "double"), ("double", "logical"),
                                   ("logical", "logical")])
def test_placement_merge(T, tx, ty):
    nrow, ncol, kx, vx, ky, vy = pc.placement_pair(T, tx, ty)
    assert kx.size + ky.size == 3 * T + 5
    x, y = _pair(nrow, ncol, kx, vx, tx, ky, vy, ty)
    for op, na_rm in VARIANTS:
        want, t = pc.expect_merge(op, na_rm, nrow, ncol, kx, vx, tx, ky, vy, ty)
        what = f"placement {op}({tx}, {ty}, na_rm={na_rm})"
        first = _raw_merge(x, y, op, na_rm).run(want, t, what)
        for _ in range(2):
            R = getattr(x, op)(y, na_rm=na_rm)
            assert R.Rtype == RTYPE[t]
            for a, b in zip(_host(R), first):
                assert a.dtype == b.dtype and np.array_equal(pc.bits(a), pc.bits(b)), what


@pytest.mark.parametrize("name", ["x_empty", "y_empty", "both_empty", "ncol_0", "nd_2x3x2"])
def test_empty_sides_and_an_nd_operand(T, name):
    nrow, ncol, kx, vx, ky, vy = pc.small_pairs(T)[name]
    x, y = _pair(nrow, ncol, kx, vx, "double", ky, vy, "double")
    for op, na_rm in VARIANTS:
        want, t = pc.expect_merge(op, na_rm, nrow, ncol, kx, vx, "double", ky, vy, "double")
        _raw_merge(x, y, op, na_rm).run(want, t, f"{name} {op} {na_rm}")
        pc.same(_host(getattr(x, op)(y, na_rm=na_rm)), want, f"{name} {op} {na_rm}, composition")


# ---------------------------------------------------------------------------
# 3. the reference's chain composed from the existing device methods, and the README's clamp chain
# ---------------------------------------------------------------------------
def _chain(x, y, op, na_rm):
    """.pminmax2 on the device: compare -> nzwhich -> x[L] -> x[L] <- v -> is.na -> nzwhich -> x[L] -> x[L] <- v"""
    replace_idx = y.compare("<" if op == "pmin" else ">", x).nzwhich()
    ans = x.subassign_lindex(replace_idx, y.subset_lindex(replace_idx))
    restore_idx = (y if na_rm else x).is_na().nzwhich()
    return ans.subassign_lindex(restore_idx, x.subset_lindex(restore_idx))


def test_one_pass_equals_the_eight_step_chain(T):
    nrow, ncol, kx, vx, ky, vy = pc.random_pair()
    x, y = _pair(nrow, ncol, kx, vx, "double", ky, vy, "double")
    for op, na_rm in VARIANTS:
        one, chain = _host(getattr(x, op)(y, na_rm=na_rm)), _host(_chain(x, y, op, na_rm))
        want, _ = pc.expect_merge(op, na_rm, nrow, ncol, kx, vx, "double", ky, vy, "double")
        pc.same(one, want, f"{op} na_rm={na_rm}")
        pc.same(chain, one, f"{op} na_rm={na_rm}: the chain against the one pass")


def test_scalar_pmin_equals_the_clamp_chain(T):
    nrow, ncol, kx, vx, _, _ = pc.random_pair()
    vx = np.where(np.isnan(vx), 7.5, vx)                               # an operand without NAs
    csc = ac._csc(kx, vx, nrow, ncol)
    x = _device(nrow, csc, "double")
    for s in (10.0, 0.25, 49.99, 1000.0):
        clamp = _host(x.subassign_lindex(x.compare(">", s).nzwhich(), s))
        one = _host(x.pmin(s))
        pc.same(one, pc.expect_map("pmin", False, csc, "double", s, "double")[0], f"pmin(x, {s})")
        pc.same(clamp, one, f"the clamp chain against pmin(x, {s})")


# ---------------------------------------------------------------------------
# 4. scalar map and sweep on the placement operand
# ---------------------------------------------------------------------------
def _placement_operand(T, t):
    nrow, ncol, kx, vx, _, _ = pc.placement_pair(T, t, t)
    return nrow, ncol, ac._csc(kx, vx, nrow, ncol)


@pytest.mark.parametrize("t", ["double", "integer"])
def test_scalar_map_across_tiles(T, t):
    """values on both sides of the scalar, s == 0 (what is beyond it disappears), s == +-Inf (the identity, bit for bit,
    but for the stored zeros), na_rm (an NA entry becomes the scalar)"""
    nrow, ncol, csc = _placement_operand(T, t)
    assert csc[2].size > T
    x = _device(nrow, csc, t)
    for op, na_rm in VARIANTS:
        sign = 1 if op == "pmin" else -1
        for s, st in ((sign * 300.25, "double"), (sign * 300, "integer"), (0.0, "double"), (0, "integer"), (sign * np.inf, "double")):
            want, rt = pc.expect_map(op, na_rm, csc, t, s, st)
            what = f"{op}({t}, {s!r} {st}, na_rm={na_rm})"
            got = _raw_map(x, op, na_rm, s, st).run(want, rt, what)
            pc.same(_host(getattr(x, op)(_scalar(s, st), na_rm=na_rm)), want, what + ", composition")
            if s == 0:
                beyond = (csc[2] > 0) if op == "pmin" else (csc[2] < 0)
                assert beyond.any() and got[1].size <= csc[2].size - int((beyond & ~pc.isna(csc[2])).sum())
            if np.isinf(s) and not na_rm and t == "double":
                stored = csc[2] != 0
                assert np.array_equal(pc.bits(got[2]), pc.bits(csc[2][stored | np.isnan(csc[2])]))
            if na_rm and s != 0:
                assert not pc.isna(got[2]).any() and pc.isna(csc[2]).any()


@pytest.mark.parametrize("t,st", [("double", "double"), ("integer", "integer"), ("integer", "double"), ("double", "logical")])
def test_sweep_rows_and_leaves(T, t, st):
    nrow, ncol, csc = _placement_operand(T, t)
    x, dim = _device(nrow, csc, t), (nrow, ncol)
    for margin in (1, 2):
        n = sw.stats_length(dim, margin)
        for op, na_rm in VARIANTS:
            k = np.random.default_rng(margin).permutation(n)
            if st == "logical":
                stats = ((k % 2) * (1 if op == "pmin" else 0)).astype(np.int32)
            else:
                stats = ((k % 700) * (1 if op == "pmin" else -1)).astype(pc.np_dtype(st)) * (0.75 if st == "double" else 1)
            want, rt = pc.expect_sweep(op, na_rm, csc, t, dim, margin, stats, st)
            what = f"sweep {op}({t}, {st}, margin {margin}, na_rm={na_rm})"
            _raw_sweep(x, op, na_rm, stats, st, sweep_form(dim, margin)).run(want, rt, what)
            R = x.sweep(op, torch.as_tensor(stats, device="cuda"), margin, logical=st == "logical", na_rm=na_rm)
            assert R.Rtype == RTYPE[rt]
            pc.same(_host(R), want, what + ", composition")


def test_sweep_over_two_dimensions_of_an_nd_operand(T):
    """margin c(2, 3) of a (5, 4, 3, 2) array: a cap per (j, k)"""
    for t in ("double", "integer"):
        nrow, csc = sw.dense_4d(t)
        x = _device(nrow, csc, t)
        for margin in ((2, 3), 3, (1, 2)):
            stats = (np.arange(sw.stats_length(sw.DIM_4D, margin)) % 9).astype(np.float64) * 0.5
            for op, na_rm in VARIANTS:
                s = stats if op == "pmin" else -stats
                want, rt = pc.expect_sweep(op, na_rm, csc, t, sw.DIM_4D, margin, s, "double")
                extents = [sw.DIM_4D[k - 1] for k in sw.as_margin(margin)]
                given = torch.as_tensor(s.reshape(extents, order="F"), device="cuda")
                pc.same(_host(x.sweep(op, given, margin, dim=sw.DIM_4D, na_rm=na_rm)), want, f"{t} {op} margin {margin}")


# ---------------------------------------------------------------------------
# 5. refusals: nothing is written outside the workspace
# ---------------------------------------------------------------------------
def test_a_scalar_on_the_wrong_side_of_zero_is_refused(T):
    nrow, ncol, csc = _placement_operand(T, "double")
    x = _device(nrow, csc, "double")
    for op, s, st in (("pmin", -1.0, "double"), ("pmin", float("nan"), "double"), ("pmin", NA_real, "double"), ("pmin", -1, "integer"),
                      ("pmin", NA_integer, "integer"), ("pmin", NA_integer, "logical"), ("pmax", 0.5, "double"), ("pmax", 1, "logical"),
                      ("pmax", float("nan"), "double"), ("pmin", -np.inf, "double"), ("pmax", np.inf, "double")):
        for na_rm in (False, True):
            r = _raw_map(x, op, na_rm, s, st)
            assert r.count() < 0 and b"result wouldn't be sparse" in r.lib.svt_last_error(), (op, s, st)
            assert r.cp.untouched() and r.nnz.value == -5 and r.ws_untouched()
    with pytest.raises(SparseArrayError, match=r"pmin\(0, -1\.0\) is not 0 \(result wouldn't be sparse\)"):
        x.pmin(-1.0)
    with pytest.raises(SparseArrayError, match=r"pmax\(0, 2\) is not 0"):
        x.pmax(2)


@pytest.mark.parametrize("op,st,value", [("pmin", "double", -0.5), ("pmin", "double", float("nan")), ("pmin", "integer", NA_integer),
                                        ("pmin", "integer", -1), ("pmax", "double", 0.5), ("pmax", "double", NA_real),
                                        ("pmax", "logical", 1), ("pmax", "logical", NA_integer)])
def test_a_vector_element_on_the_wrong_side_is_refused_on_the_device(T, op, st, value):
    """one bad element at a position past the first tile (and a later one): the smallest index is named"""
    nrow, ncol, csc = _placement_operand(T, "double")
    x, dim = _device(nrow, csc, "double"), (nrow, ncol)
    assert nrow > T + 600
    first, second = T + 500, T + 77
    stats = np.zeros(nrow, dtype=pc.np_dtype(st))
    stats[[first, second]] = value
    for na_rm in (False, True):
        r = _raw_sweep(x, op, na_rm, stats, st, sweep_form(dim, 1))
        assert r.count() < 0 and r.bad.value == second, (r.bad.value, r.lib.svt_last_error())
        assert f"element {second} ".encode() in r.lib.svt_last_error()
        assert r.cp.untouched() and r.nnz.value == -5 and r.ws_guard_intact()
    with pytest.raises(SparseArrayError, match=rf"stats\[{second}\] = .*does not keep the result sparse"):
        x.sweep(op, torch.as_tensor(stats, device="cuda"), 1, logical=st == "logical")
    good = np.zeros(nrow, dtype=pc.np_dtype(st))
    want, rt = pc.expect_sweep(op, False, csc, "double", dim, 1, good, st)
    _raw_sweep(x, op, False, good, st, sweep_form(dim, 1)).run(want, rt, "a vector of zeros")


def test_statuses_leave_the_outputs_untouched(T):
    """< 0: extents that differ, a workspace one byte short (count and fill), unknown opcodes, a scalar type outside
    logical / integer / double; > 0: na_background.  Each leaves out_col_ptr, *out_nnz and every guard band as they were."""
    nrow, ncol, kx, vx, ky, vy = pc.placement_pair(T, "double", "double")
    x, y = _pair(nrow, ncol, kx, vx, "double", ky, vy, "double")
    other = _device(nrow, ac._csc(kx[kx < 30 * nrow], vx[kx < 30 * nrow], nrow, 30), "double")
    taller = _device(nrow + 1, ac._csc(kx % nrow + (kx // nrow) * (nrow + 1), vx, nrow + 1, ncol), "double")
    stats = torch.zeros(ncol, dtype=torch.float64, device="cuda")
    form = (stats.data_ptr(), REALSXP, ncol, 0, 1, ncol)
    from sparsearray_amd.device import _lib
    nb_merge, nb_map = _lib().svt_dev_arith_merge_ws_bytes(ncol, x.nnz, y.nnz), _lib().svt_dev_arith_map_ws_bytes(ncol, x.nnz)
    negative = [(Raw("pminmax_merge", (x.handle, other.handle, 1), ncol, nb_merge), "non-conformable"),
                (Raw("pminmax_merge", (x.handle, taller.handle, 1), ncol, nb_merge), "non-conformable"),
                (Raw("pminmax_merge", (x.handle, y.handle, 0), ncol, nb_merge), "unknown operation"),
                (Raw("pminmax_merge", (x.handle, y.handle, 3), ncol, nb_merge), "unknown operation"),
                (Raw("pminmax_merge", (x.handle, y.handle, 8 | 1), ncol, nb_merge), "unknown operation"),
                (Raw("pminmax_map", (x.handle, 4, 1.0, REALSXP), ncol, nb_map), "unknown operation"),
                (Raw("pminmax_map", (x.handle, 1, 1.0, 16), ncol, nb_map), "the scalar must be of type"),
                (Raw("pminmax_map", (x.handle, 1, float(2 ** 40), INTSXP), ncol, nb_map), "not a value of its integer"),
                (Raw("pminmax_map", (x.handle, 1, 0.5, INTSXP), ncol, nb_map), "not a value of its integer"),
                (Raw("pminmax_map", (x.handle, 2, -2147483649.0, LGLSXP), ncol, nb_map), "not a value of its integer"),
                (Raw("pminmax_sweep", (x.handle, 7, *form), ncol, nb_map), "unknown operation"),
                (Raw("pminmax_sweep", (x.handle, 1, stats.data_ptr(), 16, ncol, 0, 1, ncol), ncol, nb_map), "must be of type"),
                (_raw_isfun(x, 0), "unknown operation"), (_raw_isfun(x, 4), "unknown operation")]
    for r, msg in negative:
        assert r.count() < 0 and msg.encode() in r.lib.svt_last_error(), (msg, r.lib.svt_last_error())
        assert r.cp.untouched() and r.nnz.value == -5 and r.ws_untouched()
    shorts = [_raw_merge(x, y, "pmin", False), _raw_map(x, "pmax", True, 0.0, "double"),
              Raw("pminmax_sweep", (x.handle, 1, *form), ncol, nb_map), _raw_isfun(x, "is.na")]
    for r in shorts:
        assert r.count(short=1) < 0 and b"workspace too small" in r.lib.svt_last_error()
        assert r.cp.untouched() and r.nnz.value == -5 and r.ws_untouched()
        assert r.count() == 0
        assert r.fill(torch.int32 if r.family == "isfun_map" else torch.float64, short=1) < 0
        assert b"workspace too small" in r.lib.svt_last_error() and r.ri.untouched() and r.vv.untouched()
    na = _device(nrow, ac._csc(kx, vx, nrow, ncol), "double")
    off = 4 + 4 + 3 * 8 + 3 * 8              # struct svt_dev_csc: Rtype, owned, three extents, three pointers, na_background
    ctypes.cast(na._h, ctypes.POINTER(ctypes.c_int32))[off // 4] = 1
    for r in (Raw("pminmax_merge", (na.handle, y.handle, 1), ncol, nb_merge), Raw("pminmax_merge", (x.handle, na.handle, 2), ncol, nb_merge),
              _raw_map(na, "pmin", False, 1.0, "double"), Raw("pminmax_sweep", (na.handle, 1, *form), ncol, nb_map), _raw_isfun(na, "is.na")):
        assert r.count() > 0 and b"NaArray" in r.lib.svt_last_error()
        assert r.cp.untouched() and r.nnz.value == -5 and r.ws_untouched()


# ---------------------------------------------------------------------------
# 6. is.na / is.nan / is.infinite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("t", pc.TYPES)
def test_is_functions(T, t):
    nrow, csc = pc.isfun_operand(T, t)
    x = _device(nrow, csc, t)
    for fn, method in zip(pc.ISFUNS, ("is_na", "is_nan", "is_infinite")):
        want = pc.expect_isfun(fn, csc)
        got = _raw_isfun(x, fn).run(want, "logical", f"{fn}({t})")
        R = getattr(x, method)()
        assert R.Rtype == LGLSXP
        pc.same(_host(R), want, f"{fn}({t}), composition")
        assert np.all(got[2] == 1)
        assert (got[1].size > 0) == (t == "double" or fn == "is.na")
    if t == "double":
        assert x.is_na().nnz > x.is_nan().nnz > 0 and x.is_infinite().nnz > 0


# ---------------------------------------------------------------------------
# 7. host level: Session.pmin / pmax / is_na / sweep through the C ABI
# ---------------------------------------------------------------------------
def _svt(nrow, ncol, keys, vals, t, dim=None, dimnames=None):
    cp, ri, v = ac._csc(keys, vals, nrow, ncol)
    return SVT_SparseArray.from_csc(dim or (nrow, ncol), t, cp, ri, v.astype(pc.np_dtype(t)), dimnames=dimnames)


def _check_session(res, want, t, dim, what):
    (cp, ri, v) = want
    assert res.type == t and tuple(res.dim) == tuple(dim), what
    ref = SVT_SparseArray.from_csc(dim, t, cp, ri, v)
    (gd, gs), (wd, ws) = ac.dense_nd(res), ac.dense_nd(ref)
    assert np.array_equal(gs, ws), f"{what}: stored positions"
    assert gd.dtype == wd.dtype and np.array_equal(pc.bits(gd), pc.bits(wd)), f"{what}: values"


def test_session_pmin_pmax_and_the_three_object_fold(hip, T):
    tx, ty = "integer", "double"
    nrow, ncol, kx, vx, ky, vy = pc.table_pair(tx, ty)
    names = [None, [f"c{j}" for j in range(ncol)]]
    x, y = _svt(nrow, ncol, kx, vx, tx), _svt(nrow, ncol, ky, vy, ty, dimnames=names)
    for op, na_rm in VARIANTS:
        want, t = pc.expect_merge(op, na_rm, nrow, ncol, kx, vx, tx, ky, vy, ty)
        res = getattr(hip, op)(x, y, na_rm=na_rm)
        _check_session(res, want, t, (nrow, ncol), f"Session.{op}(na_rm={na_rm})")
        assert res.dimnames is not None and list(res.dimnames[1]) == names[1]          # the first object that has them
    # three objects: pmin(a, pmin(b, c)), the middle one an N-d-shaped call away from the first
    nrow, ncol, ka, va, kb, vb = pc.random_pair(seed=9, nrow=50, ncol=12, n=240)
    kc, vc = ka[::2], -va[::2]
    a, b, c = _svt(nrow, ncol, ka, va, "double"), _svt(nrow, ncol, kb, vb, "double"), _svt(nrow, ncol, kc, vc, "double")
    for op, na_rm in VARIANTS:
        (cp, ri, v), _ = pc.expect_merge(op, na_rm, nrow, ncol, kb, vb, "double", kc, vc, "double")
        inner_keys = np.repeat(np.arange(ncol), np.diff(cp)) * nrow + ri
        want, t = pc.expect_merge(op, na_rm, nrow, ncol, ka, va, "double", inner_keys, v, "double")
        _check_session(getattr(hip, op)(a, None, b, c, na_rm=na_rm), want, t, (nrow, ncol), f"Session.{op}(a, b, c)")
    # the scalar form, on either side, and a cap per column
    csc = ac._csc(ka, va, nrow, ncol)
    want, t = pc.expect_map("pmin", True, csc, "double", 10.0, "double")
    _check_session(hip.pmin(a, 10.0, na_rm=True), want, t, (nrow, ncol), "Session.pmin(a, 10)")
    _check_session(hip.pmin(10.0, a, na_rm=True), want, t, (nrow, ncol), "Session.pmin(10, a)")
    caps = np.arange(ncol) * 2.5
    want, t = pc.expect_sweep("pmin", False, csc, "double", (nrow, ncol), 2, caps, "double")
    _check_session(hip.sweep(a, 2, caps, "pmin"), want, t, (nrow, ncol), "Session.sweep(pmin)")
    with pytest.raises(SparseArrayError, match="non-conformable arrays"):
        hip.pmin(a, x)


def test_session_pmin_on_an_nd_object(hip):
    nrow, ncol, kx, vx, ky, vy = pc.small_pairs(arith_tile())["nd_2x3x2"]
    x, y = _svt(nrow, ncol, kx, vx, "double", dim=(2, 3, 2)), _svt(nrow, ncol, ky, vy, "double", dim=(2, 3, 2))
    want, t = pc.expect_merge("pmax", False, nrow, ncol, kx, vx, "double", ky, vy, "double")
    _check_session(hip.pmax(x, y), want, t, (2, 3, 2), "Session.pmax, 2 x 3 x 2")


@pytest.mark.parametrize("t", pc.TYPES)
def test_session_is_functions(hip, T, t):
    nrow, csc = pc.isfun_operand(T, t)
    ncol = csc[0].size - 1
    x = SVT_SparseArray.from_csc((nrow, ncol), t, *csc, dimnames=[None, [str(j) for j in range(ncol)]])
    for fn, method in zip(pc.ISFUNS, ("is_na", "is_nan", "is_infinite")):
        res = getattr(hip, method)(x)
        _check_session(res, pc.expect_isfun(fn, csc), "logical", (nrow, ncol), f"Session.{method}({t})")
        assert res.dimnames is not None and list(res.dimnames[1]) == [str(j) for j in range(ncol)]
