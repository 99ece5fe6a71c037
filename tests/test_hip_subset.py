"""x[i, j] by an N-index on the GPU (kernels_subset.hip; include/svt_hip.h, svt_dev_subset_*): the shared cases of
tests/subset_cases.py through the host entry point, and the two device primitives on operands placed around the tile
T = svt_dev_subset_tile() -- against numpy on the dense matrix, ``dense[np.ix_(i, j)]``, at tolerance 0 (values as
bits).  No operand holds more than about 3 T nonzeros; one gather's RESULT holds 2100 T (the fixed grid's second trip).

The device-level reference subsets a dense matrix of TRACERS (entry number + 1, 0 where nothing is stored) with
np.ix_ and reads the result's CSC arrays off it: which entry lands where, so that values are compared as bits."""
import ctypes

import numpy as np
import pytest

import subset_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 4096


# ---------------------------------------------------------------------------
# shared cases, host entry point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_shared_case(hip, oracle, name):
    _, op, i, j = sc.BY_NAME[name]
    x, _, _ = sc.operand(op)
    res = hip.subset(x, i, j)
    sc.check(res, name, "hip ")
    sc.same_object(res, oracle.subset(x, i, j), f"hip vs oracle, {name}")


def test_three_dimensions_are_not_supported_here(hip):
    from sparsearray_amd import SparseArrayUnsupported, SVT_SparseArray
    x = SVT_SparseArray.from_dense(np.arange(24, dtype=np.float64).reshape(2, 3, 4))
    with pytest.raises(SparseArrayUnsupported, match="2-D"):
        hip.subset(x, [1], [1], [1])


def test_host_entry_checks_its_subscripts_before_the_upload(hip):
    """the entry point itself (not Session.subset's checks): NA and out-of-range are errors, and the operand was not
    uploaded for them -- the resident cache sees no miss"""
    from sparsearray_amd import NA_integer, SparseArrayError
    x, _, _ = sc.operand("integer")
    call = hip._call
    hip.resident_clear()
    hip.resident_set_limit(1 << 20)
    try:
        before = hip.resident_stats()
        for i, j in (([1, 30], None), (None, [0]), ([NA_integer], None), (None, [1, 32])):
            with pytest.raises(SparseArrayError, match="out of bounds|NAs"):
                call.C_subset_SVT_by_Nindex(x, None if i is None else np.asarray(i, np.int32),
                                            None if j is None else np.asarray(j, np.int32))
        assert hip.resident_stats() == before
        sc.check(call.C_subset_SVT_by_Nindex(x, *[None if v is None else np.asarray(v, np.int32)
                                                  for v in sc.BY_NAME["integer_both"][2:]]), "integer_both")
        assert hip.resident_stats()["misses"] == before["misses"] + 1
    finally:
        hip.resident_set_limit(0)
        hip.resident_clear()


# ---------------------------------------------------------------------------
# device level: operands around the tile
# ---------------------------------------------------------------------------
def _T():
    from sparsearray_amd.device import subset_tile
    return subset_tile()


def _layouts(T):
    """name -> column lengths"""
    return {
        "nnz_0": [0] * 5,
        "nnz_1": [0, 1, 0],
        "nnz_T_minus_1": [T // 2, 0, T // 2 - 1],
        "nnz_T": [T // 2, T // 2],
        "nnz_T_plus_1": [T, 1],                                       # a column boundary exactly on the tile boundary
        "nnz_2T_plus_1": [T - 7, 0, T + 8],
        "boundary_on_tile_boundary": [T, 5, T - 5, 3],                # at T and at 2 T
        "one_column_spans_three_tiles": [100, 2 * T + 200, 50],
        "empty_run_at_tile_boundary": [T] + [0] * 100 + [10],         # 100 empty columns all start at T ...
        "empty_run_inside_a_tile": [T - 3] + [0] * 100 + [10, 0, 0],  # ... and at T - 3, the last columns empty too
        "last_column_empty": [17, T, 0],
        "one_column_over_90_percent": [50, 2 * T + 3 * T // 4, 50, 0, 60],
        # more column boundaries in a tile than the workgroup has threads: the one-lane-per-boundary loops take
        # several trips (about 2700 boundaries in a full tile, 680 in the last one) ...
        "many_short_columns": [0, 1, 2, 3] * (3 * T // 8),
        # ... and so does a run of empty columns that all start at the same entry inside a tile
        "empty_run_longer_than_the_workgroup": [T - 3] + [0] * 600 + [10],
    }


def _nrow(T, name):
    """3 T rows; fewer where the dense tracer matrix of the reference would be large for nothing"""
    return {"many_short_columns": 64, "empty_run_longer_than_the_workgroup": T + 50}.get(name, NROW_TILES * T)


NAMES = list(_layouts(4096))
NROW_TILES = 3
WORKGROUP = 256          # SUB_NT of kernels_subset.hip: the stride of the loops over the column boundaries of a tile


@pytest.fixture(scope="module")
def tile(hip):
    return _T()


_cache = {}


def _operand(T, name):
    """(nrow, col_ptr, row_idx, val, tracer dense) of the layout; the values are the double specials cycled"""
    key = (T, name)
    if key not in _cache:
        lens = _layouts(T)[name]
        nrow = _nrow(T, name)
        rng = np.random.default_rng(len(name))
        cp = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=cp[1:])
        ri = np.concatenate([np.sort(rng.choice(nrow, size=n, replace=False)) for n in lens] +
                            [np.zeros(0, np.int64)]).astype(np.int32)
        val = sc.SPECIALS_F64[np.arange(ri.size) % len(sc.SPECIALS_F64)]
        tracer = np.zeros((nrow, len(lens)), dtype=np.int64, order="F")
        tracer[ri, np.repeat(np.arange(len(lens)), lens)] = np.arange(ri.size) + 1
        for a in (cp, ri, val, tracer):
            a.setflags(write=False)
        if name == "one_column_over_90_percent":
            assert max(lens) > 0.9 * sum(lens)
        if name == "many_short_columns":                                # column starts per tile
            starts = np.bincount(cp[:-1] // T, minlength=-(-int(cp[-1]) // T))
            assert len(lens) == 3 * T // 2 and starts[:-1].min() >= 1000 and starts.min() > 2 * WORKGROUP
        if name == "empty_run_longer_than_the_workgroup":
            assert (cp == T - 3).sum() > 2 * WORKGROUP and cp[-1] > T
        _cache[key] = (nrow, cp, ri, val, tracer)
    return _cache[key]


def _reference(tracer, val, rows0, cols0):
    """(col_ptr, row_idx, val) of x[rows0, cols0] by np.ix_ on the dense tracer matrix"""
    r = np.arange(tracer.shape[0]) if rows0 is None else np.asarray(rows0, dtype=np.int64)
    c = np.arange(tracer.shape[1]) if cols0 is None else np.asarray(cols0, dtype=np.int64)
    sub = np.asfortranarray(tracer[np.ix_(r, c)])
    flat = sub.reshape(-1, order="F")
    at = np.flatnonzero(flat)
    cp = np.zeros(c.size + 1, dtype=np.int64)
    if r.size:
        np.cumsum(np.bincount(at // r.size, minlength=c.size), out=cp[1:])
    return cp, (at % max(r.size, 1)).astype(np.int32), val[flat[at] - 1]


def _device(nrow, cp, ri, val):
    from sparsearray_amd.device import DeviceCSC
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val), device="cuda"))


def _host(R):
    torch.cuda.synchronize()
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    assert got[2].dtype == want[2].dtype and np.array_equal(sc.bits(got[2]), sc.bits(want[2])), f"{what}: val as bits"


def _increasing_half(n, seed):
    return np.flatnonzero(np.random.default_rng(seed).random(n) < 0.5).astype(np.int32)


def _gather_cols(ncol, seed):
    """every column in reverse, then repeats: longer than the axis"""
    extra = np.random.default_rng(seed).integers(0, ncol, size=ncol // 2 + 2)
    return np.concatenate([np.arange(ncol)[::-1], extra, extra[:1]]).astype(np.int32)


@pytest.mark.parametrize("name", NAMES)
def test_row_filter_around_the_tile(tile, name):
    from sparsearray_amd.device import subset_route_counts, subset_rows
    nrow, cp, ri, val, tracer = _operand(tile, name)
    A = _device(nrow, cp, ri, val)
    for rows in (_increasing_half(nrow, 1), np.arange(nrow, dtype=np.int32), np.zeros(0, np.int32),
                 np.array([nrow - 1], dtype=np.int32)):
        subset_route_counts(reset=True)
        R = subset_rows(A, rows)
        assert R.nrow == rows.size and R.ncol == A.ncol
        _same(_host(R), _reference(tracer, val, rows, None), f"{name}, {rows.size} rows")
        assert subset_route_counts() == {"column_gather": 0, "row_filter": 1, "general_rows": 0}


@pytest.mark.parametrize("name", NAMES)
def test_column_gather_around_the_tile(tile, name):
    from sparsearray_amd.device import subset_cols, subset_route_counts
    nrow, cp, ri, val, tracer = _operand(tile, name)
    A = _device(nrow, cp, ri, val)
    ncol = cp.size - 1
    for cols in (_gather_cols(ncol, 2), np.arange(ncol, dtype=np.int32), np.zeros(0, np.int32)):
        assert cols.size > ncol or cols.size in (0, ncol)
        subset_route_counts(reset=True)
        R = subset_cols(A, cols)
        assert R.nrow == nrow and R.ncol == cols.size
        _same(_host(R), _reference(tracer, val, None, cols), f"{name}, {cols.size} columns")
        assert subset_route_counts() == {"column_gather": 1, "row_filter": 0, "general_rows": 0}


def test_routes(tile):
    from sparsearray_amd.device import subset_cols, subset_route_counts
    name = "one_column_spans_three_tiles"
    nrow, cp, ri, val, tracer = _operand(tile, name)
    A = _device(nrow, cp, ri, val)
    rng = np.random.default_rng(3)
    inc = _increasing_half(nrow, 4)
    perm = rng.permutation(nrow).astype(np.int32)
    rep = rng.integers(0, nrow, size=nrow // 3).astype(np.int32)
    for rows, route in ((inc, {"column_gather": 0, "row_filter": 1, "general_rows": 0}),
                        (perm, {"column_gather": 1, "row_filter": 0, "general_rows": 1}),
                        (rep, {"column_gather": 1, "row_filter": 0, "general_rows": 1})):
        subset_route_counts(reset=True)
        R = A.subset(rows=rows)
        _same(_host(R), _reference(tracer, val, rows, None), f"{name}, rows {route}")
        assert subset_route_counts() == route
    # columns and rows in one call: the gather first, then the filter / the composition
    cols = _gather_cols(3, 5)
    for rows, route in ((inc, {"column_gather": 1, "row_filter": 1, "general_rows": 0}),
                        (rep, {"column_gather": 2, "row_filter": 0, "general_rows": 1})):
        subset_route_counts(reset=True)
        _same(_host(A.subset(rows=rows, cols=cols)), _reference(tracer, val, rows, cols), f"{name}, both")
        assert subset_route_counts() == route
    _same(_host(A.subset()), (cp, ri, val), "x[, ]")
    # the increasing subscript through the composition on purpose: t, gather, t -- the filter's arrays
    via = subset_cols(A.t(), inc).t()
    _same(_host(via), _host(A.subset(rows=inc)), "composition vs filter")


def test_gather_of_more_tiles_than_its_grid(tile):
    """The gather runs on a fixed grid and strides over the tiles of its result: a column of 3 T nonzeros gathered 700
    times, an empty column and one of 5 entries after each, gives 2101 result tiles -- every workgroup takes a first
    trip and the first ones a second.  The expectation is the three columns tiled with numpy (about 8.6 M entries)."""
    from sparsearray_amd.device import subset_cols, subset_route_counts
    GRID = 2048                          # SUB_GATHER_GRID of kernels_subset.hip
    T, reps = tile, 700
    nrow = 3 * T + 40
    rng = np.random.default_rng(12)
    lens = np.array([3 * T, 0, 5])
    cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ri = np.concatenate([np.sort(rng.choice(nrow, size=n, replace=False)) for n in lens]).astype(np.int32)
    val = sc.SPECIALS_F64[np.arange(ri.size) % len(sc.SPECIALS_F64)]
    val[::5] = np.arange(1, ri.size + 1, dtype=np.float64)[::5]        # tracers among them: which entry landed where
    cols = np.tile(np.array([0, 1, 2], dtype=np.int32), reps)
    want_cp = np.concatenate([[0], np.cumsum(np.tile(lens, reps))]).astype(np.int64)
    ntiles = -(-int(want_cp[-1]) // T)
    # more tiles than the grid has workgroups, and still so with the grid halved
    assert ntiles > GRID and ntiles > 2 * (GRID // 2) and want_cp[-1] == reps * (3 * T + 5)
    A = _device(nrow, cp, ri, val)
    subset_route_counts(reset=True)
    R = subset_cols(A, cols)
    got = _host(R)
    assert subset_route_counts() == {"column_gather": 1, "row_filter": 0, "general_rows": 0}
    assert R.nrow == nrow and R.ncol == cols.size
    _same(got, (want_cp, np.tile(ri, reps), np.tile(val, reps)), "2101 tiles")


@pytest.mark.parametrize("dtype", ["integer", "logical"])
def test_integer_and_logical_values(tile, dtype):
    from sparsearray_amd.device import DeviceCSC
    from sparsearray_amd.svt import INTSXP, LGLSXP
    nrow, cp, ri, _, tracer = _operand(tile, "nnz_2T_plus_1")
    table = sc.SPECIALS_I32 if dtype == "integer" else sc.SPECIALS_LGL
    val = table[np.arange(ri.size) % len(table)]
    A = DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                  torch.as_tensor(val, device="cuda"), logical=dtype == "logical")
    rows, cols = np.random.default_rng(6).permutation(nrow).astype(np.int32), np.array([2, 2, 0, 1], dtype=np.int32)
    for r in (rows, np.sort(rows[:nrow // 2])):
        R = A.subset(rows=r, cols=cols)
        assert R.Rtype == (INTSXP if dtype == "integer" else LGLSXP)
        _same(_host(R), _reference(tracer, val, r, cols), dtype)


def test_bits_survive_every_route(tile):
    nrow, cp, ri, val, tracer = _operand(tile, "boundary_on_tile_boundary")
    A = _device(nrow, cp, ri, val)
    have = set(sc.bits(val).tolist())
    assert have == set(sc.bits(sc.SPECIALS_F64).tolist())       # NA_real_, two other NaNs, +-Inf, -0.0, 0.0
    rng = np.random.default_rng(7)
    for rows, cols in ((None, np.array([3, 0, 0, 2, 1], np.int32)), (np.arange(0, nrow, 2, dtype=np.int32), None),
                       (rng.permutation(nrow).astype(np.int32), None)):
        got = _host(A.subset(rows=rows, cols=cols))
        want = _reference(tracer, val, rows, cols)
        _same(got, want, "specials")
        assert got[2].view(np.uint64).tolist() == want[2].view(np.uint64).tolist()
        assert set(got[2].view(np.uint64).tolist()) == have


def test_same_call_twice_gives_the_same_arrays(tile):
    nrow, cp, ri, val, _ = _operand(tile, "one_column_over_90_percent")
    A = _device(nrow, cp, ri, val)
    rows = np.random.default_rng(8).integers(0, nrow, size=nrow).astype(np.int32)
    for kw in (dict(rows=rows), dict(rows=np.unique(rows)), dict(cols=_gather_cols(5, 9))):
        _same(_host(A.subset(**kw)), _host(A.subset(**kw)), f"twice {list(kw)}")


# ---------------------------------------------------------------------------
# errors and workspace discipline: the entry points called with the test's own buffers
# ---------------------------------------------------------------------------
class Raw:
    """One primitive with caller-made buffers: ws of the advertised size followed by a guard band, out_col_ptr
    pre-filled; count() returns (status, out_nnz)."""

    def __init__(self, A, idx, rows, short=0):
        from sparsearray_amd.device import _lib, _stream
        self.lib, self.stream, self.A, self.rows = _lib(), _stream, A, rows
        self.idx = torch.as_tensor(np.asarray(idx, dtype=np.int32), device="cuda")
        self.nb = (self.lib.svt_dev_subset_rows_ws_bytes(A.nrow, A.ncol, A.nnz) if rows else
                   self.lib.svt_dev_subset_cols_ws_bytes(self.idx.numel()))
        self.ws = torch.full((self.nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.cp = torch.full(((A.ncol if rows else self.idx.numel()) + 1,), -77, dtype=torch.int64, device="cuda")
        self.short = short
        self.nnz = ctypes.c_int64(-5)

    def count(self):
        f = self.lib.svt_dev_subset_rows_count if self.rows else self.lib.svt_dev_subset_cols_count
        rc = f(self.A.handle, self.idx.data_ptr(), self.idx.numel(), self.cp.data_ptr(), ctypes.byref(self.nnz),
               self.ws.data_ptr(), self.nb - self.short, self.stream())
        torch.cuda.synchronize()
        return rc, self.nnz.value

    def fill(self, short=0):
        self.ri = torch.full((max(self.nnz.value, 1),), -77, dtype=torch.int32, device="cuda")
        self.vv = torch.zeros(max(self.nnz.value, 1), dtype=self.A.val.dtype, device="cuda")
        if self.rows:
            rc = self.lib.svt_dev_subset_rows_fill(self.A.handle, self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(),
                                                   self.ws.data_ptr(), self.nb - short, self.stream())
        else:
            rc = self.lib.svt_dev_subset_cols_fill(self.A.handle, self.idx.data_ptr(), self.idx.numel(), self.cp.data_ptr(),
                                                   self.ri.data_ptr(), self.vv.data_ptr(), self.stream())
        torch.cuda.synchronize()
        return rc

    def guard_intact(self):
        return bool((self.ws[self.nb:] == 0xA5).all())

    def outputs_untouched(self):
        return bool((self.cp == -77).all()) and self.nnz.value == -5

    def arrays(self):
        n = self.nnz.value
        return self.cp.cpu().numpy(), self.ri[:n].cpu().numpy(), self.vv[:n].cpu().numpy()


@pytest.mark.parametrize("name", ["nnz_0", "nnz_2T_plus_1", "one_column_spans_three_tiles", "empty_run_at_tile_boundary"])
def test_calls_stay_inside_the_advertised_workspace(tile, name):
    nrow, cp, ri, val, tracer = _operand(tile, name)
    A = _device(nrow, cp, ri, val)
    for rows, idx in ((True, _increasing_half(nrow, 10)), (False, _gather_cols(cp.size - 1, 11))):
        r = Raw(A, idx, rows)
        assert r.count()[0] == 0 and r.guard_intact()
        assert r.fill() == 0 and r.guard_intact()
        _same(r.arrays(), _reference(tracer, val, idx if rows else None, None if rows else idx), f"{name} raw")


def test_bad_arguments_are_refused_before_any_index_is_used(tile):
    nrow, cp, ri, val, tracer = _operand(tile, "nnz_2T_plus_1")
    A = _device(nrow, cp, ri, val)
    ncol = cp.size - 1
    lib = Raw(A, [0], False).lib
    # an index outside [0, extent): < 0, the outputs as they were
    for rows, idx in ((False, [0, ncol, 1]), (False, [1, -1]), (False, [2 ** 31 - 1]), (False, [-2 ** 31]),
                      (True, [0, 5, nrow]), (True, [-1, 3]), (True, [5, 3, nrow + 7]), (True, [-2 ** 31, 2 ** 31 - 1])):
        r = Raw(A, idx, rows)
        rc, _ = r.count()
        assert rc < 0 and b"out of bounds" in lib.svt_last_error(), (rows, idx)
        assert r.outputs_untouched() and r.guard_intact()
    # rows in range but not strictly increasing: > 0, nothing written
    for idx in ([5, 3], [4, 4], [0, 1, 2, 2], list(range(nrow)) + [0]):
        r = Raw(A, idx, True)
        assert r.count()[0] > 0 and b"strictly increasing" in lib.svt_last_error()
        assert r.outputs_untouched() and r.guard_intact()
    # a workspace one byte short: < 0 from both count calls and from the filter's fill
    for rows, idx in ((True, [1, 2]), (False, [1, 1])):
        r = Raw(A, idx, rows, short=1)
        assert r.count()[0] < 0 and b"workspace too small" in lib.svt_last_error()
        assert r.outputs_untouched() and bool((r.ws == 0xA5).all())
    r = Raw(A, [1, 2], True)
    assert r.count()[0] == 0
    assert r.fill(short=1) < 0 and b"workspace too small" in lib.svt_last_error()
    # the stream is sound after all of it: the same buffers' next calls succeed and give the rule's answer
    for rows, idx in ((True, [1, 2, nrow - 1]), (False, [2, 0, 0])):
        r = Raw(A, idx, rows)
        assert r.count()[0] == 0 and r.fill() == 0
        _same(r.arrays(), _reference(tracer, val, idx if rows else None, None if rows else idx), "after the errors")


def test_python_level_errors(tile):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported
    from sparsearray_amd.device import subset_rows
    nrow, cp, ri, val, tracer = _operand(tile, "nnz_T_plus_1")
    A = _device(nrow, cp, ri, val)
    for kw in (dict(rows=[nrow]), dict(cols=[2]), dict(rows=[0, 1], cols=[-1]), dict(rows=[3, 1, nrow])):
        with pytest.raises(SparseArrayError, match="out of bounds"):
            A.subset(**kw)
    with pytest.raises(SparseArrayUnsupported, match="strictly increasing"):
        subset_rows(A, [3, 1])
    _same(_host(A.subset(rows=[3, 1])), _reference(tracer, val, [3, 1], None), "after the errors")
