"""The cases of the statistics accuracy tests (test_stats_accuracy_cpu.py, test_hip_stats_accuracy.py): skewed column
lengths for every launch form of the column statistics, one shape per route of the row statistics, the value palettes,
and the runners that push a case through a session and hold every result against exact_stats.

A case is built once (``column_case`` / ``row_case`` are cached) together with its exact moments; the sessions only
differ in who computes ``got``.
"""
from __future__ import annotations

import functools
import warnings

import numpy as np

import exact_stats as ex
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd._hip import colstats_form, rowstats_form

INT_MAX = 2 ** 31 - 1
DBL_MAX = np.finfo(np.float64).max

# ---------------------------------------------------------------------------
# skewed column lengths: one case per form of launch_colstats (kernels_colstats.hip, colstats_route).  The form
# follows from the AVERAGE length; the lengths sit on both sides of what the form's kernel keeps in registers
# (NT * CAP = 256 / 1024 / 12288), next to an empty column and to one many times the average.
# ---------------------------------------------------------------------------
COLUMN_FORMS = {
    # avg < 160 (and not: avg < 4 with >= 4096 columns)
    "lanes16": dict(nrow=5000, lengths=[0, 1, 15, 16, 17, 255, 256, 257, 300, 4000], fill=(590, 30, 50)),
    # 160 <= avg < 1024
    "wavefront": dict(nrow=6000, lengths=[0, 63, 64, 65, 1023, 1024, 1025, 5000], fill=(56, 380, 420)),
    # 1024 <= avg <= 10240
    "workgroup_cached": dict(nrow=20000, lengths=[0, 255, 256, 257, 12287, 12288, 12289, 20000], fill=(16, 1900, 2100)),
    # avg > 10240, and not split: avg < 65536
    "workgroup_streaming": dict(nrow=30000, lengths=[30000, 0, 12289, 100, 12288, 12000], fill=(0, 0, 0)),
    # avg < 4, >= 4096 columns
    "thread": dict(nrow=2500, lengths=[2000], fill=(4999, 0, 3)),
    # fewer than 512 columns, avg >= 65536: nchunk = min(ceil(1024 / nseg), avg / 16384) = 4
    "split": dict(nrow=200000, lengths=[200000, 65, 0], fill=(0, 0, 0)),
    # the same with two leaves per column, and a column shorter than its 4 chunks
    "split_inner2": dict(nrow=100000, inner=2, lengths=[200000, 0, 65, 200000, 3], fill=(0, 0, 0), form="split"),
    # a generalized column spans two leaves (3-d operand, dims = 2)
    "wavefront_inner2": dict(nrow=3000, inner=2, lengths=[0, 63, 64, 65, 1023, 1024, 1025, 5000], fill=(56, 380, 420),
                             form="wavefront"),
    # NaArray background: the implicit elements are NAs
    "lanes16_nabg": dict(nrow=5000, lengths=[0, 1, 15, 16, 17, 255, 256, 257, 300, 4000, 5000], fill=(590, 30, 50),
                         form="lanes16", na_bg=True),
}

# which palettes each column case runs ("a" carries the planted NA / NaN)
COLUMN_PALETTES = {
    "lanes16": ["a", "c_up", "c_down", "d", "e", "i", "f"],
    "wavefront": ["a", "c_up", "c_down", "d", "e", "i", "f"],
    "workgroup_cached": ["a", "c_down", "d", "i"],
    "workgroup_streaming": ["a", "c_up", "d", "i"],
    "thread": ["a", "d", "e", "i", "f"],
    "split": ["a", "d", "i"],
    "split_inner2": ["a", "i"],
    "wavefront_inner2": ["a", "d", "i"],
    "lanes16_nabg": ["a", "i"],
}


def palette_values(palette, n, rng):
    """(values, scale): ``scale`` is a power of two that says where the magnitudes sit (centres are scaled by it)."""
    if palette in ("a", "c_up", "c_down", "e"):
        v = rng.standard_normal(n)                         # full 53-bit mantissas
        v[v == 0] = 1.0
        scale = {"c_up": 2.0 ** 400, "c_down": 2.0 ** -400}.get(palette, 1.0)
        v = v * scale                                       # exact: a power of two, squares stay in range
        if palette == "e" and n:
            ext = np.array([DBL_MAX, -DBL_MAX, 5e-324, -5e-324, np.inf, -np.inf])
            hit = rng.choice(n, size=min(n, max(6, n // 50)), replace=False)
            v[hit] = ext[np.arange(len(hit)) % 6]
        return v, scale
    if palette == "d":                                      # m * 2**e, e uniform in [-60, 60], mixed signs
        m = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
        return np.ldexp(m, rng.integers(-60, 61, n)), 1.0
    if palette == "i":
        v = rng.integers(1, 10, n) * rng.choice([-1, 1], n)
        return v.astype(np.int32), 1.0
    if palette == "f":                                      # the ends of int32
        pool = np.array([INT_MAX, -INT_MAX, 2 ** 30, -(2 ** 30), 7, -3], dtype=np.int64)
        return pool[rng.integers(0, len(pool), n)].astype(np.int32), 1.0
    if palette == "b_col":                                  # offset, ill-conditioned for a one-pass variance
        return 1e8 + rng.standard_normal(n), 1.0
    if palette == "b_row":
        return 1e3 + rng.standard_normal(n), 1.0
    if palette == "g":                                      # products that stay near 1 in any order
        return rng.choice([-1.0, 1.0], n) * (1.0 + rng.uniform(-2.0 ** -10, 2.0 ** -10, n)), 1.0
    if palette == "overflow":                               # every partial sum of two or more is +Inf
        return np.ldexp(rng.uniform(0.5, 1.0, n), 1024), 1.0
    raise KeyError(palette)


def build_segments(nrow, inner, lengths, rng):
    """CSC arrays of len(lengths) * inner leaves: segment g holds lengths[g] nonzeros at random places of its
    inner * nrow elements."""
    L = inner * nrow
    cp = np.zeros(len(lengths) * inner + 1, dtype=np.int64)
    rows = []
    for g, n in enumerate(lengths):
        pos = np.sort(rng.permutation(L)[:n]) if n else np.zeros(0, dtype=np.int64)
        rows.append((pos % nrow).astype(np.int32))
        cp[g * inner + 1:(g + 1) * inner + 1] = np.bincount(pos // nrow, minlength=inner)
    return np.cumsum(cp), np.concatenate(rows) if rows else np.zeros(0, np.int32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def column_layout(name):
    """The lengths and the offsets of a column form's case (shared by its palettes)."""
    spec = COLUMN_FORMS[name]
    rng = np.random.default_rng(sorted(COLUMN_FORMS).index(name) + 1000)
    nfill, lo, hi = spec["fill"]
    lengths = list(spec["lengths"]) + list(rng.integers(lo, hi + 1, nfill))
    lengths = [int(lengths[i]) for i in rng.permutation(len(lengths))]
    inner, nrow = spec.get("inner", 1), spec["nrow"]
    cp, ri = build_segments(nrow, inner, lengths, rng)
    return spec, lengths, cp, ri


@functools.lru_cache(maxsize=None)
def column_case(name, palette):
    spec, lengths, cp, ri = column_layout(name)
    c = Case()
    c.name, c.palette = name, palette
    c.form = spec.get("form", name)
    c.nrow, c.inner, c.na_bg = spec["nrow"], spec.get("inner", 1), spec.get("na_bg", False)
    c.nseg, c.lengths = len(lengths), np.asarray(lengths)
    c.col_ptr, c.row_idx = cp, ri
    rng = np.random.default_rng(sum(map(ord, name + palette)))
    val, c.scale = palette_values(palette, len(ri), rng)
    c.type = "double" if val.dtype == np.float64 else "integer"
    c.planted = palette in ("a", "i")
    if c.planted and not (c.na_bg and c.type == "integer"):
        # a missing value in a column the kernel keeps in registers and in one it reads twice (or streams): the
        # longest column gets an NA and (doubles) a NaN, the shortest of at least two values an NA, one in between a NaN.
        # (The leaves of an NaArray hold no NA, src/Rvector_utils.c:586-596: a NaN there, nothing in an integer one.)
        seg_beg = cp[::c.inner][:-1]
        order = np.argsort(c.lengths, kind="stable")
        longest, shortest = order[-1], order[np.searchsorted(c.lengths[order], 2)]
        middle = order[len(order) // 2]
        na, nan = (NA_real, np.nan) if c.type == "double" else (NA_integer, NA_integer)
        if c.na_bg:
            na = np.nan
        val[seg_beg[longest] + c.lengths[longest] // 3] = na
        val[seg_beg[longest] + c.lengths[longest] - 1] = nan
        val[seg_beg[shortest]] = na
        if c.lengths[middle] > 0:
            val[seg_beg[middle] + c.lengths[middle] // 2] = nan
    c.val = val
    c.center = 0.37 * c.scale
    nleaf = len(cp) - 1
    dim = (c.nrow, nleaf) if c.inner == 1 else (c.nrow, c.inner, nleaf // c.inner)
    x = SVT_SparseArray.from_csc((c.nrow, nleaf), c.type, cp, ri, val)
    c.x = SVT_SparseArray(dim, c.type, x.leaves, na_background=c.na_bg)
    c.dims = 1 if c.inner == 1 else 2
    c.cells = {na_rm: ex.column_cells(cp, val, c.nrow, c.inner, na_rm, c.na_bg) for na_rm in (False, True)}
    c.whole = {na_rm: ex.Cells(val, np.zeros(len(val), np.int64), 1, c.nrow * nleaf, na_rm, c.na_bg)
               for na_rm in (False, True)}
    return c


def assert_column_form(c):
    """The case still takes the launch form it is named after, and holds columns on both sides of the kernel's own
    register limit wherever the form has one."""
    form, nchunk = colstats_form(c.nseg, len(c.val))
    assert form == c.form, f"{c.name}: takes the form {form}, not {c.form}"
    assert (c.lengths == 0).any(), f"{c.name}: no empty column"
    cap = {"lanes16": 256, "wavefront": 1024, "workgroup_cached": 12288}.get(form)
    if cap is not None and c.inner == 1:
        for n in (cap - 1, cap, cap + 1):
            assert (c.lengths == n).any(), f"{c.name}: no column of {n}"
    if form == "split":
        assert nchunk == 4
        assert ((c.lengths > 0) & (c.lengths < nchunk)).any() or c.name == "split"
    # the whole array as one segment (summaries)
    return form


COL_OPS = ["sum", "mean", "var1", "sd1", "centered_X2_sum", "min", "max", "prod", "anyNA", "countNAs"]


def _quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            return f(*a, **k)


NO_VALUE = "NAs introduced by coercion of infinite values to integers"


def _warned(f, *a, **k):
    """(f's result, whether it gave the integer "no value" warning); every other warning stays quiet."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with np.errstate(all="ignore"):
            res = f(*a, **k)
    return res, any(NO_VALUE in str(m.message) for m in w)


def _flat(a):
    return np.asarray(a).reshape(-1, order="F")


def _note(rec, key, verdict):
    verdict.require()
    if rec is not None:
        rec[key] = max(rec.get(key, 0.0), verdict.worst)


def check_stat(op, got, cells, rec, key, center=None, rows=False, is_int=False, dgc=False, what=""):
    """One statistic of every cell against its rule: a rounding bound or identity (see exact_stats)."""
    got = _flat(got)
    what = f"{what} {op}"
    if op == "sum":
        if is_int:      # integer sums below 2**53: every order gives the exact sum
            ok = ~cells.poisoned
            assert np.all(np.isnan(got[cells.poisoned].astype(np.float64))), what
            S = cells.S[ok]
            assert all(abs(int(v)) >> -S.exp < 2 ** 53 for v in S.num)
            want = np.ldexp(S.num.astype(np.float64), S.exp)            # exact: the sums have fewer than 53 bits
            assert np.array_equal(got[ok].astype(np.float64), want), f"{what}: integer sums differ"
        else:
            _note(rec, key, ex.check_sum(got, cells, what))
    elif op == "mean":
        _note(rec, key, ex.check_mean(got, cells, what))
    elif op == "prod":
        _note(rec, key, ex.check_prod(got, cells, what))
    elif op in ("var1", "sd1", "centered_X2_sum"):
        f = ex.check_row_centered if rows else ex.check_col_centered
        kw = {} if rows else {"dgc": dgc}
        _note(rec, key, f(got, cells, center=center, op=op, what=what, **kw))
    elif op in ("min", "max"):
        ex.check_identical(got, ex.exact_minmax(cells, op == "min", as_int=is_int), what)
    elif op == "countNAs":
        ex.check_identical(got.astype(np.float64), ex.exact_count_nas(cells), what)
    elif op == "anyNA":
        assert np.array_equal(got != 0, ex.exact_count_nas(cells) > 0), what
    elif op in ("any", "all"):
        ex.check_identical(got, ex.exact_any_all(cells, op == "any"), what)
    else:
        raise KeyError(op)


def run_column_case(sess, c, rec=None, who="", colstat=None):
    """Every column statistic of the case, both na_rm, through ``sess`` (col*() of a Session), or through
    ``colstat(op, na_rm, center) -> (result, warn word set)`` when given (the device level).  Integer min / max also
    say that a cell had no value: the session by a warning, the device by its warn word, both exactly when
    exact_stats.exact_int_no_value() says so."""
    is_int = c.type == "integer"
    ops = COL_OPS + (["any", "all"] if is_int else [])
    if c.palette == "e":
        ops = ["min", "max", "anyNA", "countNAs"]            # +-Inf among the values: only these are pinned
    if c.palette in ("c_up", "c_down"):
        ops = [op for op in ops if op != "prod"]             # partial products leave the range: order decides
    for na_rm in ((False, True) if c.planted else (False,)):
        cells = c.cells[na_rm]
        for op in ops:
            center = c.center if op == "centered_X2_sum" else None
            narm = na_rm and op not in ("anyNA", "countNAs")     # (colAnyNAs / colCountNAs have no na.rm)
            if colstat is not None:
                got, warned = colstat(op, narm, center)
            else:
                got, warned = _warned(sess._colStats, op, c.x, narm, center, c.dims)
            if is_int and op in ("min", "max"):
                assert warned == ex.exact_int_no_value(cells), f"{c.name}/{c.palette} na_rm={na_rm} {op}: warning"
            check_stat(op, got, cells, rec, (who, "col " + op, c.form), center=center, is_int=is_int,
                       what=f"{c.name}/{c.palette} na_rm={na_rm}")


SUMMARY_OPS = ["sum", "mean", "var", "sd", "min", "max", "range", "anyNA", "countNAs"]


def run_summary_case(sess, c, rec=None, who=""):
    """The whole-array summaries of a column case: one cell holding every element."""
    is_int = c.type == "integer"
    form, _ = colstats_form(1, len(c.val))
    for na_rm in ((False, True) if c.planted else (False,)):
        cells = c.whole[na_rm]
        for op in SUMMARY_OPS + (["any", "all"] if is_int else []):
            if c.palette == "e" and op in ("sum", "mean", "var", "sd"):
                continue
            kw = {} if op in ("anyNA", "countNAs") else {"na_rm": na_rm}
            got = np.asarray(_quiet(getattr(sess, op), c.x, **kw))
            if is_int and op == "sum" and got.dtype == np.int32:     # naked_result(): an int, NA_integer for NA
                got = np.where(got == NA_integer, np.nan, got.astype(np.float64))
            key = (who, "summary " + op, form)
            what = f"{c.name}/{c.palette} summary na_rm={na_rm}"
            if op == "range":
                check_stat("min", got[:1], cells, rec, key, is_int=is_int, what=what)
                check_stat("max", got[1:], cells, rec, key, is_int=is_int, what=what)
            else:
                check_stat({"var": "var1", "sd": "sd1"}.get(op, op), got.reshape(1), cells, rec, key, is_int=is_int, what=what)


def run_dgc_case(sess, c, rec=None, who=""):
    """colMins / colMaxs / colRanges / colVars of the same arrays as a dgCMatrix (2-d doubles without missing values:
    col_var() of src/sparseMatrix_utils.c:173-223 has no NA rule to compare)."""
    assert c.inner == 1 and c.type == "double" and not c.planted
    x = ((c.nrow, c.nseg), c.col_ptr.astype(np.int32), c.row_idx, c.val)
    cells = c.cells[False]
    what = f"{c.name}/{c.palette} dgCMatrix"
    check_stat("min", _quiet(sess.colMins_dgCMatrix, x), cells, rec, None, what=what)
    check_stat("max", _quiet(sess.colMaxs_dgCMatrix, x), cells, rec, None, what=what)
    rng = np.asarray(_quiet(sess.colRanges_dgCMatrix, x))
    check_stat("min", rng.reshape(-1, order="F")[:c.nseg], cells, rec, None, what=what + " range")
    check_stat("max", rng.reshape(-1, order="F")[c.nseg:], cells, rec, None, what=what + " range")
    check_stat("var1", _quiet(sess.colVars_dgCMatrix, x), cells, rec, (who, "dgCMatrix var1", c.form), dgc=True, what=what)


# ---------------------------------------------------------------------------
# offset and product palettes on full columns
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_case(nrow, palette):
    """(nrow, 8) with every element stored."""
    rng = np.random.default_rng(nrow + sum(map(ord, palette)))
    c = Case()
    c.name, c.palette, c.nrow, c.inner, c.na_bg, c.nseg = f"full{nrow}", palette, nrow, 1, False, 8
    c.col_ptr = np.arange(9, dtype=np.int64) * nrow
    c.row_idx = np.tile(np.arange(nrow, dtype=np.int32), 8)
    c.val, c.scale = palette_values(palette, 8 * nrow, rng)
    c.type, c.planted, c.dims = "double", False, 1
    c.lengths = np.full(8, nrow)
    c.form, _ = colstats_form(8, 8 * nrow)
    c.center = float(np.mean(c.val)) if palette.startswith("b") else 0.37
    c.x = SVT_SparseArray.from_csc((nrow, 8), "double", c.col_ptr, c.row_idx, c.val)
    c.cells = {False: ex.column_cells(c.col_ptr, c.val, nrow)}
    c.rows = {False: ex.row_cells(c.col_ptr, c.row_idx, c.val, nrow)}
    return c


# ---------------------------------------------------------------------------
# row routes: one shape per form of rowstats_route (kernels_rowstats.hip)
# ---------------------------------------------------------------------------
ROW_OPS = ["sum", "centered_X2_sum", "centered_X2_sum+center", "min", "max", "countNAs",
           "mean", "var1", "sd1", "range", "prod"]
ROW_ROUTES = {
    # 2048-row panels, the last one ragged (2500 = 2048 + 452)
    "panel_short": dict(dim=(2500, 40), dims=1, nnz=12000, forms={"sum": ("panel", 11, 1), "min": ("panel", 11, 1)}),
    # 8192-row panels whose strata are cut into ranges added to a zeroed result (nsplit > 1); min / max keep 2048
    "panel_strata": dict(dim=(16500, 600), dims=1, nnz=99000,
                         forms={"sum": ("panel", 13, 9), "centered_X2_sum": ("panel", 13, 9), "min": ("panel", 11, 1)}),
    # all rows of an output column in LDS: centred sums take the whole-column kernel, sums its pipelined form
    "whole_column": dict(dim=(8500, 1030, 3), dims=2, nnz=60000,
                         forms={"sum": ("pipe", 0, 1), "countNAs": ("pipe", 0, 1),
                                "centered_X2_sum": ("whole_column", 0, 1), "min": ("panel", 11, 1)}),
    # the pipelined kernel over (column, chunk of 64 leaves) units: 65 strata make 2 chunks, inner * 2 >= 2048, leaves
    # of at least 8 nonzeros on average, more than 8192 rows
    "pipe_units": dict(dim=(8200, 1024, 65), dims=2, nnz=600000, ops=["sum", "countNAs", "mean"],
                       forms={"sum": ("pipe_units", 0, 1), "countNAs": ("pipe_units", 0, 1)}),
    # more than 65535 output columns: memory atomics (nine leaves in ten empty: the host entry points walk the leaves
    # of their argument one by one, and the route does not depend on how many hold something)
    "memory_atomics": dict(dim=(8, 70000, 3), dims=2, nnz=400000, empty=0.9,
                           ops=[op for op in ROW_OPS if op != "prod"],     # (composed from aperm() there)
                           forms={op: ("memory_atomics", 0, 1) for op in ("sum", "centered_X2_sum", "min", "countNAs")}),
}
ROW_PALETTES = {
    "panel_short": ["a", "b_row", "c_up", "c_down", "d", "e", "i", "f"],
    "panel_strata": ["a", "b_row", "d", "i"],
    "whole_column": ["a", "d", "i"],
    "pipe_units": ["a"],
    "memory_atomics": ["a", "d", "i"],
}


@functools.lru_cache(maxsize=None)
def row_layout(name):
    spec = ROW_ROUTES[name]
    dim = spec["dim"]
    nrow, nleaf = dim[0], int(np.prod(dim[1:]))
    rng = np.random.default_rng(sorted(ROW_ROUTES).index(name) + 2000)
    # skewed leaves here too: a tenth of the leaves empty (or spec["empty"]), one a full column, the rest around the average
    lin = np.unique(rng.integers(0, nrow * nleaf, size=int(spec["nnz"] * 1.05)))[:spec["nnz"]]
    leaf = lin // nrow
    empty = rng.choice(nleaf, int(nleaf * spec.get("empty", 0.1)), replace=False)
    lin = lin[~np.isin(leaf, empty)]
    full = int(rng.integers(0, nleaf))
    lin = np.union1d(lin, full * nrow + np.arange(nrow))
    leaf = lin // nrow
    cp = np.concatenate([[0], np.cumsum(np.bincount(leaf, minlength=nleaf))]).astype(np.int64)
    return spec, cp, (lin % nrow).astype(np.int32)


@functools.lru_cache(maxsize=None)
def row_case(name, palette):
    spec, cp, ri = row_layout(name)
    c = Case()
    c.name, c.palette, c.dim, c.dims = name, palette, spec["dim"], spec["dims"]
    c.nrow, c.nleaf = c.dim[0], len(cp) - 1
    c.inner = int(np.prod(c.dim[1:c.dims]))
    c.nstrata = c.nleaf // c.inner
    c.col_ptr, c.row_idx = cp, ri
    rng = np.random.default_rng(sum(map(ord, name + palette)) + 7)
    val, c.scale = palette_values(palette, len(ri), rng)
    c.type = "double" if val.dtype == np.float64 else "integer"
    c.planted = palette in ("a", "i")
    leaf = np.repeat(np.arange(c.nleaf, dtype=np.int64), np.diff(cp))
    cell = (leaf % c.inner) * c.nrow + ri
    if c.planted:
        # at most one missing value per row cell (exact_stats.check_row_centered says why)
        hit = rng.choice(len(val), 6, replace=False)
        hit = hit[np.unique(cell[hit], return_index=True)[1]]
        na, nan = (NA_real, np.nan) if c.type == "double" else (NA_integer, NA_integer)
        val[hit] = [na if k % 2 == 0 else nan for k in range(len(hit))]
    c.val = val
    x = SVT_SparseArray.from_csc((c.nrow, c.nleaf), c.type, cp, ri, val)
    c.x = SVT_SparseArray(c.dim, c.type, x.leaves)
    # the cells that hold a stored value, renumbered; the others are all-zero cells with one known result each
    c.touched, small = np.unique(cell, return_inverse=True)
    c.ncell = c.inner * c.nrow
    c.cells = {na_rm: ex.Cells(val, small, len(c.touched), c.nstrata, na_rm) for na_rm in (False, True)}
    base = {"b_row": 1e3}.get(palette, 0.0)
    c.center = (base + 0.25 * (1 + np.arange(c.ncell) % 7)) * c.scale
    c.rest = np.ones(c.ncell, dtype=bool)
    c.rest[c.touched] = False
    c.rest_centered = (c.center * c.center * float(c.nstrata))[c.rest]
    c.ops = spec.get("ops", ROW_OPS)
    if palette == "e":
        c.ops = ["min", "max", "range", "countNAs"]
    if palette in ("c_up", "c_down"):
        c.ops = [op for op in c.ops if op != "prod"]
    return c


def assert_row_forms(c):
    for op, want in ROW_ROUTES[c.name]["forms"].items():
        got = rowstats_form(c.nrow, c.nleaf, len(c.val), op, c.inner)
        assert got == want, f"{c.name}: {op} takes {got}, not {want}"
    if c.name == "panel_short":
        assert c.nrow % 2048 != 0
    return ROW_ROUTES[c.name]["forms"]


def _row_form_of(c, op):
    one_pass = {"mean": "sum", "var1": "centered_X2_sum", "sd1": "centered_X2_sum", "range": "min", "max": "min",
                "prod": "min", "centered_X2_sum+center": "centered_X2_sum"}.get(op, op)
    return rowstats_form(c.nrow, c.nleaf, len(c.val), one_pass, c.inner)[0]


def check_row_stat(c, op, na_rm, got, rec=None, who=""):
    """One row statistic of every cell: the touched cells by their rule, the all-zero cells by their one value."""
    is_int = c.type == "integer"
    cells = c.cells[na_rm]
    got = _flat(got)
    what = f"{c.name}/{c.palette} na_rm={na_rm}"
    key = (who, "row " + op, _row_form_of(c, op))
    if op == "range":
        lo, hi = got[:c.ncell], got[c.ncell:]
        check_stat("min", lo[c.touched], cells, rec, key, is_int=is_int, what=what + " range")
        check_stat("max", hi[c.touched], cells, rec, key, is_int=is_int, what=what + " range")
        assert np.count_nonzero(got) == np.count_nonzero(lo[c.touched]) + np.count_nonzero(hi[c.touched]), what
        return
    center = None
    if op == "centered_X2_sum+center":
        op, center = "centered_X2_sum", c.center[c.touched]
    check_stat(op, got[c.touched], cells, rec, key, center=center, rows=True, is_int=is_int, what=what)
    # a cell without stored values: 0 (NaN counts as nonzero), or the start of the centred sum, c * c * nstrata
    if center is None:
        assert np.count_nonzero(got) == np.count_nonzero(got[c.touched]), f"{what} {op}: a cell without stored values"
    else:
        assert np.array_equal(got[c.rest], c.rest_centered), f"{what} {op}: a cell without stored values"


def run_row_case(sess, c, rec=None, who="", rowstat=None):
    """Every row statistic of the case through ``sess`` (row*() of a Session), or through ``rowstat(op, na_rm,
    center)`` when given (the device level; None = not served there)."""
    for na_rm in ((False, True) if c.planted else (False,)):
        for op in c.ops:
            with_center = op.endswith("+center")
            name = op.split("+")[0]
            center = c.center if with_center else None
            if rowstat is not None:
                got = rowstat(name, na_rm, center)
                if got is None:
                    continue
            elif name == "prod" and len(c.dim) > 2 and not sess._has_rowStatsFull():
                continue        # composed from aperm(): one leaf per row cell of a 3-d operand, minutes on the host
            elif name == "range":
                got = _quiet(sess.rowRanges, c.x, na_rm, c.dims)
            elif name in ("mean", "var1", "sd1"):
                f = {"mean": sess.rowMeans, "var1": sess.rowVars, "sd1": sess.rowSds}[name]
                got = _quiet(f, c.x, na_rm, dims=c.dims)
            else:
                cen = None if center is None else center.reshape(c.dim[:c.dims], order="F")
                got = _quiet(sess._rowStats, name, c.x, na_rm, cen, c.dims)
            check_row_stat(c, op, na_rm, got, rec, who)


# ---------------------------------------------------------------------------
# rowsum / colsum: 6000 rows, 50 columns
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def groupsum_case(palette, ngroup):
    rng = np.random.default_rng(3000 + ngroup + sum(map(ord, palette)))
    nrow, ncol, nnz = 6000, 50, 15000
    lin = np.unique(rng.integers(0, nrow * ncol, size=int(nnz * 1.05)))[:nnz]
    c = Case()
    c.palette, c.ngroup, c.nrow, c.ncol = palette, ngroup, nrow, ncol
    c.col_ptr = np.concatenate([[0], np.cumsum(np.bincount(lin // nrow, minlength=ncol))]).astype(np.int64)
    c.row_idx = (lin % nrow).astype(np.int32)
    c.val, _ = palette_values(palette, len(lin), rng)
    c.planted = palette == "a"
    if c.planted:
        c.val[rng.choice(len(lin), 4, replace=False)] = [NA_real, np.nan, NA_real, np.nan]
    c.group0 = rng.integers(0, ngroup, nrow)
    c.group0[:ngroup] = np.arange(ngroup)                  # every group occurs: ugroup is 0 .. ngroup - 1
    c.x = SVT_SparseArray.from_csc((nrow, ncol), "double", c.col_ptr, c.row_idx, c.val)
    c.xt = c.x.t()
    c.rowsum = {r: ex.rowsum_cells(c.col_ptr, c.row_idx, c.val, c.group0, ngroup, r) for r in (False, True)}
    return c


def run_groupsum_case(sess, c, rec=None, who=""):
    """rowsum(x, group) and colsum(t(x), group): the same cells, the second transposed."""
    grp = [int(g) for g in c.group0]
    for na_rm in ((False, True) if c.planted else (False,)):
        got, ug = sess.rowsum(c.x, grp, na_rm=na_rm)
        assert list(ug) == list(range(c.ngroup))
        _note(rec, (who, "rowsum", str(c.ngroup)), ex.check_sum(_flat(got), c.rowsum[na_rm], f"rowsum {c.palette}"))
        got, _ = sess.colsum(c.xt, grp, na_rm=na_rm)      # t(x): (ncol, nrow); cells (j, g)
        got = np.asarray(got).T                             # -> (g, j), the cells of rowsum
        _note(rec, (who, "colsum", str(c.ngroup)), ex.check_sum(_flat(got), c.rowsum[na_rm], f"colsum {c.palette}"))
