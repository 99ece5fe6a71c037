"""The cases of the workspace-discipline tests (test_ws_cases_cpu.py, test_hip_ws_discipline.py): every device-level
entry point of the product and row-statistics families that takes a caller's workspace, on hand-built operands, with
the route each case claims and its expected outputs.

Values are small integers (|v| <= 9, none stored as 0) held as doubles or as int32 -- the dense cases of
tests/product_cases.py keep their "tracer" palette, which is exact too -- so every sum stays far below 2^53, is exact in
any order, and the expectation is plain numpy on int64, compared as bits.  var1 is exact as well: its cases have a
power of two of strata, so the row means and the squared deviations are dyadic numbers of few bits.

A case is a dict: "name", "entry" (the key of the runner in test_hip_ws_discipline.py), the operands as pattern specs,
the route it claims ("route", "form", "plan" ...: asserted without a GPU by test_ws_cases_cpu.py), "deg" for the
degenerate operands.  ``operands(case)`` builds the host operands (cached), ``expected(case)`` the list of output
arrays in the order the runner lays them out in its arena; the not-finite flag and the warn word are outputs too.
"""
from __future__ import annotations

import functools

import numpy as np

import product_cases as pc
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd._hip import load_library
from sparsearray_amd.api import OPCODES
from sparsearray_amd.svt import INTSXP, REALSXP

NP_OF = {"double": np.float64, "integer": np.int32}


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
class Op:
    """A sparse operand on the host: nrow x ncol leaves in the CSC layout of the device level."""

    def __init__(self, nrow, ncol, cp, ri, val):
        self.nrow, self.ncol = int(nrow), int(ncol)
        self.cp, self.ri, self.val = np.asarray(cp, np.int64), np.asarray(ri, np.int32), np.asarray(val)
        assert len(self.cp) == self.ncol + 1 and self.cp[-1] == len(self.ri) == len(self.val)
        self.col = np.repeat(np.arange(self.ncol, dtype=np.int64), np.diff(self.cp))

    nnz = property(lambda self: len(self.ri))
    type = property(lambda self: "integer" if self.val.dtype == np.int32 else "double")

    def dense(self):
        """int64, nrow x ncol; finite operands only"""
        v = self.val.astype(np.float64)
        assert np.all(np.isfinite(v)) and np.all(v == np.rint(v)) and not np.any(self.val == NA_integer)
        d = np.zeros((self.nrow, self.ncol), dtype=np.int64)
        d[self.ri, self.col] = v.astype(np.int64)
        return d

    def dense_float(self):
        d = np.zeros((self.nrow, self.ncol))
        d[self.ri, self.col] = self.val
        return d

    def t(self):
        order = np.lexsort((self.col, self.ri))
        cp = np.concatenate([[0], np.cumsum(np.bincount(self.ri, minlength=self.nrow))])
        return Op(self.ncol, self.nrow, cp, self.col[order], self.val[order])

    def put(self, k, v):
        """a copy with stored entry k replaced by v"""
        val = self.val.copy()
        val[k] = v
        return Op(self.nrow, self.ncol, self.cp, self.ri, val)

    def svt(self, dim=None):
        return SVT_SparseArray.from_csc(dim or (self.nrow, self.ncol), self.type, self.cp, self.ri, self.val)


def small_values(ri, col, type, which=0):
    """+-(1 + (a r + b c) mod 9), the sign from (3 r + c) mod 2: 1 <= |v| <= 9"""
    r, c = np.asarray(ri, np.int64), np.asarray(col, np.int64)
    a, b = ((7, 13), (11, 17), (5, 3))[which]
    return ((1 + (a * r + b * c) % 9) * (1 - 2 * ((3 * r + c) % 2))).astype(NP_OF[type])


def pattern(spec):
    """(nrow, ncol, cp, ri) of a pattern spec:
    ("rand", nrow, ncol, density, seed)   uniform
    ("count", nrow, ncol, nnz, seed)      exactly nnz nonzeros, uniform (the wide row operands)
    ("empty", nrow, ncol)                 no nonzero (either extent may be 0)
    ("last_col", nrow, ncol, n)           every column empty but the last, which holds n
    ("one_row", nrow, ncol, r)            every nonzero in row r, one per column
    ("full", nrow, ncol)                  every cell stored
    ("bcols", ninner, K, seed)            the second operand of the spmm cases (``_bcols``)"""
    kind, nrow, ncol = spec[:3]
    if kind == "rand":
        return (nrow, ncol) + pc.pattern_random(nrow, ncol, spec[3], spec[4])
    if kind == "count":
        lin = np.sort(np.random.default_rng(spec[4]).choice(nrow * ncol, size=spec[3], replace=False))
        row, col = lin % nrow, lin // nrow
    elif kind == "empty":
        row = col = np.zeros(0, np.int64)
    elif kind == "last_col":
        row, col = (np.arange(spec[3]) * 7) % nrow, np.full(spec[3], ncol - 1)
        assert len(np.unique(row)) == spec[3]
    elif kind == "one_row":
        row, col = np.full(ncol, spec[3]), np.arange(ncol)
    elif kind == "full":
        row, col = np.tile(np.arange(nrow), ncol), np.repeat(np.arange(ncol), nrow)
    elif kind == "bcols":
        return _bcols(nrow, ncol, spec[3])
    else:
        raise KeyError(kind)
    return (nrow, ncol) + pc._csc_from_pairs(ncol, np.asarray(row, np.int64), np.asarray(col, np.int64))


@functools.lru_cache(maxsize=64)
def operand(spec, type="double", which=0) -> Op:
    nrow, ncol, cp, ri = pattern(spec)
    col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(cp))
    return Op(nrow, ncol, cp, ri, small_values(ri, col, type, which))


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
CASES = []


def _case(name, entry, **kw):
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(name=name, entry=entry, **kw))


# ---- sparse x sparse crossprod (kernels_gram.hip) --------------------------------------------------------------
# 300 rows; X with 40 / 41 / 64 / 65 / 129 columns at 15 %, Y with 23 columns at 10 %.  One block of cells per result
# column by default (gram_gen_kernel; symmetric: gram_sym_kernel, columns j and nx - 1 - j per workgroup, so an odd nx
# pairs the middle column with itself); under set_sparse_crossprod_panel(0, 6) panels of 64 cells (gram_pan_kernel;
# symmetric: cut at the diagonal cell).  "panels": (number of panels, cells of the last one).
GRAM_PANEL = (0, 6)
GRAM_Y = ("rand", 300, 23, 0.10, 50)


def _gram_x(nx):
    return ("rand", 300, nx, 0.15, 40 + nx)


for _nx, _types in ((41, ("double", "double")), (64, ("integer", "integer")), (40, ("double", "integer")),
                    (65, ("integer", "double"))):
    _case(f"gram_gen_one_{_nx}_{_types[0][0]}{_types[1][0]}", "gram", x=_gram_x(_nx), y=GRAM_Y, types=_types, sym=False,
          panel=None, route="gen_one")
for _nx, _t in ((41, "double"), (64, "double"), (65, "integer")):
    _case(f"gram_sym_one_{_nx}_{_t[0]}", "gram", x=_gram_x(_nx), y=None, types=(_t, _t), sym=True, panel=None,
          route="sym_one", middle_pairs_itself=_nx % 2 == 1)
for _nx, _pan in ((40, (1, 40)), (64, (1, 64)), (65, (2, 1)), (129, (3, 1))):
    _case(f"gram_gen_pan_{_nx}", "gram", x=_gram_x(_nx), y=GRAM_Y, types=("double", "double"), sym=False,
          panel=GRAM_PANEL, route="gen_pan", panels=_pan)
    _case(f"gram_sym_pan_{_nx}", "gram", x=_gram_x(_nx), y=None,
          types=("integer", "integer") if _nx == 65 else ("double", "double"), sym=True, panel=GRAM_PANEL,
          route="sym_pan", panels=_pan)

# ---- sparse x sparse matmul (kernels_spmm.hip) ------------------------------------------------------------------
# A nrow x 120 at 2 % (at most 20 k nonzeros), B 120 x K at 20 % inside the leaves 0 .. 79 of A: the leaves 80 .. 119
# are the ones "no column of B refers to", looked at by the table pass only.  spmm_shape: panels of 2^ps rows, ps the
# smallest in 6 .. 13 with 2^ps >= nrow ("ps", "npan": restated by test_ws_cases_cpu.py); 8192 rows are the one size
# that fills a panel of 8192, 8193 the first with two.  Both forms run: the one-call product, and SpmmPlan's prepare
# with two products (B, then B2) on the one prepared workspace.
SPMM_INNER, SPMM_REFERENCED = 120, 80
SPMM_SHAPE = {1: (6, 1), 64: (6, 1), 65: (7, 1), 8192: (13, 1), 8193: (13, 2)}


def _spmm_a(nrow):
    return ("rand", nrow, SPMM_INNER, max(0.02, min(0.5, 60.0 / nrow)), 60 + nrow % 11)


def _spmm_b(K, seed):
    return ("bcols", SPMM_INNER, K, seed)


for _nrow in (1, 64, 65, 8192, 8193):
    for _K in (1, 16, 17):
        for _types in pc.TYPE_PAIRS:
            for _form in ("spmm", "spmm_prepared"):
                _case(f"{_form}_{_nrow}_K{_K}_{_types[0][0]}{_types[1][0]}", _form, a=_spmm_a(_nrow), b=_spmm_b(_K, 70 + _K),
                      b2=_spmm_b(_K, 90 + _K), types=_types, ps=SPMM_SHAPE[_nrow][0], npan=SPMM_SHAPE[_nrow][1])

# ---- row side (kernels_rowstats.hip) -----------------------------------------------------------------------------
# One operand per form of svt_dev_rowstats_form, the shapes of tests/stats_cases.py (ROW_ROUTES) with a power of two
# of strata where var1 runs (see the module docstring).  "forms": what one pass of the operation must take, as
# (form, panel_shift, nsplit); mean queues the pass "sum", var1 "sum" and "centered_X2_sum".  Form 0 serves sums and
# counts only and form 4 the reference's six operations, so those operands leave var1 (and 4: mean, range) out.
ROW_OPERANDS = {
    # 3: row panels of 2048 rows, the last one ragged
    "f3_short": dict(dim=(2500, 32), inner=1, nnz=10000, seed=1,
                     forms={"sum": ("panel", 11, 1), "min": ("panel", 11, 1), "centered_X2_sum": ("panel", 11, 1)}),
    # 3 with the strata cut into ranges that are added to a zeroed result (nsplit > 1)
    "f3_strata": dict(dim=(16500, 512), inner=1, nnz=85000, seed=2,
                      forms={"sum": ("panel", 13, 8), "min": ("panel", 11, 1), "centered_X2_sum": ("panel", 13, 8)}),
    # 1 (sums) and 2 (centred sums): all rows of an output column in LDS; inner = 1030 output columns
    "f12_whole": dict(dim=(8500, 1030, 4), inner=1030, nnz=60000, seed=3,
                      forms={"sum": ("pipe", 0, 1), "centered_X2_sum": ("whole_column", 0, 1), "min": ("panel", 11, 1)}),
    # 0: (output column, chunk of 64 leaves) units; 65 strata make two chunks
    "f0_units": dict(dim=(8200, 1024, 65), inner=1024, nnz=540000, seed=4, ops=("sum", "min", "range", "mean"),
                     forms={"sum": ("pipe_units", 0, 1), "min": ("panel", 11, 1)}),
    # 4: memory atomics, more than 65535 output columns; two rows
    "f4_atomics": dict(dim=(2, 65536, 4), inner=65536, nnz=60000, seed=5, ops=("sum", "min"),
                       forms={"sum": ("memory_atomics", 0, 1), "min": ("memory_atomics", 0, 1)}),
}
ROW_OPS = ("sum", "min", "range", "mean", "var1")
ROW_PASSES = {"sum": ("sum",), "min": ("min",), "range": ("min",), "mean": ("sum",), "var1": ("sum", "centered_X2_sum")}


def _row_x(name):
    r = ROW_OPERANDS[name]
    return ("count", r["dim"][0], int(np.prod(r["dim"][1:])), r["nnz"], 100 + r["seed"])


for _n, _r in ROW_OPERANDS.items():
    for _t in ("double", "integer"):
        if _r["inner"] <= 65535:
            _case(f"rowsums_{_n}_{_t[0]}", "rowsums", x=_row_x(_n), type=_t, row=_n, inner=_r["inner"], op="sum")
            _case(f"rowsums_prepared_{_n}_{_t[0]}", "rowsums_prepared", x=_row_x(_n), type=_t, row=_n, inner=_r["inner"],
                  op="sum")
        for _op in _r.get("ops", ROW_OPS):
            _case(f"rowstats_{_op}_{_n}_{_t[0]}", "rowstats", x=_row_x(_n), type=_t, row=_n, inner=_r["inner"], op=_op)

# ---- colMedians (kernels_median.hip) ---------------------------------------------------------------------------
# The operand of tests/test_medians.py::test_hip_colmedians_radix_select_against_numpy, built by ``median_operand``:
# columns of every length class of the count and select kernels, duplicates, low-bit differences, +-Inf.
_case("colmedians_routes", "colmedians", x="median_operand")
_case("colmedians_small", "colmedians", x=("rand", 101, 60, 0.4, 83))

# ---- rowsum(): the ids of every nonzero, prepared once (kernels_rowstats.hip, launch_rowsum_gid) ---------------------
# One operand per svt_dev_rowsum_prepare_form: "flat" (two ids per thread) and "windowed" (65536 rows, 64 columns and
# more); the workspace of these calls is the `gid` buffer.  Groups: ``group_of``.
_case("rowsum_ids_flat", "rowsum_prepared", x=("rand", 600, 30, 0.1, 81), ngroup=5, form=("flat", 0))
_case("rowsum_ids_windowed", "rowsum_prepared", x=("rand", 65536, 66, 0.002, 82), ngroup=7, form=("windowed", 8))

# ---- sparse x dense (kernels_mult.hip, kernels_mult_pbc.hip) ------------------------------------------------------
# structures and the tracer palette of tests/product_cases.py.  svt_dev_crossprod_csc_dense has the general kernels
# only; svt_dev_crossprod_pbc takes them below 256 rows ("none"), else the kernel of its layout.
for _s, _K, _layout, _kind in (("general255", 20, (40, 16, 7), "none"), ("small256", 1, (40, 16, 7), "dma"),
                               ("gather5000", 70, (40, 4, 9), "gather")):
    _case(f"csc_dense_{_s}", "csc_dense", structure=_s, K=_K)
    _case(f"pbc_{_s}", "pbc", structure=_s, K=_K, layout=_layout, kind=_kind)

# ---- degenerate operands -------------------------------------------------------------------------------------------
# An extent of 0 on each axis in turn, no nonzero at all, one row, one column, every column empty but the last, every
# nonzero in one row.  The expectation is the dense rule; a result without cells has a flag of 0.
_DD = ("double", "double")
for _deg, _x, _y in (("nx0", ("empty", 30, 0), ("rand", 30, 5, 0.3, 1)), ("ny0", ("rand", 30, 6, 0.3, 2), ("empty", 30, 0)),
                     ("inner0", ("empty", 0, 6), ("empty", 0, 5)), ("x_nnz0", ("empty", 30, 6), ("rand", 30, 5, 0.3, 3)),
                     ("y_nnz0", ("rand", 30, 6, 0.3, 4), ("empty", 30, 5)), ("one_row", ("full", 1, 6), ("full", 1, 5)),
                     ("one_col", ("rand", 30, 1, 0.5, 5), ("rand", 30, 1, 0.5, 6)),
                     ("last_col", ("last_col", 30, 6, 9), ("last_col", 30, 5, 11)),
                     ("one_row_only", ("one_row", 30, 6, 17), ("one_row", 30, 5, 17))):
    for _panel in (None, GRAM_PANEL):
        _p = "pan" if _panel else "one"
        _case(f"gram_gen_{_p}_{_deg}", "gram", x=_x, y=_y, types=_DD, sym=False, panel=_panel, deg=_deg)
        if _deg not in ("ny0", "y_nnz0"):
            _case(f"gram_sym_{_p}_{_deg}", "gram", x=_x, y=None, types=_DD, sym=True, panel=_panel, deg=_deg)
for _deg, _a, _b in (("nrow0", ("empty", 0, 12), ("rand", 12, 4, 0.4, 7)), ("K0", ("rand", 20, 12, 0.3, 8), ("empty", 12, 0)),
                     ("inner0", ("empty", 20, 0), ("empty", 0, 4)), ("a_nnz0", ("empty", 20, 12), ("rand", 12, 4, 0.4, 9)),
                     ("b_nnz0", ("rand", 20, 12, 0.3, 10), ("empty", 12, 4)), ("one_row", ("full", 1, 12), ("rand", 12, 4, 0.4, 11)),
                     ("one_col", ("rand", 20, 12, 0.3, 12), ("rand", 12, 1, 0.5, 13)),
                     ("last_col", ("last_col", 20, 12, 7), ("last_col", 12, 4, 5)),
                     ("one_row_only", ("one_row", 20, 12, 3), ("one_row", 12, 4, 11))):
    for _form in ("spmm", "spmm_prepared"):
        _case(f"{_form}_{_deg}", _form, a=_a, b=_b, b2=_b, types=_DD, deg=_deg)
for _deg, _x, _ops in (("nrow0", ("empty", 0, 8), ("sum",)), ("ncol0", ("empty", 40, 0), ("sum",)),
                       ("nnz0", ("empty", 40, 8), ROW_OPS), ("one_row", ("full", 1, 8), ROW_OPS),
                       ("one_col", ("rand", 40, 1, 0.5, 14), ("sum", "min", "range", "mean")),
                       ("last_col", ("last_col", 40, 8, 9), ROW_OPS), ("one_row_only", ("one_row", 40, 8, 21), ROW_OPS)):
    _case(f"rowsums_{_deg}", "rowsums", x=_x, type="double", inner=1, op="sum", deg=_deg)
    _case(f"rowsums_prepared_{_deg}", "rowsums_prepared", x=_x, type="double", inner=1, op="sum", deg=_deg)
    for _op in _ops:
        _case(f"rowstats_{_op}_{_deg}", "rowstats", x=_x, type="integer" if _deg == "last_col" else "double", inner=1,
              op=_op, deg=_deg)
for _deg, _x in (("nrow0", ("empty", 0, 5)), ("ncol0", ("empty", 40, 0)), ("nnz0", ("empty", 40, 5)), ("one_row", ("full", 1, 5)),
                 ("one_col", ("rand", 40, 1, 0.5, 15)), ("last_col", ("last_col", 40, 5, 30)),
                 ("one_row_only", ("one_row", 40, 5, 2))):
    _case(f"colmedians_{_deg}", "colmedians", x=_x, deg=_deg)
for _deg, _x in (("ncol0", ("empty", 40, 0)), ("nnz0", ("empty", 40, 5)), ("one_row", ("full", 1, 5)),
                 ("one_col", ("rand", 40, 1, 0.5, 16)), ("last_col", ("last_col", 40, 5, 30)),
                 ("one_row_only", ("one_row", 40, 5, 2))):
    _case(f"rowsum_ids_{_deg}", "rowsum_prepared", x=_x, ngroup=3, deg=_deg)
# (the dense products return before they look at their workspace when ncol or K is 0, and a panel-blocked layout of an
# operand without rows or columns is not a product anybody launches: positive extents here, K = 3)
for _deg, _x in (("nnz0", ("empty", 40, 5)), ("one_row", ("full", 1, 5)), ("one_col", ("rand", 40, 1, 0.5, 17)),
                 ("last_col", ("last_col", 40, 5, 30)), ("one_row_only", ("one_row", 40, 5, 2))):
    _case(f"csc_dense_{_deg}", "csc_dense", x=_x, K=3, deg=_deg)
    _case(f"pbc_{_deg}", "pbc", x=_x, K=3, layout=(40, 16, 7), kind="none", deg=_deg)
_case("csc_dense_nrow0", "csc_dense", x=("empty", 0, 5), K=3, deg="nrow0")

BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
ENTRIES = sorted({c["entry"] for c in CASES})


def other_case(case):
    """Another case of the same entry point, on a different operand: the next one of the table that is not degenerate
    (cyclically), whose call leaves the workspace behind that property (c) reuses."""
    same = [c for c in CASES if c["entry"] == case["entry"] and "deg" not in c]
    later = [c for c in same if NAMES.index(c["name"]) > NAMES.index(case["name"])] + same
    return next(c for c in later if c["name"] != case["name"] and _operand_key(c) != _operand_key(case))


def _operand_key(c):
    return tuple(repr(c.get(k)) for k in ("x", "y", "a", "b", "structure", "type", "types"))


# ---------------------------------------------------------------------------
# operands and expectations per entry
# ---------------------------------------------------------------------------
def _bcols(ninner, K, seed):
    """B of the spmm cases: ninner x K at 20 % inside the leaves 0 .. SPMM_REFERENCED - 1, every one of them named"""
    rng = np.random.default_rng(seed)
    hit = rng.random((SPMM_REFERENCED, K)) < 0.2
    hit[np.arange(SPMM_REFERENCED), np.arange(SPMM_REFERENCED) % K] = True
    row, col = np.nonzero(hit)
    return (ninner, K) + pc._csc_from_pairs(K, row, col)


def _spec_operand(spec, type, which):
    return operand(spec, type, which)


@functools.lru_cache(maxsize=1)
def median_operand() -> Op:
    from test_medians import last_digit_columns
    rng = np.random.default_rng(66)
    nrow, cols = 5000, []
    for j in range(30):
        col = np.zeros(nrow)
        m = rng.random(nrow) < [1.0, 0.97, 0.8, 0.6, 0.51, 0.3][j % 6]
        kind = (j // 6) % 5
        v = (rng.normal(size=nrow), rng.integers(-3, 4, nrow).astype(np.float64),
             1.0 + rng.integers(0, 1 << 20, nrow) * 2.0 ** -52, -np.abs(rng.normal(size=nrow)) - (j % 3),
             np.abs(rng.normal(size=nrow)) * 1e200 * (1 if j % 2 else -1))[kind]
        col[m] = v[m]
        cols.append(col)
    short = np.zeros((nrow, 6))                             # few stored values among many zeros
    short[:3, 0] = [5, 6, 7]
    short[:nrow // 2 + 1, 1] = 2.0
    short[: nrow // 2, 2] = -2.0; short[nrow // 2:, 2] = 3.0
    short[:, 3] = np.arange(nrow) - 100.0
    short[:, 4] = np.where(np.arange(nrow) % 2 == 0, -1.0, 1.0)
    short[:, 5] = 7.0
    a = np.concatenate([np.stack(cols, axis=1), short, last_digit_columns(nrow)], axis=1)
    a[17, 3] = np.inf; a[18, 3] = -np.inf
    row, col = np.nonzero(a)
    cp, ri = pc._csc_from_pairs(a.shape[1], row, col)
    return Op(nrow, a.shape[1], cp, ri, a.T[a.T != 0])


def group_of(nrow, ngroup):
    """The int32 group ids of the rowsum cases (1-based, NA_integer every 97th row) and their 0-based slots: the last
    slot is the NA group (src/rowsum_methods.c:51-54) and holds the NA rows only"""
    r = np.arange(nrow, dtype=np.int64)
    slot = (3 * r + 1) % (ngroup - 1)
    na = r % 97 == 96
    slot[na] = ngroup - 1
    g = (slot + 1).astype(np.int32)
    g[na] = NA_integer
    return g, slot


@functools.lru_cache(maxsize=8)
def _operands(name):
    c = BY_NAME[name]
    e = c["entry"]
    if e == "gram":
        X = _spec_operand(c["x"], c["types"][0], 0)
        return dict(X=X, Y=X if c["sym"] else _spec_operand(c["y"], c["types"][1], 1))
    if e in ("spmm", "spmm_prepared"):
        return dict(A=_spec_operand(c["a"], c["types"][0], 0), B=_spec_operand(c["b"], c["types"][1], 1),
                    B2=_spec_operand(c["b2"], c["types"][1], 2))
    if e in ("csc_dense", "pbc"):
        if "structure" in c:
            ex = pc.expected(c["structure"], "tracer", c["K"])
            return dict(A=Op(ex.st.nrow, ex.st.ncol, ex.st.cp, ex.st.ri, ex.val), Y=ex.Y)
        A = _spec_operand(c["x"], "double", 0)
        r, k = np.arange(A.nrow, dtype=np.int64)[:, None], np.arange(c["K"], dtype=np.int64)[None, :]
        return dict(A=A, Y=(((5 * r + 3 * k) % 19) - 9).astype(np.float64))
    if c["x"] == "median_operand":
        return dict(A=median_operand())
    return dict(A=_spec_operand(c["x"], c.get("type", "double"), 0))


def operands(case):
    return _operands(case["name"])


def rowstats_dtype(op, type):
    rt = load_library().svt_colStats_out_Rtype(OPCODES[op], INTSXP if type == "integer" else REALSXP)
    return np.float64 if rt == REALSXP else np.int32


def row_expected(x: Op, inner, op, dtype, parts=False):
    """The row statistic of every cell (j mod inner) * nrow + r over the strata j div inner, implicit zeros included.
    ``parts``: the exact integers behind it as well (test_ws_cases_cpu.py bounds them)."""
    nrow, nstrata, ncell = x.nrow, x.ncol // inner, inner * x.nrow
    cell = (x.col % inner) * nrow + x.ri
    v = x.val.astype(np.int64)
    cnt = np.bincount(cell, minlength=ncell)
    S = np.zeros(ncell, np.int64)
    np.add.at(S, cell, v)
    big = S
    if op == "sum":
        out = S.astype(dtype)
    elif op in ("min", "max", "range"):
        assert nstrata > 0
        lo, hi = np.full(ncell, 10, np.int64), np.full(ncell, -10, np.int64)
        np.minimum.at(lo, cell, v)
        np.maximum.at(hi, cell, v)
        lo, hi = np.where(cnt < nstrata, np.minimum(lo, 0), lo), np.where(cnt < nstrata, np.maximum(hi, 0), hi)
        out = {"min": lo, "max": hi, "range": np.concatenate([lo, hi])}[op].astype(dtype)
    elif op == "mean":
        assert nstrata > 0
        out = S.astype(np.float64) / float(nstrata)
    elif op == "var1":
        N = nstrata
        assert N > 1 and N & (N - 1) == 0, "var1 is exact for a power of two of strata"
        Q = np.zeros(ncell, np.int64)                       # N^2 * sum over the strata of (x - S / N)^2
        np.add.at(Q, cell, (N * v - S[cell]) ** 2)
        Q += (N - cnt) * S * S
        big = Q
        out = Q.astype(np.float64) / float(N * N) / (N - 1.0)
    else:
        raise KeyError(op)
    return (out, big) if parts else out


def dense_colmedians(a):
    from test_medians import dense_colmedians as rule
    return rule(a, False)


@functools.lru_cache(maxsize=8)
def _expected(name):
    c = BY_NAME[name]
    e, o = c["entry"], operands(c)
    zero = np.zeros(1, np.int32)
    if e == "gram":
        return [(o["Y"].dense().T @ o["X"].dense()).astype(np.float64), zero]            # (ny, nx) = col-major nx x ny
    if e == "spmm":
        return [(o["A"].dense() @ o["B"].dense()).T.astype(np.float64), zero]            # (K, nrow)
    if e == "spmm_prepared":
        A = o["A"].dense()
        return [(A @ o["B"].dense()).T.astype(np.float64), zero, (A @ o["B2"].dense()).T.astype(np.float64), zero]
    if e in ("rowsums", "rowsums_prepared"):
        return [row_expected(o["A"], c["inner"], "sum", np.float64)]
    if e == "rowstats":
        return [row_expected(o["A"], c["inner"], c["op"], rowstats_dtype(c["op"], c["type"])), zero]
    if e == "colmedians":
        return [dense_colmedians(o["A"].dense_float())]
    if e == "rowsum_prepared":
        A, (_, slot) = o["A"], group_of(o["A"].nrow, c["ngroup"])
        out = np.zeros((A.ncol, c["ngroup"]), np.int64)                                  # (ncol, ngroup) = col-major
        np.add.at(out, (A.col, slot[A.ri]), A.val.astype(np.int64))
        return [out.astype(np.float64)]
    if e in ("csc_dense", "pbc"):
        return [(o["Y"].astype(np.int64).T @ o["A"].dense()).astype(np.float64)]          # (K, ncol)
    raise KeyError(e)


def expected(case):
    return _expected(case["name"])


# ---------------------------------------------------------------------------
# the not-finite flag (device level): small operands, one bad value each
# ---------------------------------------------------------------------------
# gram: X 50 x 12, Y 50 x 7.  spmm: A 40 x 20, B 20 x 6 inside the leaves 0 .. 11 of A; leaf 5 is referenced, leaf 15 is
# not, the first stored entry of A lies in leaf 0 (referenced), the last in leaf 19 (not referenced).
FLAG_VALUES = {"NaN": ("double", np.nan), "Inf": ("double", np.inf), "NA_real": ("double", NA_real),
               "NA_integer": ("integer", NA_integer)}
FLAG_GRAM_X, FLAG_GRAM_Y = ("rand", 50, 12, 0.3, 21), ("rand", 50, 7, 0.3, 22)
FLAG_SPMM_A = ("rand", 40, 20, 0.3, 23)
FLAG_REFERENCED = 12
FLAG_PLACES = {
    "gram_gen": ("x_first", "x_last", "y"), "gram_sym": ("x_first", "x_last"),
    "spmm": ("a_first", "a_last", "a_unreferenced", "a_referenced", "b"),
    "spmm_prepared": ("a_first", "a_last", "a_unreferenced", "a_referenced", "b"),
}
FLAG_CASES = [(form, place, value) for form, places in FLAG_PLACES.items() for place in places for value in FLAG_VALUES]
# which leaf of A an "a_*" placement must lie in, and whether some column of B names it
FLAG_LEAF = {"a_first": (0, True), "a_last": (19, False), "a_unreferenced": (15, False), "a_referenced": (5, True)}


def _flag_b(type):
    rng = np.random.default_rng(24)
    hit = rng.random((FLAG_REFERENCED, 6)) < 0.3
    hit[np.arange(FLAG_REFERENCED), np.arange(FLAG_REFERENCED) % 6] = True            # every leaf 0 .. 11 is named
    row, col = np.nonzero(hit)
    cp, ri = pc._csc_from_pairs(6, row, col)
    return Op(20, 6, cp, ri, small_values(ri, np.repeat(np.arange(6), np.diff(cp)), type, 1))


def flag_operands(form, place, value):
    """(clean operands, dirty operands, index of the bad entry) of a flag case, as dicts like ``operands``"""
    type, bad = FLAG_VALUES[value]
    dirty_first = place[0] in "xa"                          # the operand that carries the bad value has its type
    t0, t1 = (type, "double") if dirty_first else ("double", type)
    if form.startswith("gram"):
        X = operand(FLAG_GRAM_X, t0, 0)
        if form == "gram_sym":
            clean = dict(X=X, Y=X)
        else:
            clean = dict(X=X, Y=operand(FLAG_GRAM_Y, t1, 1))
        k = {"x_first": 0, "x_last": X.nnz - 1, "y": clean["Y"].nnz // 2}[place]
        if place == "y":
            return clean, dict(X=X, Y=clean["Y"].put(k, bad)), k
        Xd = X.put(k, bad)
        return clean, dict(X=Xd, Y=Xd if form == "gram_sym" else clean["Y"]), k
    A, B = operand(FLAG_SPMM_A, t0, 0), _flag_b(t1)
    clean = dict(A=A, B=B, B2=B)
    if place == "b":
        k = B.nnz // 2
        Bd = B.put(k, bad)
        return clean, dict(A=A, B=Bd, B2=Bd), k
    leaf = FLAG_LEAF[place][0]
    k = {"a_first": 0, "a_last": A.nnz - 1}.get(place, int(A.cp[leaf] + A.cp[leaf + 1]) // 2)
    return clean, dict(A=A.put(k, bad), B=B, B2=B), k


def flag_expected(form, clean):
    if form.startswith("gram"):
        return (clean["Y"].dense().T @ clean["X"].dense()).astype(np.float64)
    return (clean["A"].dense() @ clean["B"].dense()).T.astype(np.float64)


# ---------------------------------------------------------------------------
# the sharded sparse crossprod's local block (parallel.device_sparse_crossprod_block)
# ---------------------------------------------------------------------------
SHARD_A, SHARD_B = ("rand", 60, 9, 0.3, 31), ("rand", 60, 11, 0.3, 32)
SHARD_CASES = [("clean", None)] + [(w, v) for w in ("a", "b") for v in ("NaN", "Inf", "NA_real")]


def shard_operands(where, value):
    A, B = operand(SHARD_A, "double", 0), operand(SHARD_B, "double", 1)
    if where == "a":
        A = A.put(A.nnz // 3, FLAG_VALUES[value][1])
    if where == "b":
        B = B.put(B.nnz // 3, FLAG_VALUES[value][1])
    return A, B
