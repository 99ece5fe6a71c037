"""The cases of the rowsum / colsum tests (test_groupsum_cases_cpu.py, test_hip_groupsum_cases.py): one hand-built
operand per launch form of rowsum() and of its prepared form (kernels_rowstats.hip: rowsum_route, rowsum_gid_route,
rowsum_prepared_route), each named after the form it must take -- asserted through the host queries
svt_dev_rowsum_form / _prepare_form / _prepared_form, never assumed -- and the checker that holds every cell of a result
to an exact expectation.

Layout of a tall case: the twelve *window columns* first (``window_columns``: nonzeros on both sides of every window
edge the kernel's walk meets, exactly 63 / 64 / 65 / 128 of them inside one window, the last rows of the matrix), then
columns of the lengths the case names (the strides of the kernel that reads them), then random fill sized so that the
route condition nnz / ncol >= ngroup / 4 holds or fails as the form needs.  W, the window, is what the query reports.

Groups: ``slot`` (0-based, one per row) with every slot taken; the last slot is the NA group
(src/rowsum_methods.c:44-64): about 1e-3 of the rows carry NA_integer, other rows of that slot the explicit id
``ngroup``; at the R level (Session.rowsum) all of them are ``None``.  Variant "distinct": rows 0, W - 1, W and nrow - 1
in pairwise different slots (as far as ngroup allows); variant "na_ends": rows 0 and nrow - 1 in the NA group.

Palettes: "tracer" -- integer-valued doubles +-(1 .. 2**20), every cell sum an integer below 2**53 and exact in any
order of additions, compared at tolerance 0 with an int64 total: a dropped, doubled or misrouted nonzero changes a
cell; "a" and "d" of stats_cases (full mantissas with four planted NA / NaN; magnitudes over 2**+-60), held to
exact_stats.check_sum; "itracer" -- the same as int32 with two planted NAs, for the integer entry points.

``Expect.check`` looks at EVERY cell of a result the test allocated and filled with a sentinel: none may keep the
sentinel; a cell without a stored value is +0.0 (sign bit clear); a cell with one stored value is that value bit for
bit; a cell decided by a planted missing value (na_rm off; at most four per case, asserted) is NaN / NA_integer; every
other cell is the exact total (tracer, integers) or within gamma(n - 1) * sum |x| of it.
"""
from __future__ import annotations

import functools
from ctypes import byref, c_int

import numpy as np

import exact_stats as ex
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd._dispatch import _ptr
from sparsearray_amd._hip import rowsum_form, rowsum_prepare_form, rowsum_prepared_form
from sparsearray_amd.svt import make_view
from stats_cases import Case, palette_values

W = rowsum_form(1, 1, 0, 1)[2]          # rows per window of the windowed kernels, as the library reports it
SENTINEL = -1.2345e300                  # no sum of any palette comes near it
ISENTINEL = -1234567


def _spread(lo, hi, n):
    """n distinct ascending rows of [lo, hi), the first lo and the last hi - 1."""
    n = min(n, hi - lo)
    r = lo + (np.arange(n, dtype=np.int64) * (hi - lo)) // max(n, 1)
    if n > 1:
        r[-1] = hi - 1
    return r


def window_columns(nrow):
    """The rows of the twelve window columns (rows at or past nrow left out)."""
    last = ((nrow - 1) // W) * W                            # first row of the last window
    cols = [
        [],                                                 # 1  empty
        [0],                                                # 2
        [nrow - 1],                                         # 3
        [W - 1, W, 2 * W - 1, 2 * W],                       # 4  both sides of two window edges
        _spread(0, W, 64),                                  # 5  exactly one full chunk inside window 1, nothing after
        _spread(0, W, 63),                                  # 6
        _spread(0, W, 65),                                  # 7
        list(_spread(0, W, 128)) + [W + 5],                 # 8  two full chunks, then one value in window 2
        _spread(W, min(2 * W, nrow), 64),                   # 9  nothing in window 1
        np.arange(W - 100, W + 100),                        # 10 a run across the edge
        np.arange(nrow - 300, nrow),                        # 11 the last rows of the matrix
        _spread(last, nrow, 40),                            # 12 the last window only
    ]
    return [np.unique(np.asarray([r for r in c if 0 <= r < nrow], dtype=np.int64)) for c in cols]


LDS_LENGTHS = [0, 1, 255, 256, 257, 1000]                   # the 256-thread stride of rowsum_f64_lds_kernel
WAVE_LENGTHS = [0, 1, 63, 64, 65, 200]                      # the 64-lane stride of groupsum_atomic_kernel
PREPARED_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 600]    # four chunks of 64 in flight
ALL = ("tracer", "a", "d")

# form: what svt_dev_rowsum_form must answer (C: its cols_per_wg); fill = (columns, shortest, longest)
ROWSUM_CASES = {
    # ---- a workgroup per column, the int table (fewer than 65536 rows) ----
    "lds_table_g1": dict(form="lds_table", nrow=60000, ngroup=1, lengths=LDS_LENGTHS, fill=(10, 300, 500)),
    "lds_table_g3": dict(form="lds_table", nrow=60000, ngroup=3, lengths=LDS_LENGTHS, fill=(10, 300, 500),
                         variant="na_ends"),
    # nnz / ncol = 521 against ngroup / 4 = 250
    "lds_table_g1000": dict(form="lds_table", nrow=60000, ngroup=1000, lengths=LDS_LENGTHS, fill=(14, 900, 1100)),
    # 8192 groups, the full 64 KiB of the route's LDS limit, on 4 columns of at least 2048 nonzeros (no room for the
    # window columns: 4 columns is the case)
    "lds_table_g8192": dict(form="lds_table", nrow=60000, ngroup=8192, lengths=[2048, 2049, 3000, 2500], fill=(0, 0, 0),
                            window=False),
    # ---- the same behind the 16-bit table (65536 rows on) ----
    "lds_g16_63cols": dict(form="lds_g16", nrow=65536, ngroup=7, lengths=LDS_LENGTHS, fill=(45, 50, 150), ncol=63,
                           variant="na_ends"),
    # 5121 groups: 3 columns' accumulators per 160 KiB, fewer than the windowed kernel's 4; nnz / ncol ~ 1500 >= 1280
    "lds_g16_g5121": dict(form="lds_g16", nrow=65536, ngroup=5121, lengths=LDS_LENGTHS, fill=(48, 1800, 2200), ncol=66),
    # nnz / ncol ~ 2270 >= 2048
    "lds_g16_g8192": dict(form="lds_g16", nrow=65536, ngroup=8192, lengths=LDS_LENGTHS, fill=(46, 2900, 3300), ncol=64),
    # ---- windowed: 66 columns = 16 full workgroups of C = 4 and one whose last two wavefronts idle through the barriers ----
    "windowed_65536": dict(form="windowed", C=4, nrow=65536, ngroup=7, lengths=WAVE_LENGTHS, fill=(48, 50, 150), ncol=66),
    "windowed_2W": dict(form="windowed", C=4, nrow=2 * W, ngroup=7, lengths=WAVE_LENGTHS, fill=(48, 50, 150), ncol=66,
                        variant="na_ends"),
    "windowed_2W1": dict(form="windowed", C=4, nrow=2 * W + 1, ngroup=7, lengths=WAVE_LENGTHS, fill=(48, 50, 150), ncol=66),
    # 4 columns x 5120 groups x 8 bytes: the full 160 KiB
    "windowed_g5120": dict(form="windowed", C=4, nrow=2 * W + 1, ngroup=5120, lengths=WAVE_LENGTHS, fill=(48, 1800, 2200),
                           ncol=66),
    "windowed_1025cols": dict(form="windowed", C=5, nrow=65536, ngroup=7, lengths=WAVE_LENGTHS, fill=(1007, 20, 60),
                              ncol=1025, variant="na_ends"),
    "windowed_4000cols": dict(form="windowed", C=16, nrow=2 * W, ngroup=7, lengths=WAVE_LENGTHS, fill=(3982, 10, 40),
                              ncol=4000),
    # 16 columns x 1280 groups x 8 bytes: the full 160 KiB; nnz / ncol ~ 330 >= 320
    "windowed_4000cols_g1280": dict(form="windowed", C=16, nrow=65536, ngroup=1280, lengths=WAVE_LENGTHS,
                                    fill=(3982, 322, 338), ncol=4000, palettes=("tracer",)),
    # ---- memory atomics ----
    # one group more than the LDS kernels take, on columns long enough for them (nnz / ncol ~ 2300 >= 2048)
    "atomic_g8193": dict(form="atomic", nrow=65536, ngroup=8193, lengths=WAVE_LENGTHS, fill=(48, 2900, 3300), ncol=66,
                         variant="na_ends"),
    # columns one nonzero short of a quarter of the groups on average: nnz = 64 * 250 - 1
    "atomic_short": dict(form="atomic", nrow=65536, ngroup=1000, lengths=WAVE_LENGTHS, fill=(46, 200, 400), ncol=64,
                         nnz=64 * 250 - 1),
    # ---- the prepared sums (svt_dev_rowsum_prepared): C = 4, C = 1, C = 1 with the full 160 KiB ----
    "prepared_g5120": dict(form="atomic", nrow=21000, ngroup=5120, lengths=PREPARED_LENGTHS, fill=(4, 50, 150),
                           window=False, prepared_C=4),
    "prepared_g5121": dict(form="atomic", nrow=21000, ngroup=5121, lengths=PREPARED_LENGTHS, fill=(4, 50, 150),
                           window=False, prepared_C=1, variant="na_ends"),
    "prepared_g20480": dict(form="atomic", nrow=21000, ngroup=20480, lengths=PREPARED_LENGTHS, fill=(4, 50, 150),
                            window=False, prepared_C=1),
}
TALL = [n for n, s in ROWSUM_CASES.items() if s["nrow"] >= 65536]
ROWSUM_PARAMS = [(n, p) for n, s in ROWSUM_CASES.items() for p in s.get("palettes", ALL)]

# Operands that differ by one step and take different forms: (case whose operand is run, the parameter stepped, its
# other value, the form there).  Asserted through the query alone.
BOUNDARY_PAIRS = [
    ("windowed_65536", "nrow", 65535, "lds_table"),
    ("lds_g16_63cols", "ncol", 64, "windowed"),
    ("windowed_g5120", "ngroup", 5121, "lds_g16"),
    ("lds_g16_g5121", "ngroup", 5120, "windowed"),
    ("lds_g16_g8192", "ngroup", 8193, "atomic"),
    ("atomic_g8193", "ngroup", 8192, "lds_g16"),
    ("atomic_short", "nnz", 64 * 250, "windowed"),
]


def _random_rows(rng, nrow, n):
    return np.sort(rng.choice(nrow, size=n, replace=False, shuffle=False)).astype(np.int64)


def build_groups(rng, n, ngroup, variant, special=()):
    """(slot, na): ``slot`` 0-based with every slot taken, ``na`` the elements that carry NA (all in the last slot).
    ``special``: the elements that variant "distinct" puts into pairwise different slots (as far as ngroup allows) and
    of which "na_ends" puts the first and the last into the NA group."""
    slot = rng.integers(0, ngroup, n)
    na = rng.random(n) < 1e-3
    special = list(dict.fromkeys(int(r) for r in special))
    free = np.setdiff1d(np.arange(n), special)
    taken = rng.choice(free, size=min(ngroup, len(free)), replace=False)
    slot[taken] = np.arange(len(taken))                     # every slot occurs (the callers keep ngroup <= len(free))
    na[taken] = False
    spare = np.setdiff1d(free, taken)
    if len(spare):
        na[rng.choice(spare)] = True                        # at least one NA
    slot[na] = ngroup - 1
    if variant == "distinct":
        for k, r in enumerate(special):
            slot[r], na[r] = k % max(ngroup - 1, 1), False  # (not the NA slot, while there is another)
    else:
        for r in special[1:-1]:
            na[r] = False
        for r in (special[0], special[-1]):
            slot[r], na[r] = ngroup - 1, True
    return slot.astype(np.int64), na


def device_group(slot, na):
    """The int32 ids the C entry points take: 1-based, NA_integer where ``na``."""
    g = (slot + 1).astype(np.int32)
    g[na] = NA_integer
    return g


@functools.lru_cache(maxsize=None)
def rowsum_layout(name):
    spec = ROWSUM_CASES[name]
    rng = np.random.default_rng(5000 + sorted(ROWSUM_CASES).index(name))
    nrow, ngroup = spec["nrow"], spec["ngroup"]
    cols = window_columns(nrow) if spec.get("window", True) else []
    cols += [_random_rows(rng, nrow, n) for n in spec["lengths"]]
    nfill, lo, hi = spec["fill"]
    fill = [int(n) for n in rng.integers(lo, hi + 1, nfill)]
    if "nnz" in spec:                                       # an exact total: the last fill column takes the difference
        fill[-1] += spec["nnz"] - (sum(len(c) for c in cols) + sum(fill))
        assert 0 < fill[-1] < nrow
    cols += [_random_rows(rng, nrow, n) for n in fill]
    c = Case()
    c.name, c.spec, c.form, c.C = name, spec, spec["form"], spec.get("C", 0)
    c.nrow, c.ncol, c.ngroup = nrow, len(cols), ngroup
    assert c.ncol == spec.get("ncol", c.ncol), f"{name}: {c.ncol} columns"
    c.lengths = np.array([len(r) for r in cols], dtype=np.int64)
    c.col_ptr = np.concatenate([[0], np.cumsum(c.lengths)]).astype(np.int64)
    c.row_idx = np.concatenate(cols).astype(np.int32)
    c.nnz = len(c.row_idx)
    assert c.nnz == spec.get("nnz", c.nnz)
    c.col = np.repeat(np.arange(c.ncol, dtype=np.int64), c.lengths)
    c.variant = spec.get("variant", "distinct")
    c.slot, c.na = build_groups(rng, nrow, ngroup, c.variant, special=(0, W - 1, W, nrow - 1) if nrow > W else (0, nrow - 1))
    c.group32 = device_group(c.slot, c.na)
    c.cell = c.slot[c.row_idx] + ngroup * c.col             # cell (g, j) = g + ngroup * j
    # the R level: every row of the last slot is NA (None); the sorted unique groups are then 0 .. ngroup - 2, None
    c.r_group = [None if s == ngroup - 1 else int(s) for s in c.slot]
    # column groups for colsum() of the same operand: 5 groups, the last one NA
    c.cslot, c.cna = build_groups(rng, c.ncol, min(5, c.ncol), "distinct")
    c.ncgroup = min(5, c.ncol)
    c.cgroup32 = device_group(c.cslot, c.cna)
    c.ccell = c.row_idx.astype(np.int64) + nrow * c.cslot[c.col]      # cell (i, g) = i + nrow * g
    return c


def assert_rowsum_form(c, type="double", col_ptr32=False):
    """The case takes the form it is named after, with the columns per workgroup it names; returns the form."""
    form, C, win = rowsum_form(c.nrow, c.ncol, c.nnz, c.ngroup, type, col_ptr32)
    want = c.form if type == "double" and not col_ptr32 else "atomic"
    assert win == W
    assert (form, C) == (want, c.C if want == "windowed" else 0), f"{c.name}: takes {form} with C = {C}, not {want} / {c.C}"
    if want == "windowed":
        assert C * c.ngroup * 8 <= 160 * 1024
        if c.name in ("windowed_g5120", "windowed_4000cols_g1280"):
            assert C * c.ngroup * 8 == 160 * 1024, f"{c.name}: not the full LDS"
        if c.ncol == 66:
            assert c.ncol % C == 2                          # the last workgroup holds two columns: two wavefronts idle
    if c.nrow > W:
        assert c.spec.get("window", True) is False or (c.lengths[4:9] == [64, 63, 65, 129, 64]).all()
    assert np.array_equal(np.unique(c.slot), np.arange(c.ngroup)), f"{c.name}: a group without a row"
    assert c.na.any() and (c.slot[c.na] == c.ngroup - 1).all()
    if c.nrow > W:
        ends = [0, W - 1, W, c.nrow - 1]
        if c.variant == "distinct":
            assert len(set(c.slot[ends])) == min(4, max(c.ngroup - 1, 1)) and not c.na[ends].any()
        else:
            assert c.na[0] and c.na[c.nrow - 1]
    return form


def assert_boundary_pair(name, param, other, form_there):
    c = rowsum_layout(name)
    here = dict(nrow=c.nrow, ncol=c.ncol, nnz=c.nnz, ngroup=c.ngroup)
    assert abs(here[param] - other) == 1
    assert rowsum_form(**here)[0] == c.form
    there = dict(here, **{param: other})
    assert rowsum_form(**there)[0] == form_there, f"{name} with {param} = {other}: {rowsum_form(**there)[0]}, not {form_there}"
    assert form_there != c.form


@functools.lru_cache(maxsize=None)
def case_values(key, n, palette):
    """The values of an operand of n nonzeros (``key``: the case's name): doubles, or int32 for "itracer"."""
    rng = np.random.default_rng(sum(map(ord, key + palette)) + 11)
    if palette in ("tracer", "itracer"):
        v = rng.integers(1, 2 ** 20 + 1, n) * rng.choice([-1, 1], n)
        if palette == "tracer":
            return v.astype(np.float64)
        v = v.astype(np.int32)
        v[rng.choice(n, 2, replace=False)] = NA_integer
        return v
    v, _ = palette_values(palette, n, rng)
    if palette == "a":
        v[rng.choice(n, 4, replace=False)] = [NA_real, np.nan, NA_real, np.nan]
    return v


def planted(palette):
    return palette in ("a", "itracer")


class Expect:
    """What every cell of a rowsum / colsum result must be: ``vals`` the stored values, ``cell`` the cell of each."""

    def __init__(self, vals, cell, ncell, na_rm, exact):
        vals, cell = np.asarray(vals), np.asarray(cell, dtype=np.int64)
        self.ncell, self.na_rm, self.is_int = int(ncell), bool(na_rm), vals.dtype != np.float64
        miss = (vals == NA_integer) if self.is_int else np.isnan(vals)
        take = ~miss
        self.stored = np.bincount(cell, minlength=ncell)
        self.poisoned = np.zeros(ncell, dtype=bool)
        if not na_rm:
            self.poisoned[cell[miss]] = True
        # cells with one stored value that takes part: the result is that value
        k = np.flatnonzero(take & (self.stored[cell] == 1))
        self.one_cell, self.one_val = cell[k], vals[k]
        self.total = None
        self.cells = None
        if exact:                                           # integer-valued: int64 totals
            self.total = np.zeros(ncell, dtype=np.int64)
            np.add.at(self.total, cell[take], vals[take].astype(np.int64))
            assert np.abs(self.total).max(initial=0) < 2 ** (31 if self.is_int else 53)
        else:                                               # the cells of two or more stored values, renumbered
            self.multi = np.flatnonzero(self.stored >= 2)
            new_id = np.full(ncell, -1, dtype=np.int64)
            new_id[self.multi] = np.arange(len(self.multi))
            sel = new_id[cell] >= 0
            self.cells = ex.Cells(vals[sel], new_id[cell[sel]], len(self.multi), self.stored[self.multi], na_rm)

    def check(self, got, what="", max_poisoned=4):
        """Every cell of ``got`` (flat, cell order).  Returns the worst err / bound (0 for the exact palettes)."""
        got = np.ascontiguousarray(np.asarray(got).reshape(-1))
        assert got.shape == (self.ncell,), f"{what}: {got.shape} cells, not {self.ncell}"
        assert not np.any(got == (ISENTINEL if self.is_int else SENTINEL)), f"{what}: a cell was not written"
        npois = int(self.poisoned.sum())
        assert npois <= max_poisoned, f"{what}: {npois} cells compared by class"
        ok = ~self.poisoned
        if self.is_int:
            assert got.dtype == np.int32
            want = np.where(self.poisoned, NA_integer, self.total)
            assert np.array_equal(got.astype(np.int64), want), f"{what}: integer sums differ"
            return 0.0
        assert got.dtype == np.float64
        bits = got.view(np.uint64)
        assert np.all(np.isnan(got[self.poisoned])), f"{what}: a cell with a missing value and na.rm=FALSE is not NaN"
        # no value takes part: no stored value, or one that na.rm removed
        zero = (self.stored <= 1) & ok
        zero[self.one_cell] = False
        assert np.all(bits[zero] == 0), f"{what}: a cell without a value is not +0.0"
        assert np.array_equal(bits[self.one_cell], self.one_val.view(np.uint64)), \
            f"{what}: a cell with one value is not that value"
        ncompared = int(zero.sum()) + len(self.one_cell)
        if self.total is not None:
            rest = ok & (self.stored >= 2)
            assert np.array_equal(got[rest], self.total[rest].astype(np.float64)), f"{what}: a sum differs from the exact total"
            assert not np.any(np.signbit(got[rest]) & (got[rest] == 0)), f"{what}: -0.0"
            ncompared += int(rest.sum())
            worst = 0.0
        else:
            v = ex.check_sum(got[self.multi], self.cells, what).require()
            ncompared += v.ncompared
            worst = v.worst
        assert ncompared == self.ncell - npois, f"{what}: {self.ncell - npois - ncompared} cells left out"
        return worst


@functools.lru_cache(maxsize=None)
def rowsum_expect(name, palette, na_rm):
    c = rowsum_layout(name)
    return Expect(case_values(name, c.nnz, palette), c.cell, c.ngroup * c.ncol, na_rm, palette.endswith("tracer"))


@functools.lru_cache(maxsize=None)
def colsum_expect(name, palette, na_rm):
    """colsum() of a rowsum case's operand by its 5 column groups."""
    c = rowsum_layout(name)
    return Expect(case_values(name, c.nnz, palette), c.ccell, c.nrow * c.ncgroup, na_rm, palette.endswith("tracer"))


@functools.lru_cache(maxsize=None)
def case_svt(name, palette):
    c = rowsum_layout(name)
    v = case_values(name, c.nnz, palette)
    return SVT_SparseArray.from_csc((c.nrow, c.ncol), "integer" if v.dtype == np.int32 else "double", c.col_ptr, c.row_idx, v)


# ---------------------------------------------------------------------------
# the host entry points, called with an output of the test's own
# ---------------------------------------------------------------------------
def call_xsum(sess, entry, x, group32, ngroup, na_rm, ncell):
    """svt_rowsum_SVT / svt_colsum_SVT (or the checker's) into a sentinel-filled buffer; returns it flat."""
    d = sess._call
    is_int = x.type == "integer"
    out = np.full(ncell, ISENTINEL if is_int else SENTINEL, dtype=np.int32 if is_int else np.float64)
    g = np.ascontiguousarray(group32, dtype=np.int32)
    ov = c_int(0)
    xv = make_view(x)
    d._check(d._fn(entry)(byref(xv), _ptr(g), int(ngroup), int(na_rm), _ptr(out), byref(ov)))
    assert ov.value == 0
    return out


def call_dgc(sess, entry, c, val, group32, ngroup, na_rm, ncell):
    """svt_rowsum_dgCMatrix / svt_colsum_dgCMatrix on the CSC arrays of ``c`` with an int32 'p' slot."""
    d = sess._call
    out = np.full(ncell, SENTINEL)
    p, i = c.col_ptr.astype(np.int32), np.ascontiguousarray(c.row_idx, dtype=np.int32)
    xx, g = np.ascontiguousarray(val, dtype=np.float64), np.ascontiguousarray(group32, dtype=np.int32)
    d._check(d._fn(entry)(int(c.nrow), int(c.ncol), _ptr(xx), _ptr(i), _ptr(p), _ptr(g), int(ngroup), int(na_rm), _ptr(out)))
    return out


def _note(rec, key, worst):
    if rec is not None:
        rec[key] = max(rec.get(key, 0.0), worst)


def na_rms(palette):
    return (False, True) if planted(palette) else (False,)


def run_rowsum_case(sess, name, palette, rec=None, who=""):
    """svt_rowsum_SVT on the case with NA_integer, and rowsum() of the R level with ``None``, for the NA group."""
    c = rowsum_layout(name)
    form = assert_rowsum_form(c)
    x = case_svt(name, palette)
    for na_rm in na_rms(palette):
        e = rowsum_expect(name, palette, na_rm)
        got = call_xsum(sess, "rowsum_SVT", x, c.group32, c.ngroup, na_rm, e.ncell)
        _note(rec, (who, "rowsum_SVT", form), e.check(got, f"{name}/{palette} rowsum_SVT na_rm={na_rm}"))
        # the R level: rowsum() with None for the NA group (its result is the dispatcher's own array)
        got, ug = sess.rowsum(x, c.r_group, na_rm=na_rm)
        assert ug == list(range(c.ngroup - 1)) + [None]
        _note(rec, (who, "rowsum_SVT", form), e.check(np.asarray(got).reshape(-1, order="F"),
                                                      f"{name}/{palette} rowsum() with None na_rm={na_rm}"))


def run_dgc_case(sess, name, palette, rec=None, who=""):
    """svt_rowsum_dgCMatrix and svt_colsum_dgCMatrix on the same operand: the atomic form, by the int32 offsets."""
    c = rowsum_layout(name)
    assert_rowsum_form(c, col_ptr32=True)
    val = case_values(name, c.nnz, palette)
    for na_rm in na_rms(palette):
        e = rowsum_expect(name, palette, na_rm)
        got = call_dgc(sess, "rowsum_dgCMatrix", c, val, c.group32, c.ngroup, na_rm, e.ncell)
        _note(rec, (who, "rowsum_dgCMatrix", "atomic"), e.check(got, f"{name}/{palette} rowsum_dgCMatrix na_rm={na_rm}"))
        e = colsum_expect(name, palette, na_rm)
        got = call_dgc(sess, "colsum_dgCMatrix", c, val, c.cgroup32, c.ncgroup, na_rm, e.ncell)
        _note(rec, (who, "colsum_dgCMatrix", "atomic"), e.check(got, f"{name}/{palette} colsum_dgCMatrix na_rm={na_rm}"))


def run_int_rowsum_case(sess, oracle, name):
    """Integer rowsum: atomic by type; the int64 totals, and the reference's result."""
    c = rowsum_layout(name)
    assert_rowsum_form(c, type="integer")
    x = case_svt(name, "itracer")
    for na_rm in (False, True):
        e = rowsum_expect(name, "itracer", na_rm)
        got = call_xsum(sess, "rowsum_SVT", x, c.group32, c.ngroup, na_rm, e.ncell)
        e.check(got, f"{name} integer rowsum na_rm={na_rm}", max_poisoned=2)
        if oracle is not None and oracle is not sess:
            assert np.array_equal(got, call_xsum(oracle, "rowsum_SVT", x, c.group32, c.ngroup, na_rm, e.ncell))


# ---------------------------------------------------------------------------
# colsum: 300 x 200, column lengths around 64 (the lanes of the wavefront that walks a column)
# ---------------------------------------------------------------------------
COLSUM_NGROUPS = (1, 40)
COLSUM_PALETTES = ("tracer", "a", "d", "itracer")


@functools.lru_cache(maxsize=None)
def colsum_layout(ngroup):
    rng = np.random.default_rng(7000 + ngroup)
    nrow, ncol = 300, 200
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 300] + [int(n) for n in rng.integers(56, 73, ncol - 9)]
    cols = [_random_rows(rng, nrow, n) for n in lengths]
    c = Case()
    c.name, c.nrow, c.ncol, c.ngroup = f"colsum_g{ngroup}", nrow, ncol, ngroup
    c.lengths = np.array(lengths, dtype=np.int64)
    c.col_ptr = np.concatenate([[0], np.cumsum(c.lengths)]).astype(np.int64)
    c.row_idx = np.concatenate(cols).astype(np.int32)
    c.nnz = len(c.row_idx)
    c.col = np.repeat(np.arange(ncol, dtype=np.int64), c.lengths)
    c.cslot, c.cna = build_groups(rng, ncol, ngroup, "distinct")
    c.empty_group = None
    if ngroup > 2:                                          # one group without any column: its cells are +0.0 (or 0)
        c.empty_group = 17 % (ngroup - 1)
        move = (c.cslot == c.empty_group)
        c.cslot[move] = (c.empty_group + 1) % (ngroup - 1)
    c.cgroup32 = device_group(c.cslot, c.cna)
    c.ccell = c.row_idx.astype(np.int64) + nrow * c.cslot[c.col]
    return c


@functools.lru_cache(maxsize=None)
def colsum_case_expect(ngroup, palette, na_rm):
    c = colsum_layout(ngroup)
    return Expect(case_values(c.name, c.nnz, palette), c.ccell, c.nrow * ngroup, na_rm, palette.endswith("tracer"))


def run_colsum_case(sess, ngroup, palette, rec=None, who="", oracle=None):
    c = colsum_layout(ngroup)
    assert c.cna.any() and (c.cslot[c.cna] == ngroup - 1).all()
    assert {0, 1, 63, 64, 65} <= set(c.lengths.tolist())
    if ngroup > 2:
        assert not (c.cslot == c.empty_group).any()
    v = case_values(c.name, c.nnz, palette)
    x = SVT_SparseArray.from_csc((c.nrow, c.ncol), "integer" if v.dtype == np.int32 else "double", c.col_ptr, c.row_idx, v)
    for na_rm in na_rms(palette):
        e = colsum_case_expect(ngroup, palette, na_rm)
        got = call_xsum(sess, "colsum_SVT", x, c.cgroup32, ngroup, na_rm, e.ncell)
        _note(rec, (who, "colsum_SVT", "atomic"), e.check(got, f"{c.name}/{palette} colsum_SVT na_rm={na_rm}",
                                                          max_poisoned=4 if palette == "a" else 2))
        if ngroup > 2:                                      # the group without a column: written, and +0.0 / 0
            blk = got[c.empty_group * c.nrow:(c.empty_group + 1) * c.nrow]
            assert not blk.any() and not np.signbit(blk.astype(np.float64)).any()
        if palette == "itracer" and oracle is not None and oracle is not sess:
            assert np.array_equal(got, call_xsum(oracle, "colsum_SVT", x, c.cgroup32, ngroup, na_rm, e.ncell))


# ---------------------------------------------------------------------------
# the prepared form
# ---------------------------------------------------------------------------
def expected_ids(c):
    """The 16-bit id of every nonzero: slot(group[row_idx[k]])."""
    return c.slot[c.row_idx].astype(np.uint16)


def assert_prepare_form(c, nnz=None):
    """(form, C) of svt_dev_rowsum_prepare for the case: windowed from 65536 rows and 64 columns on."""
    form, C = rowsum_prepare_form(c.nrow, c.ncol, c.nnz if nnz is None else nnz, c.ngroup)
    want = "windowed" if c.nrow >= 65536 and c.ncol >= 64 else "flat"
    assert form == want, f"{c.name}: the ids take {form}, not {want}"
    if form == "windowed":
        assert C == {64: 8, 66: 8, 1025: 8, 4000: 16}[c.ncol], f"{c.name}: ids with C = {C}"
    else:
        assert C == 0
    return form, C


def assert_prepared_form(c):
    """C of svt_dev_rowsum_prepared for the case; the cases named prepared_* state theirs."""
    ok, C = rowsum_prepared_form(c.ncol, c.ngroup)
    assert ok and 1 <= C <= 16 and C * c.ngroup * 8 <= 160 * 1024
    if "prepared_C" in c.spec:
        assert C == c.spec["prepared_C"], f"{c.name}: prepared with C = {C}"
    if c.name == "prepared_g20480":
        assert C * c.ngroup * 8 == 160 * 1024
    return C
