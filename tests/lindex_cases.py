"""Operands, indices and values for subsetting and subassignment by a linear index (L-index) or a matrix subscript
(M-index): DeviceCSC.subset_lindex / subset_mindex / subassign_lindex / subassign_mindex and Session.subset_by_Lindex /
... (.subset_SVT_by_Lindex, R/SparseArray-subsetting.R; .subassign_SVT_by_Lindex, R/SparseArray-subassignment.R;
subassign_leaf_by_OPBuf, src/SparseArray_subassignment.c), shared by tests/test_zzzzz_lindex_cpu.py and
tests/test_zzzzz_lindex_hip.py.

An operand is its cells: the sorted 0-based cell numbers of the STORED entries of the column-major array (cell = row +
nrow * leaf) and their values.  The expectation is numpy's on the dense column-major array:

  subsetting     ``dense.ravel(order="F")[L]``, NA for an NA index;
  subassignment  an explicit loop over the positions p -- ``flat[L[p]] = value[p % len(value)]`` after widening to the
                 result's type (the wider of logical < integer < double; NA_integer_ becomes NA_real_) -- so it does not
                 lean on what numpy does with repeats: the last occurrence of a cell wins;
  stored mask    an assigned cell is stored iff its final value is not zero (a NaN or NA is stored, -0.0 and 0 are not);
                 every other cell keeps x's own mask, a stored zero of x included.

``dense_*`` state that on the dense array and its mask, for operands small enough to have one; ``expect_*`` state the
same on the cells alone (an array of 70000 x 70000 has no dense form here), and tests/test_zzzzz_lindex_cpu.py holds the
two against each other wherever both exist.  Everything is compared at tolerance 0: the values AS BITS
(subset_cases.bits) and the stored cells.

The shapes are the smallest that reach each branch of the device code: S = 2048 keys per tile of the sort (svt_sort.h),
4096 elements per tile of the scan (svt_scan.h), T = 2048 merged places per tile of the merge (kernels_arith.hip), one
8-bit pass of the sort per started byte of ncells - 1.
"""
from __future__ import annotations

import functools

import numpy as np

from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from subset_cases import NP_DTYPE, SPECIALS_F64, SPECIALS_I32, SPECIALS_LGL, bits

S = 2048            # keys per tile of the sort
SCAN = 4096         # elements per tile of the scan
T = 2048            # merged places per tile of the merge
TYPE_ORDER = ("logical", "integer", "double")
LINDEX_NA = -2 ** 63
NAN_PAYLOAD = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
MINUS_ZERO = np.array([0x8000000000000000], dtype=np.uint64).view(np.float64)[0]


def wider(t1, t2):
    return max(t1, t2, key=TYPE_ORDER.index)


def widen(a, from_type, to_type):
    """values of ``from_type`` in the dtype of ``to_type``: the same bits, or int32 -> double with NA_integer_ -> NA_real_"""
    a = np.asarray(a, dtype=NP_DTYPE[from_type])
    if NP_DTYPE[to_type] == NP_DTYPE[from_type]:
        return a.copy()
    out = a.astype(np.float64)
    out[a == NA_integer] = NA_real
    return out


def na_of(type_):
    return NA_real if type_ == "double" else NA_integer


class Operand:
    """dim, type, the sorted cells of the stored entries and their values; ``na_background``: an NaArray"""

    def __init__(self, dim, type_, cells, vals, na_background=False):
        self.dim, self.type, self.na_background = tuple(int(d) for d in dim), type_, na_background
        self.nrow = self.dim[0]
        self.ncol = int(np.prod(self.dim[1:], dtype=object)) if len(self.dim) > 1 else 1
        self.ncells = self.nrow * self.ncol
        self.cells = np.asarray(cells, dtype=np.int64)
        self.vals = np.asarray(vals, dtype=NP_DTYPE[type_])
        assert self.cells.shape == self.vals.shape and (np.diff(self.cells) > 0).all()
        assert self.cells.size == 0 or (0 <= self.cells[0] and self.cells[-1] < self.ncells)

    def csc(self):
        """(col_ptr int64[ncol + 1], row_idx int32, val) of the device layout"""
        leaf = self.cells // self.nrow
        col_ptr = np.searchsorted(leaf, np.arange(self.ncol + 1, dtype=np.int64)).astype(np.int64)
        return col_ptr, (self.cells - leaf * self.nrow).astype(np.int32), self.vals

    def svt(self):
        """the host object (leaves: the outermost dimension slowest)"""
        cp, ri, vv = self.csc()
        x = SVT_SparseArray.from_csc(self.dim, self.type, cp, ri, vv)
        x.na_background = self.na_background
        return x

    @property
    def has_dense(self):
        return self.ncells <= 1 << 22


def tracer(type_, cells):
    """values that encode the cell, never 0 and never NA"""
    cells = np.asarray(cells, dtype=np.int64)
    if type_ == "double":
        return (cells % 1000003).astype(np.float64) + 1.25
    if type_ == "integer":
        return (cells % 1000003 + 1).astype(np.int32)
    return np.ones(cells.size, dtype=np.int32)


def specials(type_, n):
    table = {"double": SPECIALS_F64, "integer": SPECIALS_I32, "logical": SPECIALS_LGL}[type_]
    return table[np.arange(n) % table.size]


def random_cells(ncells, n, seed):
    return np.sort(np.random.default_rng(seed).choice(ncells, size=n, replace=False)).astype(np.int64)


def mindex_of(dim, L):
    """the 0-based coordinate rows (K, ndim) int32 of the 0-based cells L"""
    L = np.asarray(L, dtype=np.int64)
    out = np.zeros((L.size, len(dim)), dtype=np.int32)
    for a, d in enumerate(dim):
        out[:, a] = L % d
        L = L // d
    return out


# ---------------------------------------------------------------------------
# the expectation on the dense column-major array
# ---------------------------------------------------------------------------
def dense_and_stored(op):
    """(flat column-major values with the background filled in, flat mask of the stored cells)"""
    assert op.has_dense
    flat = np.zeros(op.ncells, dtype=NP_DTYPE[op.type])
    if op.na_background:
        flat[:] = na_of(op.type)
    stored = np.zeros(op.ncells, dtype=bool)
    flat[op.cells] = op.vals
    stored[op.cells] = True
    return flat, stored


def dense_subset(op, L):
    flat, _ = dense_and_stored(op)
    L = np.asarray(L, dtype=np.int64)
    na = L == LINDEX_NA
    out = flat[np.where(na, 0, L)]
    out[na] = na_of(op.type)
    return out


def dense_subassign(op, L, value, v_type):
    """(the result's type, flat values, flat stored mask) by a loop over the positions"""
    new_type = wider(op.type, v_type)
    flat, stored = dense_and_stored(op)
    flat = widen(flat, op.type, new_type)
    v = widen(value, v_type, new_type)
    touched = {}
    for p, cell in enumerate(np.asarray(L, dtype=np.int64).tolist()):
        flat[cell] = v[p % v.size]
        touched[cell] = True
    for cell in touched:
        stored[cell] = not (flat[cell] == 0)            # a NaN is != 0: stored
        if not stored[cell]:
            flat[cell] = 0                                  # a cell that is not stored reads +0
    return new_type, flat, stored


# ---------------------------------------------------------------------------
# the same on the cells alone
# ---------------------------------------------------------------------------
def expect_subset(op, L):
    L = np.asarray(L, dtype=np.int64)
    na = L == LINDEX_NA
    out = np.zeros(L.size, dtype=NP_DTYPE[op.type])
    if op.na_background:
        out[:] = na_of(op.type)
    pos = np.searchsorted(op.cells, L)
    hit = ~na & (pos < op.cells.size)
    hit[hit] = op.cells[pos[hit]] == L[hit]
    out[hit] = op.vals[pos[hit]]
    out[na] = na_of(op.type)
    return out


def expect_subassign(op, L, value, v_type):
    """(the result's type, the sorted stored cells, their values)"""
    new_type = wider(op.type, v_type)
    v = widen(value, v_type, new_type)
    L = np.asarray(L, dtype=np.int64)
    # the last position of every assigned cell: a stable sort keeps the positions of a cell in order
    order = np.argsort(L, kind="stable")
    sl = L[order]
    last = np.ones(sl.size, dtype=bool)
    last[:-1] = sl[1:] != sl[:-1]
    a_cells, a_vals = sl[last], v[order[last] % v.size]
    keep_x = ~np.isin(op.cells, a_cells)
    keep_a = ~(a_vals == 0)
    cells = np.concatenate([op.cells[keep_x], a_cells[keep_a]])
    vals = np.concatenate([widen(op.vals, op.type, new_type)[keep_x], a_vals[keep_a]])
    o = np.argsort(cells, kind="stable")
    return new_type, cells[o], vals[o]


def same_as_dense(cells, vals, flat, stored):
    return np.array_equal(np.flatnonzero(stored), cells) and np.array_equal(bits(flat[cells]), bits(vals))


# ---------------------------------------------------------------------------
# gather cases: name -> (operand, L 0-based with LINDEX_NA)
# ---------------------------------------------------------------------------
COLUMN_LENGTHS = (0, 1, 2, 3, 64, 65, 5000, 0)


@functools.lru_cache(maxsize=None)
def column_lengths_operand(type_="double", na_background=False):
    """6000 rows; column c holds COLUMN_LENGTHS[c] entries on rows 7, 7 + step, ... (first stored row 7, so that a row
    below the first exists; the last stored row below 5999, so that one above it does)"""
    nrow, cells = 6000, []
    for c, n in enumerate(COLUMN_LENGTHS):
        rows = 7 + np.arange(n, dtype=np.int64) * (1 if n == 5000 else 11)
        cells.append(c * nrow + rows)
    cells = np.concatenate(cells)
    return Operand((nrow, len(COLUMN_LENGTHS)), type_, cells, tracer(type_, cells), na_background)


def column_edge_queries(op):
    """per column: the first and the last stored row, one below the first, one above the last; rows 0 and nrow - 1 of
    every column, the empty ones included"""
    cp, ri, _ = op.csc()
    out = []
    for c in range(op.ncol):
        rows = ri[cp[c]:cp[c + 1]].astype(np.int64)
        q = [0, op.nrow - 1]
        if rows.size:
            q += [rows[0], rows[-1], rows[0] - 1, rows[-1] + 1, rows[rows.size // 2], rows[rows.size // 2] + 1]
        out.append(c * op.nrow + np.unique(np.clip(np.array(q, dtype=np.int64), 0, op.nrow - 1)))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def specials_operand(type_):
    """37 x 23 with the type's special values stored: for a double NA_real_, a NaN payload, +-Inf, a stored -0.0, a
    stored 0.0"""
    cells = random_cells(37 * 23, 200, {"double": 2, "integer": 3, "logical": 4}[type_])
    return Operand((37, 23), type_, cells, specials(type_, cells.size))


@functools.lru_cache(maxsize=None)
def huge_operand():
    """70000 x 70000 (4.9e9 cells, past 2^32) with a handful of entries, one of them past cell 2^32"""
    n = 70000
    cells = np.array([5, n * 3 + 69999, n * 40000 + 12345, 2 ** 32 + 17, n * 69999 + 69999], dtype=np.int64)
    assert cells[3] > 2 ** 32 and n * n > 2 ** 32
    return Operand((n, n), "double", np.sort(cells), tracer("double", np.sort(cells)))


@functools.lru_cache(maxsize=None)
def three_d_operand(type_="double"):
    cells = random_cells(11 * 7 * 5, 120, 8)
    return Operand((11, 7, 5), type_, cells, tracer(type_, cells))


def _gather_cases():
    op = column_lengths_operand()
    edges = column_edge_queries(op)
    rng = np.random.default_rng(11)
    sp = specials_operand("double")
    huge = huge_operand()
    near = np.concatenate([huge.cells, huge.cells + 1, huge.cells - 1, [0, huge.ncells - 1, 2 ** 32, 2 ** 32 - 1]])
    d3 = three_d_operand()
    return {
        "column_edges": (op, edges),
        "column_edges_shuffled_with_repeats": (op, rng.permutation(np.concatenate([edges, edges[::3]]))),
        "every_stored_cell": (op, op.cells),
        "NA_indices": (op, np.array([LINDEX_NA, 7, LINDEX_NA, op.cells[-1], LINDEX_NA], dtype=np.int64)),
        "only_NA": (op, np.full(3, LINDEX_NA, dtype=np.int64)),
        "K_0": (op, np.zeros(0, dtype=np.int64)),
        "K_past_one_block": (op, rng.integers(0, op.ncells, 1000)),
        "specials_double_every_cell": (sp, np.arange(sp.ncells, dtype=np.int64)),
        "specials_integer_every_cell": (specials_operand("integer"), np.arange(37 * 23, dtype=np.int64)[::-1]),
        "specials_logical": (specials_operand("logical"), rng.integers(0, 37 * 23, 300)),
        "na_background_double": (column_lengths_operand("double", True), np.concatenate([edges, [LINDEX_NA]])),
        "na_background_integer": (column_lengths_operand("integer", True), edges),
        "past_2_32_cells": (huge, near[(near >= 0) & (near < huge.ncells)]),
        "three_d": (d3, rng.integers(0, d3.ncells, 400)),
        "empty_operand": (Operand((9, 4), "double", [], []), np.arange(36, dtype=np.int64)),
    }


GATHER = _gather_cases()
GATHER_NAMES = list(GATHER)


# ---------------------------------------------------------------------------
# subassignment cases: name -> (operand, L 0-based, value, value type)
# ---------------------------------------------------------------------------
def _vec(type_, n, seed, zeros=0.0):
    rng = np.random.default_rng(seed)
    if type_ == "double":
        v = rng.integers(1, 50, n).astype(np.float64) / 4 * rng.choice([-1.0, 1.0], n)
    elif type_ == "integer":
        v = (rng.integers(1, 50, n) * rng.choice([-1, 1], n)).astype(np.int32)
    else:
        v = np.ones(n, dtype=np.int32)
    if zeros:
        v[rng.random(n) < zeros] = 0
    return v


def _unsorted_K(K):
    """K indices with repeats and no order over 300 x 40 (two passes), values with zeros"""
    def f():
        cells = random_cells(12000, 900, 20)
        op = Operand((300, 40), "double", cells, tracer("double", cells))
        L = np.random.default_rng(21 + K).integers(0, 12000, K)
        return op, L, _vec("double", K, 22, zeros=0.3), "double"
    return f


def _passes(dim, seed):
    def f():
        ncells = int(np.prod(dim, dtype=object))
        rng = np.random.default_rng(seed)
        cells = np.unique(rng.integers(0, ncells, 60))
        op = Operand(dim, "double", cells, tracer("double", cells))
        L = np.concatenate([rng.integers(0, ncells, 150), cells[::2], [ncells - 1, 0, ncells - 1]])
        return op, rng.permutation(L), _vec("double", L.size, seed + 1, zeros=0.25), "double"
    return f


def _run_of_5000(last):
    """1000 smaller cells, 5000 repeats of one cell, 1000 larger ones, shuffled: the run of equal keys covers sorted
    places 1000 .. 5999 -- across the sort tiles' edges at 2048 and 4096 and the scan tile's at 4096"""
    def f():
        ncells = 300 * 40
        cells = random_cells(ncells, 500, 30)
        op = Operand((300, 40), "double", cells, tracer("double", cells))
        c = 6000
        others = np.concatenate([np.arange(0, 2000, 2), np.arange(7000, 9000, 2)])
        rng = np.random.default_rng(31)
        L = rng.permutation(np.concatenate([others, np.full(5000, c)]))
        v = _vec("double", L.size, 32)
        v[np.flatnonzero(L == c)[-1]] = last
        return op, L, v, "double"
    return f


def _v_0_w():
    cells = np.array([3, 17, 40], dtype=np.int64)
    op = Operand((10, 6), "double", cells, tracer("double", cells))
    #      cell 17: v, 0, w  -> w;  cell 3: v, 0 -> deleted;  cell 5 (not stored): 0, w, 0 -> nothing;  cell 6: 0, w -> w
    L = np.array([17, 3, 5, 17, 6, 5, 3, 17, 5, 6], dtype=np.int64)
    v = np.array([1.5, 2.5, 0.0, 0.0, 0.0, 7.0, 0.0, -3.0, 0.0, 9.0])
    return op, L, v, "double"


def _one_per_leaf(shuffled):
    def f():
        dim = (7, 10000)
        cells = random_cells(70000, 300, 33)
        op = Operand(dim, "double", cells, tracer("double", cells))
        L = np.arange(5000, dtype=np.int64) * 2 * 7 + (np.arange(5000) % 7)        # leaf 2k, row k % 7
        if shuffled:
            L = np.random.default_rng(34).permutation(L)
        return op, L, _vec("double", 5000, 35, zeros=0.2), "double"
    return f


def _one_leaf():
    cells = random_cells(900 * 5, 700, 36)
    op = Operand((900, 5), "double", cells, tracer("double", cells))
    L = 900 * 3 + np.random.default_rng(37).integers(0, 900, 1500)
    return op, L, _vec("double", 1500, 38, zeros=0.3), "double"


def _merged_length(total):
    """nnz(x) + nnz(Y) == total: Y holds 1047 distinct cells of column 1 of 1200 rows, over x's entries there, next to an
    untouched column of 172"""
    def f():
        nx = total - 1047 - 172
        cells = np.concatenate([np.arange(0, 1200, 7), 1200 + np.arange(nx)])
        assert cells.size == nx + 172
        op = Operand((1200, 2), "double", cells, tracer("double", cells))
        L = 1200 + np.arange(100, 1147, dtype=np.int64)
        return op, L, _vec("double", 1047, 40, zeros=0.2), "double"
    return f


def _pair_split():
    # one column: x stores rows 0 .. 1100, Y rows 1 .. 1100: the merged sequence is x0, x1 y1, x2 y2, ... -- x1024 is
    # place 2047, the last of the first tile, and the y entry it is paired with the first of the second
    cells = np.arange(1101, dtype=np.int64)
    op = Operand((1200, 1), "double", cells, tracer("double", cells))
    return op, np.arange(1, 1101, dtype=np.int64), _vec("double", 1100, 41, zeros=0.1), "double"


def _zeros_and_specials():
    """x stores the special doubles (a stored 0.0 and a stored -0.0 among them) on every third cell; the index reaches
    every second cell with the specials as values: zero onto an entry (deleted), zero onto nothing, -0.0 (deleted), NaN
    and NA stored, a covered stored zero replaced or deleted, an uncovered stored zero kept"""
    cells = np.arange(0, 37 * 23, 3, dtype=np.int64)
    op = Operand((37, 23), "double", cells, specials("double", cells.size))
    L = np.arange(0, 37 * 23, 2, dtype=np.int64)
    return op, L, np.random.default_rng(63).permutation(specials("double", L.size)), "double"      # (shuffled: every pairing occurs)


def _types(tx, tv):
    def f():
        cells = random_cells(29 * 31, 250, 50)
        op = Operand((29, 31), tx, cells, specials(tx, cells.size))
        L = np.random.default_rng(51).permutation(np.concatenate([cells[::2], random_cells(29 * 31, 200, 52)]))
        if tv == "double":
            return op, L, np.concatenate([SPECIALS_F64, _vec("double", L.size - 8, 53)]), tv
        # (a logical vector with an NA has no spelling as a Python value: TRUE and FALSE only)
        return op, L, _vec("logical", L.size, 53, zeros=0.4) if tv == "logical" else specials(tv, L.size), tv
    return f


def _nvals(n):
    def f():
        cells = random_cells(50 * 12, 200, 54)
        op = Operand((50, 12), "double", cells, tracer("double", cells))
        L = random_cells(50 * 12, 120, 55)[::-1].copy()       # descending: the unsorted route
        return op, L, _vec("double", n, 56, zeros=0.25 if n > 1 else 0.0), "double"
    return f


def _route_pair(shuffled):
    def f():
        cells = random_cells(400 * 30, 3000, 57)
        op = Operand((400, 30), "double", cells, tracer("double", cells))
        L = random_cells(400 * 30, 2500, 58)
        v = _vec("double", L.size, 59, zeros=0.3)
        if shuffled:
            o = np.random.default_rng(60).permutation(L.size)
            L, v = L[o], v[o]
        return op, L, v, "double"
    return f


def _three_d():
    op = three_d_operand("integer")
    L = np.random.default_rng(61).integers(0, op.ncells, 200)
    return op, L, _vec("integer", 200, 62, zeros=0.3), "integer"


ASSIGN = {
    "unsorted_K_2047": _unsorted_K(S - 1),
    "unsorted_K_2048": _unsorted_K(S),
    "unsorted_K_2049": _unsorted_K(S + 1),
    "one_pass_200_cells": _passes((20, 10), 70),
    "three_passes_90000_cells": _passes((300, 300), 71),
    "five_passes_past_2_32_cells": _passes((70000, 70000), 72),
    "run_of_5000_last_nonzero": _run_of_5000(4.5),
    "run_of_5000_last_zero": _run_of_5000(0.0),
    "v_0_w_on_one_cell": _v_0_w,
    "one_index_per_leaf_5000_leaves": _one_per_leaf(False),
    "one_index_per_leaf_shuffled": _one_per_leaf(True),
    "every_index_in_one_leaf": _one_leaf,
    "merged_length_T_minus_1": _merged_length(T - 1),
    "merged_length_T": _merged_length(T),
    "merged_length_T_plus_1": _merged_length(T + 1),
    "pair_split_across_a_tile_edge": _pair_split,
    "zeros_minus_zero_NaN_NA_and_stored_zeros": _zeros_and_specials,
    "types_integer_x_double_values": _types("integer", "double"),
    "types_logical_x_integer_values": _types("logical", "integer"),
    "types_double_x_integer_values_with_NA": _types("double", "integer"),
    "types_logical_x_logical_values": _types("logical", "logical"),
    "nvals_1": _nvals(1),
    "nvals_K": _nvals(120),
    "nvals_divides_K": _nvals(30),
    "route_sorted": _route_pair(False),
    "route_shuffled": _route_pair(True),
    "three_d": _three_d,
    "x_empty": lambda: (Operand((70, 9), "double", [], []), np.array([5, 600, 5, 77], dtype=np.int64),
                        np.array([1.5, -2.0, 0.0, 3.25]), "double"),
}
ASSIGN_NAMES = list(ASSIGN)
# which route each case takes: the sorted one exactly when the cells are strictly increasing
SORTED_ROUTE = {"one_index_per_leaf_5000_leaves", "merged_length_T_minus_1", "merged_length_T", "merged_length_T_plus_1",
                "pair_split_across_a_tile_edge", "zeros_minus_zero_NaN_NA_and_stored_zeros", "route_sorted"}


@functools.lru_cache(maxsize=None)
def assign_case(name):
    op, L, value, v_type = ASSIGN[name]()
    L = np.ascontiguousarray(L, dtype=np.int64)
    value = np.ascontiguousarray(value, dtype=NP_DTYPE[v_type])
    for a in (L, value, op.cells, op.vals):
        a.setflags(write=False)
    return op, L, value, v_type


@functools.lru_cache(maxsize=None)
def assign_expected(name):
    op, L, value, v_type = assign_case(name)
    new_type, cells, vals = expect_subassign(op, L, value, v_type)
    cells.setflags(write=False)
    vals.setflags(write=False)
    return new_type, cells, vals


def merged_length(name):
    """nnz(x) + nnz(Y): what the merge cuts into tiles of T"""
    op, L = assign_case(name)[:2]
    return op.cells.size + np.unique(L).size


def longest_run(name):
    """the longest run of equal cells in the sorted keys"""
    L = np.sort(assign_case(name)[1])
    edges = np.flatnonzero(np.concatenate([[True], L[1:] != L[:-1], [True]]))
    return int(np.diff(edges).max())
