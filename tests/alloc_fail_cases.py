"""A failed allocation in the middle of a composition: one row per entry point that leaves a new sparse operand in the
caller's allocator (include/svt_hip.h, "device level"), shared by the test without a GPU (host memory, operands without
entries, the first and the second allocation fail: nothing is launched before either) and the one on the device (torch
allocations, every allocation from the third on fails in turn).

A row is (name, entry point, ncol of the result, bytes per value, call).  ``call(lib, o, tail)`` makes the call: ``o``
holds the operands (``Operands``), ``tail`` the arguments from ``alloc`` to ``out_val`` in the order of svt_dev_subset --
(alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val) -- and the row puts what its entry point has besides
(out_Rtype, the overflow word, bad_index, the extents of abind, not_finite) where the header has it."""
import ctypes
from ctypes import c_int, c_int64, c_void_p

from sparsearray_amd.api import ARITH_OPCODES, COMPARE_OPCODES, ISFUN_OPCODES, LOGIC_OPCODES, PMINMAX_OPCODES
from sparsearray_amd.svt import LGLSXP, REALSXP

ARITH_SCALAR = 1                                            # kind of svt_dev_arith_map
SENTINEL_NNZ, SENTINEL_PTR = -7, 0xA5A5A5A0


class Operands:
    """What the rows read.  Handles: ``x``, ``y`` (5 x 4 double), ``lx``, ``ly`` (5 x 4 logical), ``b`` (4 x 3 double),
    ``v`` (2 x 2 double).  Pointers (host or device, as the test has them): ``dense`` (20 doubles), ``stats`` (4 doubles
    >= 0, one per column), ``vals`` (1 double), ``rows`` / ``leaves`` (2 int32 each, increasing), ``cols`` (2 int32),
    ``rows3`` (3 int32, increasing), ``rows_general`` (3 int32, unsorted with a repeat), ``L`` (2 int64 cells), ``M``
    (2 x 2 int32 coordinates, column-major), ``word`` (an int32 for the overflow / not_finite flag; None without a GPU),
    ``stream``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.dim = (c_int64 * 2)(5, 4)
        self.rt, self.bad = c_int(-7), c_int64(-7)
        self.nrow, self.nleaves = c_int64(-7), c_int64(-7)


def _rt(o):
    return ctypes.byref(o.rt)


def _sweep(o):
    return (o.stats, REALSXP, 4, 0, 1, 4)


ROWS = [
    ("arith_merge", "svt_dev_arith_merge", 4, 8, lambda lib, o, t: lib.svt_dev_arith_merge(
        o.x, o.y, ARITH_OPCODES["+"], *t[:3], _rt(o), *t[3:], o.word, o.stream)),
    ("arith_map", "svt_dev_arith_map", 4, 8, lambda lib, o, t: lib.svt_dev_arith_map(
        o.x, ARITH_SCALAR, ARITH_OPCODES["*"], 2.0, REALSXP, *t[:3], _rt(o), *t[3:], o.word, o.stream)),
    ("compare_merge", "svt_dev_compare_merge", 4, 4, lambda lib, o, t: lib.svt_dev_compare_merge(
        o.x, o.y, COMPARE_OPCODES["!="], *t, o.stream)),
    ("compare_map", "svt_dev_compare_map", 4, 4, lambda lib, o, t: lib.svt_dev_compare_map(
        o.x, COMPARE_OPCODES[">"], 0.0, REALSXP, *t, o.stream)),
    ("logic_merge", "svt_dev_logic_merge", 4, 4, lambda lib, o, t: lib.svt_dev_logic_merge(
        o.lx, o.ly, LOGIC_OPCODES["|"], *t, o.stream)),
    ("pminmax_merge", "svt_dev_pminmax_merge", 4, 8, lambda lib, o, t: lib.svt_dev_pminmax_merge(
        o.x, o.y, PMINMAX_OPCODES["pmin"], *t[:3], _rt(o), *t[3:], o.stream)),
    ("pminmax_map", "svt_dev_pminmax_map", 4, 8, lambda lib, o, t: lib.svt_dev_pminmax_map(
        o.x, PMINMAX_OPCODES["pmin"], 1.0, REALSXP, *t[:3], _rt(o), *t[3:], o.stream)),
    ("isfun_map", "svt_dev_isfun_map", 4, 4, lambda lib, o, t: lib.svt_dev_isfun_map(
        o.x, ISFUN_OPCODES["is.na"], *t, o.stream)),
    ("arith_sweep", "svt_dev_arith_sweep", 4, 8, lambda lib, o, t: lib.svt_dev_arith_sweep(
        o.x, ARITH_OPCODES["*"], *_sweep(o), *t[:3], _rt(o), *t[3:], o.word, ctypes.byref(o.bad), o.stream)),
    ("compare_sweep", "svt_dev_compare_sweep", 4, 4, lambda lib, o, t: lib.svt_dev_compare_sweep(
        o.x, COMPARE_OPCODES[">"], *_sweep(o), *t, ctypes.byref(o.bad), o.stream)),
    ("pminmax_sweep", "svt_dev_pminmax_sweep", 4, 8, lambda lib, o, t: lib.svt_dev_pminmax_sweep(
        o.x, PMINMAX_OPCODES["pmin"], *_sweep(o), *t[:3], _rt(o), *t[3:], ctypes.byref(o.bad), o.stream)),
    ("abind", "svt_dev_abind", 4, 8, lambda lib, o, t: lib.svt_dev_abind(
        (c_void_p * 2)(o.x, o.y), 2, 0, None, REALSXP, *t[:3], ctypes.byref(o.nrow), ctypes.byref(o.nleaves), *t[3:], o.stream)),
    ("from_dense", "svt_dev_from_dense", 4, 8, lambda lib, o, t: lib.svt_dev_from_dense(
        o.dense, REALSXP, 5, 4, REALSXP, 0, *t, o.stream)),
    ("subset_cols", "svt_dev_subset", 2, 8, lambda lib, o, t: lib.svt_dev_subset(o.x, None, -1, o.cols, 2, *t, o.stream)),
    ("subset_rows", "svt_dev_subset", 4, 8, lambda lib, o, t: lib.svt_dev_subset(o.x, o.rows3, 3, None, -1, *t, o.stream)),
    ("subassign_vector", "svt_dev_subassign_vector", 4, 8, lambda lib, o, t: lib.svt_dev_subassign_vector(
        o.x, o.rows, 2, o.leaves, 2, o.vals, 1, REALSXP, *t[:3], _rt(o), *t[3:], o.stream)),
    ("subassign_svt", "svt_dev_subassign_svt", 4, 8, lambda lib, o, t: lib.svt_dev_subassign_svt(
        o.x, o.rows, 2, o.leaves, 2, o.v, *t[:3], _rt(o), *t[3:], o.stream)),
    ("subassign_lindex", "svt_dev_subassign_lindex", 4, 8, lambda lib, o, t: lib.svt_dev_subassign_lindex(
        o.x, o.L, 2, o.vals, 1, REALSXP, *t[:3], _rt(o), *t[3:], o.stream)),
    ("subassign_mindex", "svt_dev_subassign_mindex", 4, 8, lambda lib, o, t: lib.svt_dev_subassign_mindex(
        o.x, o.M, 2, 2, o.dim, o.vals, 1, REALSXP, *t[:3], _rt(o), *t[3:], o.stream)),
]
# on the device only: the product asks the device for its LDS size before it allocates; an unsorted row subscript with
# a repeat takes t() -> gather -> t(), the route with the most allocations
GPU_ROWS = ROWS + [
    ("spgemm", "svt_dev_spgemm", 3, 8, lambda lib, o, t: lib.svt_dev_spgemm(o.x, o.b, *t, o.word, o.stream)),
    ("subset_rows_general", "svt_dev_subset", 4, 8, lambda lib, o, t: lib.svt_dev_subset(
        o.x, o.rows_general, 3, None, -1, *t, o.stream)),
]


class Outputs:
    """out_nnz and the three result pointers, holding sentinels"""

    def __init__(self):
        self.nnz = c_int64(SENTINEL_NNZ)
        self.ptr = [c_void_p(SENTINEL_PTR) for _ in range(3)]

    def byref(self):
        return [ctypes.byref(self.nnz)] + [ctypes.byref(p) for p in self.ptr]

    def untouched(self):
        return self.nnz.value == SENTINEL_NNZ and all(p.value == SENTINEL_PTR for p in self.ptr)


def check_failure(lib, entry, rc, live, outs):
    """what every failed allocation must leave behind"""
    msg = lib.svt_last_error().decode()
    assert rc == -1, (rc, msg)
    assert f"{entry}: device allocation failed" in msg, msg
    assert len(live) == 0, f"{len(live)} blocks were not released"
    assert outs.untouched()
