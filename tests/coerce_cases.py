"""Cases of the coercions dense array <-> sparse operand and of nzwhich (include/svt_hip.h, svt_dev_from_dense /
svt_dev_to_dense / svt_dev_nzwhich), shared by tests/test_zzzz_coerce_cpu.py and tests/test_hip_coerce.py.

A case is (dense numpy array in R's layout, type, na_background, ans_type); its expectation comes from numpy alone:

    flat = a.reshape(-1, order="F");  pos = np.flatnonzero(keep(flat))
    row_idx = pos % nrow;  val = flat[pos], widened where the case asks
    col_ptr = np.searchsorted(pos, np.arange(nleaves + 1) * nrow)

The shapes are the smallest at which the kernels can still go wrong, T = the tile of the kernels: one row; many leaf
boundaries per tile; the wavefront edge; a leaf over several tiles; cell counts around a multiple of T; nothing kept and
everything kept; runs of empty leaves; more tiles than the capped grid of 2048 workgroups; extents of zero; 1-D to 4-D.
The values cycle over a palette per type that holds what the keep rule must tell apart (-0.0, NaN, NA_real_, a NaN of
another payload, +-Inf, a subnormal; NA_integer_ and INT_MAX; TRUE, FALSE and NA)."""
import functools
import struct

import numpy as np

from sparsearray_amd._hip import load_library
from sparsearray_amd.svt import NA_integer, NA_real, is_NA_real

T = 4096
assert load_library().svt_dev_coerce_tile() == T
GRID = 2048                                             # the cap of the kernels' grids, in workgroups = tiles in flight

NP_OF = {"logical": np.int32, "integer": np.int32, "double": np.float64}
NAN_PAYLOAD = np.frombuffer(struct.pack("<Q", 0x7FF8000000000123), dtype=np.float64)[0]
PALETTE = {
    "double": np.array([1.5, -0.0, np.nan, NA_real, 0.0, NAN_PAYLOAD, np.inf, -2.25, -np.inf, 5e-324, NA_real, 1e300, 3.0]),
    "integer": np.array([1, 0, NA_integer, 2 ** 31 - 1, -7, 12345, NA_integer], dtype=np.int32),
    "logical": np.array([1, 0, NA_integer, 1], dtype=np.int32),
}


def background(type_, na_background):
    if not na_background:
        return NP_OF[type_](0)
    return NA_real if type_ == "double" else NA_integer


def dense(shape, type_, na_background=False, density=0.3, seed=0, empty_leaves=(), everything=False):
    """A dense array of ``shape`` in R's layout: the background where nothing is placed, palette values (some of which
    the keep rule drops) at about ``density`` of the cells, the leaves of ``empty_leaves`` all background; or
    (``everything``) a kept value in every cell."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape, dtype=np.int64))
    flat = np.full(n, background(type_, na_background), dtype=NP_OF[type_])
    if everything:
        flat[:] = 1 if type_ == "logical" else 7
    else:
        at = np.flatnonzero(rng.random(n) < density)
        flat[at] = PALETTE[type_][(np.arange(at.size) + seed) % len(PALETTE[type_])]
        nrow = shape[0]
        for q in empty_leaves:
            flat[q * nrow:(q + 1) * nrow] = background(type_, na_background)
    return flat.reshape(shape, order="F")


def keep_mask(flat, type_, na_background):
    if na_background:
        return ~is_NA_real(flat) if type_ == "double" else flat != NA_integer
    return flat != 0


def widen(v, type_, ans_type):
    """values of ``type_`` in ``ans_type``: the same element size as bits, int32 -> double with NA_integer_ -> NA_real_"""
    if NP_OF[type_] == NP_OF[ans_type]:
        return v.copy()
    assert ans_type == "double"
    out = v.astype(np.float64)
    out[v == NA_integer] = NA_real
    return out


def expected(a, type_, na_background, ans_type):
    """(col_ptr, row_idx, val, pos) of the operand of ``a``"""
    nrow = a.shape[0]
    nleaves = int(np.prod(a.shape[1:], dtype=np.int64))
    flat = a.reshape(-1, order="F")
    pos = np.flatnonzero(keep_mask(flat, type_, na_background)).astype(np.int64)
    row_idx = (pos % max(nrow, 1)).astype(np.int32)
    val = widen(flat[pos], type_, ans_type)
    col_ptr = np.searchsorted(pos, np.arange(nleaves + 1, dtype=np.int64) * nrow).astype(np.int64)
    return col_ptr, row_idx, val, pos


def dense_of(a, type_, na_background, ans_type):
    """``a`` as the dense array of ``ans_type`` the operand stands for: the kept cells widened, the background elsewhere"""
    flat = a.reshape(-1, order="F")
    out = np.full(flat.size, background(ans_type, na_background), dtype=NP_OF[ans_type])
    k = keep_mask(flat, type_, na_background)
    out[k] = widen(flat[k], type_, ans_type)
    return out.reshape(a.shape, order="F")


# name -> (shape, type, keywords of dense()); each is run under both backgrounds
SHAPES = {
    "nrow_1": ((1, 5000), "double", {}),
    "nrow_7_3000_leaves": ((7, 3000), "integer", {}),
    "nrow_64": ((64, 130), "double", {}),
    "nrow_65": ((65, 130), "logical", {}),
    "nrow_T_2_leaves": ((T, 2), "double", {}),
    "nrow_T_plus_1_3_leaves": ((T + 1, 3), "integer", {}),
    "nrow_3T_plus_5_2_leaves": ((3 * T + 5, 2), "double", {}),
    "cells_2T_minus_1_1d": ((2 * T - 1,), "double", {}),
    "cells_2T_1d": ((2 * T,), "integer", {}),
    "cells_2T_plus_1_1d": ((2 * T + 1,), "logical", {}),
    "cells_3T_as_96_by_128": ((96, 128), "double", {"density": 0.6}),
    "all_background": ((100, 90), "double", {"density": 0.0}),
    "all_kept": ((100, 90), "integer", {"everything": True}),
    "empty_leaves_first_last_and_in_runs": ((50, 400), "double", {"empty_leaves": tuple(range(10)) + tuple(range(100, 300))
                                                                  + tuple(range(380, 400))}),
    "more_tiles_than_the_grid": ((1050, 8000), "logical", {}),
    # nzwhich cuts the ENTRIES into tiles: more than GRID * T of them, so that its grid takes a second trip
    "more_entry_tiles_than_the_grid": ((1050, 8000), "logical", {"everything": True}),
    "dim_0_5": ((0, 5), "double", {}),
    "dim_5_0": ((5, 0), "integer", {}),
    "dim_4_0_3": ((4, 0, 3), "double", {}),
    "dim_5_4_3": ((5, 4, 3), "double", {"density": 0.5}),
    "dim_3_4_2_5": ((3, 4, 2, 5), "integer", {"density": 0.5}),
    "doubles_dense_specials": ((37, 11), "double", {"density": 1.0}),
    "integers_dense_specials": ((37, 11), "integer", {"density": 1.0}),
    "logicals_dense_specials": ((37, 11), "logical", {"density": 1.0}),
}
assert 1050 * 8000 > GRID * T
WIDENINGS = [("logical", "integer"), ("logical", "double"), ("integer", "double")]

# name -> (shape, type, na_background, ans_type, keywords)
CASES = {}
for _name, (_shape, _type, _kw) in SHAPES.items():
    for _na in (False, True):
        CASES[_name + ("_na" if _na else "")] = (_shape, _type, _na, _type, _kw)
for _from, _to in WIDENINGS:
    for _na in (False, True):
        CASES[f"widen_{_from}_to_{_to}" + ("_na" if _na else "")] = ((65, 130), _from, _na, _to, {"density": 0.5})
        CASES[f"widen_{_from}_to_{_to}_3d" + ("_na" if _na else "")] = ((5, 4, 3), _from, _na, _to, {"density": 0.7})
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(a, type, na_background, ans_type, (col_ptr, row_idx, val, pos)); computed once, never written to"""
    shape, type_, na, ans_type, kw = CASES[name]
    a = dense(shape, type_, na, seed=NAMES.index(name), **kw)
    want = expected(a, type_, na, ans_type)
    for arr in (a,) + want:
        arr.setflags(write=False)
    return a, type_, na, ans_type, want
