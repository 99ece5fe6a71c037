"""Operands and cases for abind() / cbind() / rbind() (Session.abind, device.abind; src/SparseArray_abind.c), shared by
tests/test_zz_abind_cpu.py (the Session logic and this module's own expectation) and tests/test_hip_abind.py (the device).

The rule is numpy's: ``np.concatenate(..., axis=along - 1)`` of the dense arrays (background filled in, values widened to
the result's type: integer or logical -> double converts the value, NA_integer_ becomes NA_real_; logical -> integer keeps
the bits) and of the boolean masks of STORED entries, at tolerance 0: values equal AS BITS, and nothing created or
dropped -- a stored zero stays stored.  ``build``, ``dense_and_stored``, ``bits`` and the palettes of special values
are those of tests/subset_cases.py.
"""
from __future__ import annotations

import functools

import numpy as np

from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from subset_cases import NP_DTYPE, bits, build, dense_and_stored

T = 4096                                # svt_dev_abind_tile(); tests/test_zz_abind_cpu.py checks it against the library
TYPE_ORDER = ("logical", "integer", "double")


def as_2d(x):
    """the same leaves as the (rows, leaves) matrix"""
    return SVT_SparseArray((x.dim[0], len(x.leaves)), x.type, x.leaves, svt_is_null=x.svt_is_null,
                           na_background=x.na_background)


def nd(x2, dim):
    """the 2-D object ``x2`` of prod(dim[1:]) columns as the N-d object of extents ``dim``"""
    assert x2.dim == (dim[0], int(np.prod(dim[1:], dtype=np.int64)))
    return SVT_SparseArray(dim, x2.type, x2.leaves, svt_is_null=x2.svt_is_null, na_background=x2.na_background)


def dense_nd(x):
    dense, stored = dense_and_stored(as_2d(x))
    return dense.reshape(x.dim, order="F"), stored.reshape(x.dim, order="F")


def widen(a, type):
    """values of an int32 or float64 array as the R type ``type``"""
    if NP_DTYPE[type] == a.dtype:
        return a
    assert type == "double" and a.dtype == np.int32
    out = a.astype(np.float64)
    out[a == NA_integer] = NA_real
    return out


def rand_mask(dim, density, seed):
    return np.random.default_rng(seed).random(dim) < density


def exact_mask(dim, k, seed):
    """a mask with exactly ``k`` entries"""
    m = np.zeros(int(np.prod(dim)), dtype=bool)
    m[np.random.default_rng(seed).choice(m.size, size=k, replace=False)] = True
    return m.reshape(dim, order="F")


def obj(dim, type="double", density=0.4, seed=0, palette="tracer", mask=None, na_background=False, empty_leaves=()):
    dim = tuple(dim)
    d2 = (dim[0], int(np.prod(dim[1:], dtype=np.int64)))
    mask = rand_mask(d2, density, seed) if mask is None else np.asarray(mask, dtype=bool).reshape(d2, order="F")
    mask = mask.copy()
    mask[:, list(empty_leaves)] = False
    return nd(build(d2, type, mask, palette, na_background=na_background), dim)


def _leaf_run_masks(before):
    """two operands of 50 rows x 400 leaves: exactly ``before`` entries between them in the leaves [0, 45), the leaves
    [45, 345) empty in both, entries again from leaf 345 on"""
    head = exact_mask((100, 45), before, 40)
    tail = rand_mask((100, 55), 0.3, 41)
    full = np.zeros((100, 400), dtype=bool)
    full[:, :45], full[:, 345:] = head, tail
    return full[:50], full[50:]


# name -> (along, builder of the objects).  Row form first, then the leaf forms, then the types.
_CASES = {
    "rows_5_and_7": (1, lambda: [obj((5, 3), seed=1), obj((7, 3), seed=2)]),
    "rows_empty_leaf_left": (1, lambda: [obj((5, 3), seed=3, empty_leaves=(1,)), obj((7, 3), density=0.9, seed=4)]),
    "rows_empty_leaf_right": (1, lambda: [obj((5, 3), density=0.9, seed=5), obj((7, 3), seed=6, empty_leaves=(1,))]),
    "rows_empty_leaf_both": (1, lambda: [obj((5, 3), seed=7, empty_leaves=(1,)), obj((7, 3), seed=8, empty_leaves=(1,))]),
    "rows_object_of_0_rows": (1, lambda: [obj((5, 3), seed=9), obj((0, 3)), obj((4, 3), seed=10)]),
    "rows_object_of_0_nonzeros": (1, lambda: [obj((4, 3), density=0.0), obj((5, 3), seed=11), obj((2, 3), density=0.0)]),
    "rows_all_empty": (1, lambda: [obj((4, 3), density=0.0), obj((5, 3), density=0.0)]),
    "rows_one_object": (1, lambda: [obj((9, 4), seed=12)]),
    "rows_1d": (1, lambda: [obj((6,), seed=13), obj((3,), seed=14)]),
    "rows_70_objects": (1, lambda: [obj((3, 5), density=0.5, seed=100 + n) for n in range(70)]),
    "rows_nnz_T": (1, lambda: [obj((100, 50), mask=exact_mask((100, 50), 2000, 15)),
                               obj((100, 50), mask=exact_mask((100, 50), T - 2000, 16))]),
    "rows_nnz_T_plus_1": (1, lambda: [obj((100, 50), mask=exact_mask((100, 50), 2000, 17)),
                                      obj((100, 50), mask=exact_mask((100, 50), T + 1 - 2000, 18))]),
    "rows_nnz_2T_plus_1": (1, lambda: [obj((100, 50), mask=exact_mask((100, 50), 4500, 19)),
                                       obj((100, 50), mask=exact_mask((100, 50), 2 * T + 1 - 4500, 20))]),
    # one result leaf of 6000 + 4500 entries: three tiles, the boundary between the objects inside the middle one
    "rows_leaf_over_three_tiles": (1, lambda: [obj((6000, 1), density=1.1), obj((5000, 1), mask=exact_mask((5000, 1), 4500, 21))]),
    # 600 empty pieces at entry 4000 (inside the first tile: more boundaries than the workgroup has threads) and at
    # entry 4096 (exactly on the tile boundary)
    "rows_300_empty_leaves_inside_a_tile": (1, lambda: [obj((50, 400), mask=m) for m in _leaf_run_masks(4000)]),
    "rows_300_empty_leaves_on_the_tile_boundary": (1, lambda: [obj((50, 400), mask=m) for m in _leaf_run_masks(T)]),
    "cbind_3_matrices_one_without_columns": (2, lambda: [obj((6, 4), seed=22), obj((6, 0)), obj((6, 5), seed=23)]),
    "cbind_zero_rows": (2, lambda: [obj((0, 4)), obj((0, 2))]),
    "cbind_no_columns_at_all": (2, lambda: [obj((6, 0)), obj((6, 0))]),
    "cbind_one_object": (2, lambda: [obj((6, 4), seed=24)]),
    "cbind_70_objects": (2, lambda: [obj((4, n % 3), density=0.6, seed=200 + n) for n in range(70)]),
    "along2_of_3d": (2, lambda: [obj((4, 3, 2), seed=25), obj((4, 2, 2), seed=26), obj((4, 0, 2))]),
    "along3_of_4d_inner3_outer2": (3, lambda: [obj((3, 3, 2, 2), seed=27), obj((3, 3, 1, 2), seed=28), obj((3, 3, 3, 2), seed=29)]),
    "along_last_of_3d": (3, lambda: [obj((4, 3, 2), seed=30), obj((4, 3, 1), seed=31)]),
    "along_new_dimension": (3, lambda: [obj((4, 3), seed=32), obj((4, 3), seed=33), obj((4, 3), density=0.0)]),
    "cbind_piece_on_the_tile_boundary": (2, lambda: [obj((100, 50), mask=exact_mask((100, 50), T, 34)), obj((100, 7), seed=35)]),
    "cbind_300_empty_columns_inside_a_tile": (2, lambda: [obj((100, 45), mask=exact_mask((100, 45), 4000, 36)), obj((100, 300), density=0.0),
                                                           obj((100, 20), seed=37)]),
    "types_logical_integer_double_rows": (1, lambda: [obj((9, 4), "logical", palette="specials", seed=50),
                                                      obj((8, 4), "integer", palette="specials", seed=51),
                                                      obj((7, 4), "double", palette="specials", seed=52)]),
    "types_logical_integer_double_cols": (2, lambda: [obj((9, 4), "double", palette="specials", seed=53),
                                                      obj((9, 3), "logical", palette="specials", seed=54),
                                                      obj((9, 5), "integer", palette="specials", seed=55)]),
    "types_logical_integer": (1, lambda: [obj((9, 4), "logical", palette="specials", seed=56),
                                          obj((8, 4), "integer", palette="specials", seed=57)]),
    "types_logical_only": (2, lambda: [obj((9, 4), "logical", palette="specials", seed=58), obj((9, 2), "logical", seed=59)]),
    "types_integer_only": (1, lambda: [obj((9, 4), "integer", palette="specials", seed=60), obj((3, 4), "integer", seed=61)]),
    "types_double_specials_rows": (1, lambda: [obj((9, 4), palette="specials", seed=62), obj((8, 4), palette="specials", seed=63)]),
    "types_double_specials_cols": (2, lambda: [obj((9, 4), palette="specials", seed=64), obj((9, 6), palette="specials", seed=65)]),
    "types_one_integer_object": (2, lambda: [obj((9, 4), "integer", palette="specials", seed=66)]),
    "naarray_pair_cols": (2, lambda: [obj((9, 4), palette="specials", seed=67, na_background=True),
                                      obj((9, 3), palette="specials", seed=68, na_background=True)]),
    "naarray_integer_and_double_rows": (1, lambda: [obj((5, 4), "integer", seed=69, na_background=True),
                                                    obj((6, 4), "double", palette="specials", seed=70, na_background=True)]),
}
NAMES = list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(along, objects, ans_type, expected dense, expected stored mask); the arrays are read-only"""
    along, make = _CASES[name]
    objects = make()
    ans_type = max((x.type for x in objects), key=TYPE_ORDER.index)
    ndim = max(along, max(x.ndim for x in objects))
    parts = [dense_nd(x) for x in objects]
    pad = lambda a: a.reshape(a.shape + (1,) * (ndim - a.ndim), order="F")      # noqa: E731
    want = np.concatenate([pad(widen(d, ans_type)) for d, _ in parts], axis=along - 1)
    want_stored = np.concatenate([pad(s) for _, s in parts], axis=along - 1)
    want.setflags(write=False)
    want_stored.setflags(write=False)
    return along, objects, ans_type, want, want_stored


def padded_dims(name):
    """the dim of every object with the trailing 1s abind() gives it"""
    along, objects = case(name)[:2]
    ndim = max(along, max(x.ndim for x in objects))
    return [x.dim + (1,) * (ndim - len(x.dim)) for x in objects]


def check_invariants(res):
    assert isinstance(res, SVT_SparseArray)
    assert len(res.leaves) == int(np.prod(res.dim[1:], dtype=np.int64))
    for lf in res.leaves:
        if lf is None:
            continue
        offs = np.asarray(lf[0])
        assert offs.size > 0 and offs.dtype == np.int32
        assert offs[0] >= 0 and offs[-1] < res.dim[0] and np.all(np.diff(offs) > 0)
        assert lf[1] is None or (len(lf[1]) == offs.size and np.asarray(lf[1]).dtype == res.np_dtype)
    assert res.svt_is_null == all(lf is None for lf in res.leaves)


def check(res, name, what=""):
    along, objects, ans_type, want, want_stored = case(name)
    what = f"{what}{name}"
    check_invariants(res)
    assert res.type == ans_type, f"{what}: type {res.type}, want {ans_type}"
    assert res.na_background == objects[0].na_background, f"{what}: the background"
    assert res.dim == want.shape, f"{what}: dim {res.dim}, want {want.shape}"
    got, got_stored = dense_nd(res)
    assert np.array_equal(got_stored, want_stored), f"{what}: the stored entries differ"
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), f"{what}: values differ as bits"


def restate(objects, along, ans_type):
    """concatenate_leaves (along == 1) and concatenate_SVTs with its recursion (along >= 2), leaf by leaf in plain Python
    on objects of the same number of dimensions: the device rules of include/svt_hip.h, not numpy's"""
    x = objects[0]
    dtype = NP_DTYPE[ans_type]

    def vals(o, lf):
        return widen(np.ones(len(lf[0]), o.np_dtype) if lf[1] is None else np.asarray(lf[1]), ans_type).astype(dtype, copy=False)
    leaves = []
    if along == 1:
        off = np.concatenate([[0], np.cumsum([o.dim[0] for o in objects])])
        for L in range(len(x.leaves)):
            parts = [(o.leaves[L][0] + np.int32(off[n]), vals(o, o.leaves[L])) for n, o in enumerate(objects)
                     if o.leaves[L] is not None]
            leaves.append(None if not parts else (np.concatenate([p[0] for p in parts]).astype(np.int32),
                                                  np.concatenate([p[1] for p in parts])))
        dim = (int(off[-1]),) + x.dim[1:]
    else:
        inner = int(np.prod(x.dim[1:along - 1], dtype=np.int64))
        outer = int(np.prod(x.dim[along:], dtype=np.int64))
        ext = [o.dim[along - 1] for o in objects]
        start = np.concatenate([[0], np.cumsum(ext)])
        D = int(start[-1])
        for c in range(outer):
            for j in range(D):
                n = max(k for k in range(len(objects)) if start[k] <= j and ext[k] > 0)
                for a in range(inner):
                    lf = objects[n].leaves[a + inner * ((j - int(start[n])) + ext[n] * c)]
                    leaves.append(None if lf is None else (np.asarray(lf[0], np.int32), vals(objects[n], lf)))
        dim = x.dim[:along - 1] + (D,) + x.dim[along:]
    return SVT_SparseArray(dim, ans_type, leaves, na_background=x.na_background)


# ---------------------------------------------------------------------------
# the refusals of the device level: all of them are answered on the host, before anything is launched, read or written
# ---------------------------------------------------------------------------
LGLSXP, INTSXP, REALSXP = 10, 13, 14


def bare_handles(lib, specs):
    """(handles, their table) of operands of (Rtype, nrow, ncol) whose arrays are never read"""
    import ctypes
    hs = [lib.svt_wrap_device_csc(rt, nrow, ncol, 0, None, None, None) for rt, nrow, ncol in specs]
    assert all(hs)
    return hs, (ctypes.c_void_p * len(hs))(*hs)


REFUSALS = [
    # (what, specs of (Rtype, nrow, ncol), nobj or None for all of them, inner, ext, ans_Rtype, message)
    ("nobj_0", [(REALSXP, 4, 3)], 0, 1, None, REALSXP, "at least one object"),
    ("leaf_counts_differ", [(REALSXP, 4, 3), (REALSXP, 4, 2)], None, 1, None, REALSXP, "leaves"),
    ("nrow_differ", [(REALSXP, 4, 3), (REALSXP, 5, 3)], None, 1, [3, 3], REALSXP, "rows"),
    ("ncol_not_inner_ext_outer", [(REALSXP, 4, 6), (REALSXP, 4, 5)], None, 2, [3, 2], REALSXP, "inner \\* ext \\* outer"),
    ("outer_differs", [(REALSXP, 4, 6), (REALSXP, 4, 8)], None, 2, [3, 2], REALSXP, "outer"),
    ("ans_type_narrower", [(INTSXP, 4, 3), (REALSXP, 4, 3)], None, 1, None, INTSXP, "narrower"),
    ("ans_type_logical_for_integer", [(LGLSXP, 4, 3), (INTSXP, 4, 3)], None, 1, None, LGLSXP, "narrower"),
    ("ans_type_unknown", [(REALSXP, 4, 3)], None, 1, None, 16, "invalid requested type"),
    ("row_sum_past_int", [(REALSXP, 2 ** 30, 3), (REALSXP, 2 ** 30, 3)], None, 1, None, REALSXP, "2\\^31 - 1"),
    ("negative_ext", [(REALSXP, 4, 3), (REALSXP, 4, 3)], None, 1, [3, -3], REALSXP, "negative extent"),
]
