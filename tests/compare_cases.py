"""Operands, operations and expectations for Compare and Logic on SVT operands (Session.compare / logic,
DeviceCSC.compare / logic), shared by tests/test_z_compare_cpu.py (the host rule functions, the case builder's proofs) and
tests/test_hip_compare.py (the device kernels).

THE EXPECTATION is R's definition, element-wise on the dense arrays with numpy (never a walk over leaves):
  Compare   both sides as.double() (NA_integer_ -> NA_real_); na = isnan(x) | isnan(y);
            value = where(na, NA_integer_, op(x, y)) as int32
  Logic     the three-valued tables: & is FALSE next to a FALSE, else NA next to an NA, else TRUE;
            | is TRUE next to a TRUE, else NA next to an NA, else FALSE
An implicit entry is a 0 (FALSE).  A position is stored in the result exactly when it is stored in an operand and the
value there is not 0.  Everything is compared bit for bit; there is no tolerance.
"""
from __future__ import annotations

import functools
import operator

import numpy as np

import arith_cases as ac
import subset_cases as sc
from sparsearray_amd import NA_integer, SVT_SparseArray

COMPARE_OPS = {"==": operator.eq, "!=": operator.ne, "<=": operator.le, ">=": operator.ge, "<": operator.lt, ">": operator.gt}
MERGE_OPS = ("!=", "<", ">")
LOGIC_OPS = ("&", "|")
NA = np.int32(NA_integer)


# ---------------------------------------------------------------------------
# R's definitions, element-wise
# ---------------------------------------------------------------------------
def compare_values(op, x, y):
    """x op y on arrays (or an array and a scalar) of int32 or float64: int32 values 0 / 1 / NA"""
    xd, yd = ac.as_double(np.atleast_1d(np.asarray(x))), ac.as_double(np.atleast_1d(np.asarray(y)))
    na = np.isnan(xd) | np.isnan(yd)
    with np.errstate(invalid="ignore"):
        v = COMPARE_OPS[op](xd, yd)
    return np.where(na, NA, v.astype(np.int32)).astype(np.int32)


def logic_values(op, x, y):
    """x & y, x | y on int32 arrays of 0 / 1 / NA"""
    x, y = np.asarray(x, np.int32), np.asarray(y, np.int32)
    na = (x == NA) | (y == NA)
    if op == "&":
        return np.where((x == 0) | (y == 0), 0, np.where(na, NA, 1)).astype(np.int32)
    return np.where((x == 1) | (y == 1), 1, np.where(na, NA, 0)).astype(np.int32)


def scalar_value(s, s_type):
    """the scalar as the array element of its R type"""
    return np.float64(s) if s_type == "double" else np.int32(s)


class Expected:
    """dense int32 values and the stored mask of a logical result"""

    def __init__(self, dense, stored):
        self.dense = np.asfortranarray(dense, dtype=np.int32)
        self.stored = np.asfortranarray(stored & (self.dense != 0))
        self.dense.setflags(write=False)
        self.stored.setflags(write=False)


def expect_compare_merge(op, x, y):
    dx, sx = ac.dense_nd(x)
    dy, sy = ac.dense_nd(y)
    return Expected(compare_values(op, dx, dy), sx | sy)


def expect_compare_scalar(op, x, s, s_type):
    dx, sx = ac.dense_nd(x)
    return Expected(compare_values(op, dx, scalar_value(s, s_type)), sx)


def expect_logic(op, x, y):
    dx, sx = ac.dense_nd(x)
    dy, sy = ac.dense_nd(y)
    return Expected(logic_values(op, dx, dy), sx | sy)


def check_result(res, x, want: Expected, what=""):
    """a Session result against the expectation: a "logical" object of x's dim with explicit values 1 / NA, rows
    ascending in every leaf, the stored mask and the values exactly"""
    assert isinstance(res, SVT_SparseArray) and res.dim == x.dim and res.type == "logical" and not res.na_background, what
    for lf in res.leaves:
        if lf is None:
            continue
        offs = np.asarray(lf[0])
        assert offs.size > 0 and offs.dtype == np.int32 and lf[1] is not None and len(lf[1]) == offs.size, what
        assert np.asarray(lf[1]).dtype == np.int32 and np.all((lf[1] == 1) | (lf[1] == NA)), f"{what}: a value that is not TRUE or NA"
        assert offs[0] >= 0 and offs[-1] < res.dim[0] and np.all(np.diff(offs) > 0), f"{what}: rows do not ascend"
    got, got_stored = ac.dense_nd(res)
    assert np.array_equal(got_stored, want.stored), \
        f"{what}: the stored entries differ at {np.argwhere(got_stored != want.stored)[:5].tolist()}"
    assert got.dtype == np.int32 and np.array_equal(got[want.stored], want.dense[want.stored]), f"{what}: values differ"


# ---------------------------------------------------------------------------
# shared operands, through the host entry points
# ---------------------------------------------------------------------------
def _logical(dim, density, seed, values, empty_cols=()):
    """a logical object: the entries of a seeded mask stored, ``values`` (TRUE, NA and stored FALSEs) cycled over them"""
    m = np.random.default_rng(seed).random(dim) < density
    m[:, list(empty_cols)] = False
    x = ac._from_values(dim, "integer", m, values)
    return SVT_SparseArray(dim, "logical", x.leaves)


_OPERANDS = {
    "l1": lambda: _logical(ac.DIM, 0.4, 41, [1, NA_integer, 0, 1, 1, 0, NA_integer], (3,)),
    "l2": lambda: _logical(ac.DIM, 0.4, 42, [NA_integer, 1, 1, 0, 1, NA_integer, 0, 1], (3, 9)),
    "l_lacunar": lambda: sc.build(ac.DIM, "logical", np.random.default_rng(43).random(ac.DIM) < 0.3, lacunar_cols=(0, 5, 28)),
    # stored zeros of both signs next to ordinary values
    "d_stored_zeros": lambda: ac._from_values(ac.DIM, "double", np.random.default_rng(44).random(ac.DIM) < 0.4,
                                              [0.0, -0.0, 2.0, -2.0, 5e-324, -5e-324, 1.0]),
}


@functools.lru_cache(maxsize=None)
def operand(name):
    return _OPERANDS[name]() if name in _OPERANDS else ac.operand(name)


# (name, x, op, scalar, its R type)
SCALAR_CASES = (
    [(f"{x}_{n}", x, op, s, st) for x in ("d1", "i1", "d1s", "i1s", "d1l", "d_mixed_sign", "i_mixed_sign", "l1")
     for n, op, s, st in (("gt_0", ">", 0, "integer"), ("ne_0", "!=", 0, "integer"), ("lt_0", "<", 0.0, "double"),
                          ("ge_1", ">=", 1, "integer"), ("le_minus_1", "<=", -1, "integer"), ("eq_3", "==", 3, "integer"),
                          ("gt_inf", ">", np.inf, "double"), ("lt_minus_inf", "<", -np.inf, "double"))] +
    [("i1_gt_2.5", "i1", ">", 2.5, "double"), ("i_mixed_sign_gt_2.5", "i_mixed_sign", ">", 2.5, "double"),
     ("i1s_gt_2.5", "i1s", ">", 2.5, "double"), ("l1_eq_true", "l1", "==", True, "logical"),
     ("l1_gt_false", "l1", ">", False, "logical"),
     ("stored_zeros_gt_0", "d_stored_zeros", ">", 0, "integer"), ("stored_zeros_ne_0", "d_stored_zeros", "!=", 0.0, "double"),
     ("stored_zeros_lt_0", "d_stored_zeros", "<", 0.0, "double"),
     ("empty", "d_empty", ">", 0, "integer"), ("ncol_0", "d_ncol0", "!=", 0, "integer"), ("nrow_0", "d_nrow0", ">", 0, "integer"),
     ("three_dimensions", "i3d", ">=", 90, "integer")])
SCALAR_NAMES = [c[0] for c in SCALAR_CASES]
SCALAR_BY_NAME = {c[0]: c for c in SCALAR_CASES}
assert len(SCALAR_BY_NAME) == len(SCALAR_CASES)

LOGIC_CASES = [("na_and_false_both_sides", "l1", "l2"), ("same_operand", "l1", "l1"), ("lacunar_left", "l_lacunar", "l2"),
               ("lacunar_right", "l1", "l_lacunar")]


# ---------------------------------------------------------------------------
# device level: the key and value placements of arith_cases.device_cases(T) under the new rules
# ---------------------------------------------------------------------------
def logical_values(n, seed):
    """n values drawn from {1, 0, NA}"""
    return np.random.default_rng(seed).choice(np.array([1, 0, NA_integer], dtype=np.int32), size=n)


def device_operands(c, values, seed=0):
    """The (kx, vx, ky, vy) of a case of arith_cases.device_cases: ``values`` "double" keeps the case's own values
    (as doubles), "integer" truncates them to int32 (equal values stay equal), "mixed" truncates both and keeps x a
    double operand, "logical" draws from {1, 0, NA}."""
    if values == "logical":
        return c.kx, logical_values(c.kx.size, 100 + seed), c.ky, logical_values(c.ky.size, 200 + seed)
    vx, vy = c.vx.astype(np.float64), c.vy.astype(np.float64)
    if values != "double":
        vx, vy = np.trunc(vx), np.trunc(vy).astype(np.int32)
        if values == "integer":
            vx = vx.astype(np.int32)
    return c.kx, np.ascontiguousarray(vx), c.ky, np.ascontiguousarray(vy)


def device_expect(rule, op, kx, vx, ky, vy, nrow, ncol):
    """the result's CSC triple (col_ptr, row_idx, int32 values) by numpy on the union of the stored positions"""
    keys = np.union1d(kx, ky)
    dx, dy = np.zeros(keys.size, dtype=vx.dtype), np.zeros(keys.size, dtype=vy.dtype)
    dx[np.searchsorted(keys, kx)] = vx
    dy[np.searchsorted(keys, ky)] = vy
    v = compare_values(op, dx, dy) if rule == "compare" else logic_values(op, dx, dy)
    keep = v != 0
    return ac._csc(keys[keep], v[keep], nrow, ncol)


def map_expect(op, cp, ri, val, s, s_type, ncol):
    """x op s on one operand's CSC triple"""
    v = compare_values(op, val, scalar_value(s, s_type))
    keep = v != 0
    col = np.repeat(np.arange(ncol), np.diff(cp))
    want_cp = np.zeros(ncol + 1, np.int64)
    np.cumsum(np.bincount(col[keep], minlength=ncol), out=want_cp[1:])
    return want_cp, ri[keep], v[keep]
