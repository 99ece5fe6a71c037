"""Operands, operations and expectations for Arith, unary minus and Math on SVT operands (Session.arith / unary_minus /
math), shared by tests/test_arith_cpu.py (the case builder's own proofs, the host rule functions) and
tests/test_hip_arith.py (the device kernels).

THE EXPECTATION is R's definition of the operators, element-wise on the dense arrays with numpy (never a walk over
leaves): an implicit entry is a 0 of the operand's type, int op int is computed exactly in int64 and becomes NA_integer_
(with the overflow flag) outside (INT_MIN, INT_MAX], a double side turns NA_integer_ into NA_real_, ``%%`` is
``x - s * floor(x / s)`` and ``%/%`` is ``floor(x / s)`` with R's infinite and zero cases, ``^`` is R_pow.  A position
is stored in the result exactly when it is stored in an operand and the result there is not ``== 0``.

HOW VALUES ARE COMPARED: as bits, and the stored mask exactly, with these classes per element (``cls``):
  EXACT      the bits of the numpy result.
  NAN_SIGN   the result is a NaN that numpy computed by ARITHMETIC from at most one NaN operand -- that operand,
             quieted, or the default NaN of an invalid operation (Inf - Inf, 0 * Inf, sqrt(-1)).  All bits but the
             sign are compared, so the payload and NA-ness (low word 1954) must survive.  IEEE 754-2008 6.3 leaves
             the sign of a NaN result of an arithmetic operation to the implementation (x86 produces the default NaN
             with the sign set, gfx950 with the sign clear; `0 - y` may or may not flip a NaN's sign), which is the
             issue's "the payload is the hardware's choice" for the one bit numpy's answer cannot fix either.  The
             sign operations -- unary minus, abs, sign() -- are bit operations and stay EXACT.
  ANY_NAN    arithmetic on two NaN operands: only "is NaN" is compared.
  ULPS       log1p, expm1 and ``^`` call the device math library: the yardstick is the correctly rounded value
             (mpmath at 200 bits, rounded to nearest), the distance is counted in representable doubles, and a NaN
             is compared as "is NaN" plus NA-ness when the operand was NA.
"""
from __future__ import annotations

import functools

import numpy as np

import subset_cases as sc
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd.svt import is_NA_real

EXACT, NAN_SIGN, ANY_NAN, ULPS = 0, 1, 2, 3
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SIGN = np.uint64(1 << 63)
MERGE_OPS = ("+", "-", "*")
SCALAR_OPS = ("*", "/", "^", "%%", "%/%")
MATH_OPS = ("abs", "sign", "sqrt", "floor", "ceiling", "trunc", "log1p", "expm1")
ULPS_MATH = ("log1p", "expm1")


# ---------------------------------------------------------------------------
# R's definitions, element-wise
# ---------------------------------------------------------------------------
def as_double(a):
    """as.double() of an integer array (NA_integer_ -> NA_real_); a double array as it is"""
    if a.dtype == np.float64:
        return a
    out = a.astype(np.float64)
    out[a == NA_integer] = NA_real
    return out


def out_type(kind, op, x_type, y_type=None):
    """the result's type: get_Arith_output_type (R/SparseArray-Arith-methods.R:38-52) and .Arith_SVT1_v2's coercion"""
    if kind == "math":
        return "double"
    if kind == "neg":
        return x_type
    if op in ("/", "^"):
        return "double"
    return "integer" if x_type == "integer" and y_type == "integer" else "double"


def _int_arith(op, x, y):
    """int op int: (values int32, overflow flag)"""
    x64, y64 = x.astype(np.int64), np.broadcast_to(np.asarray(y), x.shape).astype(np.int64)
    na = (x64 == INT_MIN) | (y64 == INT_MIN)
    safe_y = np.where(y64 == 0, 1, y64)
    if op == "+":
        v = x64 + y64
    elif op == "-":
        v = x64 - y64
    elif op == "*":
        v = x64 * y64
    elif op == "%%":
        v, na = np.mod(x64, safe_y), na | (y64 == 0)
    elif op == "%/%":
        v, na = np.floor_divide(x64, safe_y), na | (y64 == 0)
    else:
        raise ValueError(op)
    over = ~na & ((v <= INT_MIN) | (v > INT_MAX))
    return np.where(na | over, INT_MIN, v).astype(np.int32), bool(over.any())


def _correctly_rounded(f, args):
    """f(*args) in mpmath at 200 bits, rounded to the nearest double"""
    import mpmath
    with mpmath.workprec(200):
        v = f(*[mpmath.mpf(float(a)) for a in args])
        if isinstance(v, mpmath.mpc):
            return float("nan")
        return float(v)


def r_pow(x, y):
    """R_pow (arithmetic.c), one element: the specials by rule, the rest correctly rounded"""
    import mpmath
    x, y = float(x), float(y)
    if x == 1.0 or y == 0.0:
        return 1.0
    if np.isnan(x) or np.isnan(y):
        return x + y
    if np.isinf(x) or np.isinf(y) or x == 0.0:
        if x < 0 and np.isinf(y):
            return float("nan")
        if x == -np.inf and y != np.trunc(y):
            return float("nan")
        with np.errstate(all="ignore"):
            return float(np.power(np.float64(x), np.float64(y)))        # 0, Inf, +-0: exact by IEEE 754 9.2.1
    if x < 0 and y != np.trunc(y):
        return float("nan")
    return _correctly_rounded(mpmath.power, (x, y))


def r_log1p(x):
    import mpmath
    x = float(x)
    if np.isnan(x) or x == np.inf or x == 0.0:
        return x
    if x < -1.0:
        return float("nan")
    if x == -1.0:
        return -np.inf
    return _correctly_rounded(mpmath.log1p, (x,))


def r_expm1(x):
    import mpmath
    x = float(x)
    if np.isnan(x) or x == np.inf or x == 0.0:
        return x
    if x == -np.inf:
        return -1.0
    return _correctly_rounded(mpmath.expm1, (x,))


def _double_arith(op, x, y):
    """double op double by R's rules; (values, cls)"""
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), x.shape)
    nx, ny = np.isnan(x), np.isnan(y)
    inf = np.inf
    with np.errstate(all="ignore"):
        if op == "+":
            v = x + y
        elif op == "-":
            v = x - y
        elif op == "*":
            v = x * y
        elif op == "/":
            v = x / y
        elif op == "%%":
            v = x - y * np.floor(x / y)
            v = np.where(y == inf, np.where(nx | (x > 0), x, inf), v)
            v = np.where(y == -inf, np.where(nx | (x < 0), x, -inf), v)
            v = np.where(x == 0.0, np.where(ny, y, 0.0), v)
            v = np.where((y == 0.0) | np.isinf(x), np.nan, v)
        elif op == "%/%":
            v = np.floor(x / y)
            v = np.where((y == inf) & (x < 0) & (x != -inf), -1.0, v)
            v = np.where((y == -inf) & (x > 0) & (x != inf), -1.0, v)
            v = np.where(((y == inf) & (x == -inf)) | ((y == -inf) & (x == inf)), np.nan, v)
        elif op == "^":
            v = np.array([r_pow(a, b) for a, b in zip(x.reshape(-1), y.reshape(-1))], dtype=np.float64).reshape(x.shape)
            return v, np.full(x.shape, ULPS, dtype=np.int8)
        else:
            raise ValueError(op)
    v = np.asarray(v, dtype=np.float64)
    cls = np.full(x.shape, EXACT, dtype=np.int8)
    cls[np.isnan(v)] = NAN_SIGN
    cls[np.isnan(v) & nx & ny] = ANY_NAN
    return v, cls


def _math(op, x):
    with np.errstate(all="ignore"):
        if op == "abs":
            return np.abs(x), None
        if op == "sign":
            return np.where(np.isnan(x), x, np.where(x > 0, 1.0, np.where(x < 0, -1.0, 0.0))), None
        if op in ULPS_MATH:
            f = r_log1p if op == "log1p" else r_expm1
            return (np.array([f(a) for a in x.reshape(-1)], dtype=np.float64).reshape(x.shape),
                    np.full(x.shape, ULPS, dtype=np.int8))
        v = {"sqrt": np.sqrt, "floor": np.floor, "ceiling": np.ceil, "trunc": np.trunc}[op](x)
    cls = np.full(x.shape, EXACT, dtype=np.int8)
    cls[np.isnan(v)] = NAN_SIGN
    return v, cls


class Expected:
    """dense values, their comparison classes, the stored mask, the result's type, the overflow flag, and for the ULPS
    class the mask of the elements whose operand was NA"""

    def __init__(self, type, dense, cls, stored, overflow=False, from_na=None):
        self.type, self.overflow = type, bool(overflow)
        self.dense = np.asfortranarray(dense, dtype=sc.NP_DTYPE[type])
        self.cls = np.asfortranarray(np.zeros(dense.shape, np.int8) if cls is None else cls)
        nonzero = (self.dense != 0) | (np.isnan(self.dense) if type == "double" else False)
        self.stored = np.asfortranarray(stored & nonzero)
        self.from_na = np.asfortranarray(np.zeros(dense.shape, bool) if from_na is None else from_na)
        for a in (self.dense, self.cls, self.stored, self.from_na):
            a.setflags(write=False)


def dense_nd(x):
    """(dense, stored) of an object of any dimension, shaped nrow x leaves"""
    flat = SVT_SparseArray((x.dim[0], len(x.leaves)), x.type, x.leaves, na_background=x.na_background)
    return sc.dense_and_stored(flat)


def expect_merge(op, x, y):
    dx, sx = dense_nd(x)
    dy, sy = dense_nd(y)
    t = out_type("merge", op, x.type, y.type)
    if t == "integer":
        v, over = _int_arith(op, dx, dy)
        return Expected(t, v, None, sx | sy, over)
    v, cls = _double_arith(op, as_double(dx), as_double(dy))
    return Expected(t, v, cls, sx | sy)


def expect_scalar(op, x, s, s_type):
    dx, sx = dense_nd(x)
    t = out_type("scalar", op, x.type, s_type)
    if t == "integer":
        v, over = _int_arith(op, dx, np.int32(s))
        return Expected(t, v, None, sx, over)
    xd = as_double(dx)
    v, cls = _double_arith(op, xd, np.float64(s))
    return Expected(t, v, cls, sx, from_na=is_NA_real(xd))


def expect_neg(x):
    dx, sx = dense_nd(x)
    if x.type == "integer":
        return Expected("integer", np.where(dx == NA_integer, NA_integer, -dx.astype(np.int64)).astype(np.int32), None, sx)
    return Expected("double", np.negative(dx), None, sx)


def expect_math(op, x):
    dx, sx = dense_nd(x)
    v, cls = _math(op, dx)
    return Expected("double", v, cls, sx, from_na=is_NA_real(dx))


def ulp_distance(got, want):
    """how many representable doubles lie between got and want (finite or infinite, not NaN), element-wise"""
    def ordered(a):
        b = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
        return np.where(b < 0, np.int64(-2 ** 63) - b, b).astype(object)
    return np.abs(ordered(got) - ordered(want))


def compare(got_dense, got_stored, want: Expected, what="", max_ulps=0):
    """asserts the comparison of the module docstring; returns the largest ULPS distance seen (0 without that class)"""
    assert got_dense.dtype == want.dense.dtype, f"{what}: dtype {got_dense.dtype}"
    assert got_dense.shape == want.dense.shape, f"{what}: shape {got_dense.shape}, want {want.dense.shape}"
    assert np.array_equal(got_stored, want.stored), \
        f"{what}: the stored entries differ at {np.argwhere(got_stored != want.stored)[:5].tolist()}"
    at = want.stored
    g, w, cls = got_dense[at], want.dense[at], want.cls[at]
    gb, wb = sc.bits(g), sc.bits(w)
    m = cls == EXACT
    assert np.array_equal(gb[m], wb[m]), f"{what}: values differ as bits at {np.flatnonzero(m & (gb != wb))[:5].tolist()}"
    worst = 0
    if want.type == "double":
        m = cls == NAN_SIGN
        assert np.array_equal(gb[m] & ~SIGN, wb[m] & ~SIGN), f"{what}: NaN payloads differ: {gb[m][:4]}, want {wb[m][:4]}"
        m = cls == ANY_NAN
        assert np.all(np.isnan(g[m])), f"{what}: not NaN where two NaNs met"
        m = cls == ULPS
        if m.any():
            wn = np.isnan(w[m])
            assert np.array_equal(np.isnan(g[m]), wn), f"{what}: NaN where a number is due, or the reverse"
            na = want.from_na[at][m]
            assert np.array_equal(is_NA_real(g[m])[na], np.ones(int(na.sum()), bool)), f"{what}: an NA did not stay NA"
            d = ulp_distance(g[m][~wn], w[m][~wn])
            worst = int(d.max()) if d.size else 0
            assert worst <= max_ulps, f"{what}: {worst} ulps from the correctly rounded value, the bound is {max_ulps}"
    return worst


def check_result(res, x, want: Expected, what="", max_ulps=0):
    """a Session result against the expectation; the leaf invariants of subset_cases"""
    assert isinstance(res, SVT_SparseArray) and res.dim == x.dim and res.type == want.type and not res.na_background, what
    for lf in res.leaves:
        if lf is None:
            continue
        offs = np.asarray(lf[0])
        assert offs.size > 0 and offs.dtype == np.int32 and lf[1] is not None and len(lf[1]) == offs.size, what
        assert offs[0] >= 0 and offs[-1] < res.dim[0] and np.all(np.diff(offs) > 0), f"{what}: rows do not ascend"
    got, got_stored = dense_nd(res)
    return compare(got, got_stored, want, what, max_ulps)


# ---------------------------------------------------------------------------
# shared operands (small; through the host entry points)
# ---------------------------------------------------------------------------
def _mask(dim, density, seed, empty_cols=()):
    m = np.random.default_rng(seed).random(dim) < density
    m[:, list(empty_cols)] = False
    return m


DIM = (41, 29)
_OPERANDS = {
    # two patterns that overlap in part, columns 3, 4 and 20 empty in one, 4 and 11 in the other
    "d1": lambda: sc.build(DIM, "double", _mask(DIM, 0.3, 1, (3, 4, 20))),
    "d2": lambda: sc.build(DIM, "double", _mask(DIM, 0.3, 2, (4, 11))),
    "i1": lambda: sc.build(DIM, "integer", _mask(DIM, 0.3, 3, (3, 4, 20))),
    "i2": lambda: sc.build(DIM, "integer", _mask(DIM, 0.3, 4, (4, 11))),
    "d1s": lambda: sc.build(DIM, "double", _mask(DIM, 0.4, 5), "specials"),
    "d2s": lambda: sc.build(DIM, "double", _mask(DIM, 0.4, 6, (0,)), "specials"),
    "i1s": lambda: sc.build(DIM, "integer", _mask(DIM, 0.4, 7), "specials"),
    "i2s": lambda: sc.build(DIM, "integer", _mask(DIM, 0.4, 8, (0,)), "specials"),
    # lacunar leaves (all ones, stored without values) on either side
    "d1l": lambda: sc.build(DIM, "double", _mask(DIM, 0.3, 1, (3, 4, 20)), lacunar_cols=(0, 5, 6, 28)),
    "i2l": lambda: sc.build(DIM, "integer", _mask(DIM, 0.3, 4, (4, 11)), lacunar_cols=(5, 7, 28)),
    "d_empty": lambda: sc.build(DIM, "double", np.zeros(DIM, bool)),
    "i_empty": lambda: sc.build(DIM, "integer", np.zeros(DIM, bool)),
    "d_ncol0": lambda: sc.build((7, 0), "double", np.zeros((7, 0), bool)),
    "d_nrow0": lambda: sc.build((0, 5), "double", np.zeros((0, 5), bool)),
    # the pattern of d1 with other values, and a pattern that shares no position with d1
    "d1_other_values": lambda: sc.build(DIM, "double", _mask(DIM, 0.3, 1, (3, 4, 20)), "specials"),
    "d_disjoint_from_d1": lambda: sc.build(DIM, "double", ~_mask(DIM, 0.3, 1, (3, 4, 20)) & _mask(DIM, 0.3, 9)),
    "d_disjoint_from_d1s": lambda: sc.build(DIM, "double", ~_mask(DIM, 0.4, 5) & _mask(DIM, 0.5, 10)),
    "d3d": lambda: SVT_SparseArray.from_dense(np.where(_mask((9, 5, 4), 0.4, 11), np.arange(1.0, 181.0).reshape(9, 5, 4), 0.0)),
    "d3d_2": lambda: SVT_SparseArray.from_dense(np.where(_mask((9, 5, 4), 0.4, 12), -np.arange(1.0, 181.0).reshape(9, 5, 4), 0.0)),
    "i3d": lambda: SVT_SparseArray.from_dense(np.where(_mask((9, 5, 4), 0.4, 13), np.arange(1, 181).reshape(9, 5, 4), 0)
                                              .astype(np.int32)),
    # integers whose sums, differences and products leave (INT_MIN, INT_MAX]
    "i_big1": lambda: _from_values(DIM, "integer", _mask(DIM, 0.5, 14), [INT_MAX, -INT_MAX, 65536, 3, INT_MAX - 1, 46341]),
    "i_big2": lambda: _from_values(DIM, "integer", _mask(DIM, 0.5, 15), [1, -1, 65536, INT_MAX, -2, 46341, 2]),
    # doubles that underflow under * 1e-320, next to some that do not
    "d_small": lambda: _from_values(DIM, "double", _mask(DIM, 0.3, 16), [1e-5, 1.0, -3e-4, 2.5e3, 1e10, -1e-10, 4e-324]),
    "d_mixed_sign": lambda: _from_values(DIM, "double", _mask(DIM, 0.4, 17),
                                         [-7.5, 7.5, 3.0, -3.0, 0.5, -0.5, 1e300, -1e300, 2.0, 9.0, -8.0, 1.0, 0.25, 6.0]),
    "i_mixed_sign": lambda: _from_values(DIM, "integer", _mask(DIM, 0.4, 18), [-7, 7, 3, -3, 6, -6, 1, -1, 100, -100, 9]),
}


def _from_values(dim, type, mask, values):
    """an object with the entries of ``mask`` stored and ``values`` cycled over them"""
    x = sc.build(dim, type, mask)
    table, k, leaves = np.asarray(values, dtype=sc.NP_DTYPE[type]), 0, []
    for lf in x.leaves:
        if lf is None:
            leaves.append(None)
            continue
        leaves.append((lf[0], np.ascontiguousarray(table[(k + np.arange(lf[0].size)) % table.size])))
        k += lf[0].size
    return SVT_SparseArray(dim, type, leaves)


@functools.lru_cache(maxsize=None)
def operand(name):
    return _OPERANDS[name]()


# (name, x, y, ops): x op y through Session.arith
MERGE_CASES = [
    ("double_double", "d1", "d2", MERGE_OPS),
    ("int_int", "i1", "i2", MERGE_OPS),
    ("int_double", "i1", "d2", MERGE_OPS),
    ("double_int", "d1", "i2", MERGE_OPS),
    ("specials_double_double", "d1s", "d2s", MERGE_OPS),
    ("specials_int_int", "i1s", "i2s", MERGE_OPS),
    ("specials_int_double", "i1s", "d2s", MERGE_OPS),
    ("specials_double_int", "d1s", "i2s", MERGE_OPS),
    ("lacunar_both_sides", "d1l", "i2l", MERGE_OPS),
    ("lacunar_left", "d1l", "d2", MERGE_OPS),
    ("empty_left", "d_empty", "d2", MERGE_OPS),
    ("empty_right", "i1", "i_empty", MERGE_OPS),
    ("empty_both", "d_empty", "i_empty", MERGE_OPS),
    ("ncol_0", "d_ncol0", "d_ncol0", MERGE_OPS),
    ("nrow_0", "d_nrow0", "d_nrow0", MERGE_OPS),
    ("three_dimensions", "d3d", "d3d_2", MERGE_OPS),
    ("three_dimensions_int_double", "i3d", "d3d", MERGE_OPS),
    ("identical_operands", "d1", "d1", MERGE_OPS),                     # x - x: an empty result
    ("identical_patterns", "d1", "d1_other_values", MERGE_OPS),
    ("disjoint_patterns", "d1", "d_disjoint_from_d1", MERGE_OPS),
    ("only_nan_and_inf_survive_an_implicit_zero", "d1s", "d_disjoint_from_d1s", ("*",)),
    ("int_overflow", "i_big1", "i_big2", MERGE_OPS),
]
MERGE_PARAMS = [(c[0], op) for c in MERGE_CASES for op in c[3]]
MERGE_BY_NAME = {c[0]: c for c in MERGE_CASES}

# (name, x, op, scalar, its R type): x op s through Session.arith
SCALAR_CASES = (
    [(f"{x}_{op}_{st}", x, op, s, st) for x in ("d1", "i1", "d1s", "i1s", "d1l", "d_mixed_sign", "i_mixed_sign")
     for op in SCALAR_OPS for s, st in ((3, "integer"), (2.5, "double"))] +
    [("pow_inf", "d_mixed_sign", "^", np.inf, "double"), ("pow_inf_int", "i_mixed_sign", "^", np.inf, "double"),
     ("pow_inf_specials", "d1s", "^", np.inf, "double"),
     ("mod_minus_3", "d_mixed_sign", "%%", -3, "integer"), ("mod_minus_3_int", "i_mixed_sign", "%%", -3, "integer"),
     ("mod_minus_3_specials", "d1s", "%%", -3.0, "double"), ("idiv_minus_3_int", "i_mixed_sign", "%/%", -3, "integer"),
     ("idiv_minus_3", "d_mixed_sign", "%/%", -3.0, "double"),
     ("mod_inf", "d_mixed_sign", "%%", np.inf, "double"), ("mod_minus_inf", "d1s", "%%", -np.inf, "double"),
     ("idiv_inf", "d_mixed_sign", "%/%", np.inf, "double"), ("idiv_minus_inf", "d1s", "%/%", -np.inf, "double"),
     ("times_0", "d1s", "*", 0.0, "double"), ("times_0_int", "i1s", "*", 0, "integer"),
     ("times_0_int_by_double", "i1s", "*", 0.0, "double"), ("times_0_no_specials", "d1", "*", 0, "integer"),
     ("times_1e-320_underflow", "d_small", "*", 1e-320, "double"),
     ("int_overflow", "i_big1", "*", 3, "integer"), ("int_big_mod", "i_big1", "%%", 7, "integer"),
     ("div_by_minus_small", "d1s", "/", -4e-324, "double"),
     ("empty", "d_empty", "*", 2.0, "double"), ("ncol_0", "d_ncol0", "/", 2.0, "double"),
     ("three_dimensions", "i3d", "%/%", 7, "integer")])
SCALAR_NAMES = [c[0] for c in SCALAR_CASES]
SCALAR_BY_NAME = {c[0]: c for c in SCALAR_CASES}
assert len(SCALAR_BY_NAME) == len(SCALAR_CASES)

NEG_OPERANDS = ("d1", "i1", "d1s", "i1s", "d1l", "i2l", "d_empty", "d3d", "i3d")
MATH_OPERANDS = ("d1", "d1s", "d_mixed_sign", "d1l", "d_empty", "d3d")

# The fixed inputs of the three functions compared in ulps: denormals, values near -1 (log1p), near 0, large values,
# the specials.  One column each; the pow list is met with the exponents of POW_EXPONENTS.
_DEN = [4.9406564584124654e-324, -4.9406564584124654e-324, 2.2250738585072009e-308, -1.5e-310, 1e-320]
_NEAR0 = [1e-300, -1e-300, 1e-17, -1e-17, 1e-9, -1e-9, 3e-5, -3e-5, 0.001, -0.001, 0.1, -0.1, 0.5, -0.5]
_SPEC = [NA_real, float("nan"), np.inf, -np.inf, -0.0, 0.0]
ULPS_INPUTS = {
    "log1p": _DEN + _NEAR0 + [-1.0, -1.0 + 2.0 ** -52, -0.9999999999, -0.999, -0.75, -1.5, -1e300, 1.0, 2.0, 1.7182818284590452,
                              10.0, 1e5, 1e10, 1e100, 1.7976931348623157e308] + _SPEC,
    "expm1": _DEN + _NEAR0 + [-1.0, 1.0, 0.6931471805599453, -0.6931471805599453, 5.0, -5.0, 36.0, -36.0, -38.0, 100.0, -100.0,
                              709.0, 709.782712893384, 710.0, -745.0, -1e300, 1e300] + _SPEC,
    "^": _DEN + _NEAR0 + [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 10.0, 0.9999999999999999, 1.0000000000000002, 1e5, -1e5, 1e100,
                          1e154, 1.3407807929942596e154, 1e300, -1e300, 1.7976931348623157e308] + _SPEC,
}
POW_EXPONENTS = [(2, "integer"), (3, "integer"), (0.5, "double"), (2.5, "double"), (1e-3, "double"), (17.0, "double"),
                 (1074.0, "double"), (np.inf, "double")]


@functools.lru_cache(maxsize=None)
def ulps_operand(fn):
    """the inputs of ``fn`` as a one-column object, every one of them stored (the zeros too)"""
    v = np.array(ULPS_INPUTS[fn], dtype=np.float64)
    return SVT_SparseArray((v.size, 1), "double", [(np.arange(v.size, dtype=np.int32), v)])


# ---------------------------------------------------------------------------
# device level: operands placed around the tile T, as CSC triples over LINEAR positions column * nrow + row
# ---------------------------------------------------------------------------
def merged_places(kx, ky):
    """The merged sequence of two ascending key arrays, x's entry first on equal keys, by numpy's stable sort: (keys of
    the merged places, side of every place: 0 = x, 1 = y)."""
    keys = np.concatenate([kx, ky])
    side = np.concatenate([np.zeros(kx.size, np.int8), np.ones(ky.size, np.int8)])
    order = np.lexsort((side, keys))
    return keys[order], side[order]


def _csc(keys, vals, nrow, ncol):
    keys = np.asarray(keys, dtype=np.int64)
    cp = np.zeros(ncol + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // nrow, minlength=ncol), out=cp[1:])
    return cp, (keys % nrow).astype(np.int32), np.ascontiguousarray(vals)


class DeviceCase:
    """x op y on (nrow, ncol) from linear keys; .x / .y: (col_ptr, row_idx, val); .want: the result's CSC triple by
    numpy on the union of the stored positions."""

    def __init__(self, nrow, ncol, kx, vx, ky, vy, op, pairs_at=()):
        self.nrow, self.ncol, self.op, self.pairs_at = int(nrow), int(ncol), op, tuple(pairs_at)
        self.kx, self.ky = np.asarray(kx, np.int64), np.asarray(ky, np.int64)
        assert np.all(np.diff(self.kx) > 0) and np.all(np.diff(self.ky) > 0)
        assert (self.kx.size == 0 or self.kx[-1] < nrow * ncol) and (self.ky.size == 0 or self.ky[-1] < nrow * ncol)
        self.vx, self.vy = np.asarray(vx), np.asarray(vy)
        self.x, self.y = _csc(self.kx, self.vx, nrow, ncol), _csc(self.ky, self.vy, nrow, ncol)

    @property
    def merged_length(self):
        return self.kx.size + self.ky.size

    @functools.cached_property
    def want(self):
        keys = np.union1d(self.kx, self.ky)
        t = "integer" if self.vx.dtype == np.int32 and self.vy.dtype == np.int32 else "double"
        dx = np.zeros(keys.size, dtype=self.vx.dtype)
        dy = np.zeros(keys.size, dtype=self.vy.dtype)
        dx[np.searchsorted(keys, self.kx)] = self.vx
        dy[np.searchsorted(keys, self.ky)] = self.vy
        if t == "integer":
            v, self.overflow = _int_arith(self.op, dx, dy)
            cls = np.zeros(keys.size, np.int8)
        else:
            (v, cls), self.overflow = _double_arith(self.op, as_double(dx), as_double(dy)), False
        keep = (v != 0) | (np.isnan(v) if t == "double" else False)
        self.cls = cls[keep]
        return _csc(keys[keep], v[keep], self.nrow, self.ncol)


def _vals(n, seed, type="double"):
    """values that never cancel by accident: distinct magnitudes, both signs"""
    rng = np.random.default_rng(seed)
    if type == "integer":
        return (rng.integers(1, 1000, size=n) * rng.choice([-1, 1], size=n)).astype(np.int32)
    return np.round(rng.uniform(1.0, 100.0, size=n), 3) * rng.choice([-1.0, 1.0], size=n)


def _straddling(T, nrow, ncol, op, cancel):
    """x holds the linear positions 0 .. 2T+10, y the positions T-1 and 2T-2: the pairs sit at the merged places
    (T-1, T) and (2T-1, 2T).  cancel: the pairs' results are zero (op "-": equal values)."""
    kx = np.arange(2 * T + 11)
    ky = np.array([T - 1, 2 * T - 2])
    vx = _vals(kx.size, 21)
    vy = vx[ky].copy() if cancel else _vals(2, 22)
    return DeviceCase(nrow, ncol, kx, vx, ky, vy, op, pairs_at=(T - 1, 2 * T - 1))


def _tile_exact(T, length, op):
    """a merged sequence of exactly ``length`` places: x takes two thirds, y the rest, a third of y's keys are x's too"""
    nx = (2 * length) // 3
    ny = length - nx
    rng = np.random.default_rng(length)
    kx = np.sort(rng.choice(4 * T, size=nx, replace=False))
    shared = rng.choice(kx, size=min(ny // 3, nx), replace=False)
    free = np.setdiff1d(np.arange(4 * T), kx)
    ky = np.sort(np.concatenate([shared, rng.choice(free, size=ny - shared.size, replace=False)]))
    return DeviceCase(97, (4 * T) // 97 + 1, kx, _vals(nx, 23), ky, _vals(ny, 24), op)


@functools.lru_cache(maxsize=None)
def device_cases(T):
    rng = np.random.default_rng(31)
    cases = {}
    # one column holding everything, nrow > 3 T
    nrow = 3 * T + 17
    kx = np.sort(rng.choice(nrow, size=T + T // 2, replace=False))
    ky = np.sort(rng.choice(nrow, size=T + T // 3, replace=False))
    cases["one_column_holds_everything"] = DeviceCase(nrow, 1, kx, _vals(kx.size, 1), ky, _vals(ky.size, 2), "+")
    cases["one_column_times"] = DeviceCase(nrow, 1, kx, _vals(kx.size, 1), ky, _vals(ky.size, 2), "*")
    # 100 000 empty columns around a handful of entries
    ncol, nrow = 100_003, 11
    kx = np.array([0, 5, 50_000 * 11 + 3, 50_000 * 11 + 4, 100_002 * 11 + 10])
    ky = np.array([5, 6, 50_000 * 11 + 4, 70_000 * 11, 100_002 * 11 + 10])
    cases["100000_empty_columns"] = DeviceCase(nrow, ncol, kx, _vals(5, 3), ky, _vals(5, 4), "-")
    # the straddling pairs: in one long column, and spread over columns of 50 rows
    cases["straddling_pairs_one_column"] = _straddling(T, 2 * T + 11, 1, "+", False)
    cases["straddling_pairs_columns"] = _straddling(T, 50, (2 * T + 11) // 50 + 1, "*", False)
    cases["straddling_pairs_cancel"] = _straddling(T, 50, (2 * T + 11) // 50 + 1, "-", True)
    for length in (T - 1, T, T + 1, 2 * T):
        cases[f"merged_length_{length - T:+d}_from_T" if length != 2 * T else "merged_length_2T"] = _tile_exact(T, length, "+")
    # a tile in which every entry cancels: the first T merged places are T/2 equal pairs, what follows differs
    k = np.arange(T // 2 + 300)
    vx = _vals(k.size, 5)
    vy = vx.copy()
    vy[T // 2:] *= 2.0
    cases["a_tile_cancels"] = DeviceCase(64, k.size // 64 + 1, k, vx, k, vy, "-")
    # all-match operands: the same pattern, other values; and the same shifted by one unmatched entry, which puts
    # every pair across an odd / even place -- across the threads' runs of 8
    k = np.sort(rng.choice(3 * T, size=T + 100, replace=False))
    cases["all_match"] = DeviceCase(61, (3 * T) // 61 + 1, k, _vals(k.size, 6), k, _vals(k.size, 7), "+")
    k1 = np.arange(1, T + 200)
    cases["all_match_shifted"] = DeviceCase(61, (T + 200) // 61 + 1, np.arange(0, T + 200), _vals(T + 200, 8), k1,
                                            _vals(k1.size, 9), "*")
    cases["all_match_int"] = DeviceCase(61, (3 * T) // 61 + 1, k, _vals(k.size, 10, "integer"), k,
                                        _vals(k.size, 11, "integer"), "*")
    cases["int_double"] = DeviceCase(61, (3 * T) // 61 + 1, k, _vals(k.size, 12, "integer"), k1, _vals(k1.size, 13), "-")
    cases["empty_x"] = DeviceCase(61, 40, np.zeros(0, np.int64), np.zeros(0), k1[k1 < 61 * 40], _vals(int((k1 < 61 * 40).sum()), 14), "-")
    cases["empty_both"] = DeviceCase(61, 40, np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), np.zeros(0), "+")
    return cases


DEVICE_NAMES = list(device_cases(2048))
