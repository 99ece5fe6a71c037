"""Values, operands and expectations for pmin() / pmax() and is.na() / is.nan() / is.infinite() on sparse operands, shared
by tests/test_zzzzzzz_pminmax_cpu.py (the builder's own proofs, the rule program, the step-by-step emulation of the
reference's .pminmax2, the Session's checks) and tests/test_zzzzzzz_pminmax_hip.py (the device kernels and the host entry
points).

THE EXPECTATION is the closed formula of the rule on dense numpy arrays, selected on BITS (``_select`` works on the
uint64 / int32 view, so a NaN keeps its payload and NA_real_ stays NA_real_):

    na_rm False:  isna(x) ? x : isna(y) ? y : (y < x ? y : x)        (pmax: y > x)
    na_rm True:   isna(y) ? x : isna(x) ? y : (y < x ? y : x)

on both sides widened to the wider type (logical < integer < double; NA_integer_ becomes NA_real_).  A position is stored
in the result exactly when it is stored on either side and the result there is not ``== 0``.  ``steps`` is the other
statement: the five steps of .pminmax2 (compare, nzwhich, assign, is.na, restore) by index assignment.
"""
from __future__ import annotations

import functools

import numpy as np

import arith_cases as ac
import compare_cases as cc
import sweep_cases as sw
from sparsearray_amd import NA_integer, NA_real

OPS = ("pmin", "pmax")
TYPES = ("logical", "integer", "double")
ISFUNS = ("is.na", "is.nan", "is.infinite")
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]      # a NaN that is not R_NaN
DBL_MAX = np.finfo(np.float64).max
INT_MAX = 2 ** 31 - 1

# the value table: zeros of both signs, ordinary values, the extremes, a NaN with a payload, NA
TABLE = {"double": np.array([0.0, -0.0, 1.5, -2.0, DBL_MAX, np.inf, -np.inf, NAN_PAYLOAD, NA_real]),
         "integer": np.array([0, 1, -7, INT_MAX, NA_integer], dtype=np.int32),
         "logical": np.array([0, 1, NA_integer], dtype=np.int32)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def out_type(tx, ty):
    return TYPES[max(TYPES.index(tx), TYPES.index(ty))]


def np_dtype(t):
    return np.float64 if t == "double" else np.int32


def isna(a):
    return np.isnan(a) if a.dtype == np.float64 else a == NA_integer


def widen(a, t):
    """the values in the result's type: int32 -> float64 converts, NA_integer_ becomes NA_real_"""
    a = np.asarray(a)
    if t != "double" or a.dtype == np.float64:
        return a.astype(np_dtype(t), copy=True)
    return ac.as_double(a)


def _select(mask, a, b):
    """np.where on the bit patterns"""
    return np.where(mask, bits(a), bits(b)).view(a.dtype)


def formula(op, na_rm, x, y):
    """the closed formula on two arrays of the result's type"""
    assert x.dtype == y.dtype and op in OPS
    with np.errstate(invalid="ignore"):
        take_y = (y < x) if op == "pmin" else (y > x)
    plain = _select(take_y, y, x)
    if na_rm:
        return _select(isna(y), x, _select(isna(x), y, plain))
    return _select(isna(x), x, _select(isna(y), y, plain))


def steps(op, na_rm, x, y, t):
    """.pminmax2 step by step on dense 1-D arrays of the operands' own types ``x`` and ``y``; ``t`` the result's type"""
    cmp = cc.compare_values("<" if op == "pmin" else ">", y, x)          # op(y, x): 0, 1 or NA
    replace_idx = np.flatnonzero(cmp != 0)                                   # nzwhich(): an NA is not a zero
    ans = widen(x, t)                                                        # ans <- x; the assignment sets the type
    ans[replace_idx] = widen(y, t)[replace_idx]                              # ans[replace_idx] <- y[replace_idx]
    is_na = isna(y) if na_rm else isna(x)
    restore_idx = np.flatnonzero(is_na)                                      # nzwhich(is_na)
    ans[restore_idx] = widen(x, t)[restore_idx]                              # ans[restore_idx] <- x[restore_idx]
    return ans


def isfun_values(fn, v):
    """int32 1 / 0"""
    if v.dtype != np.float64:
        return ((v == NA_integer) if fn == "is.na" else np.zeros(v.shape, bool)).astype(np.int32)
    if fn == "is.na":
        return np.isnan(v).astype(np.int32)
    if fn == "is.nan":
        return (np.isnan(v) & ((bits(v) & np.uint64(0xFFFFFFFF)) != np.uint64(1954))).astype(np.int32)
    return np.isinf(v).astype(np.int32)


def keeps_sparse(op, s, s_type):
    """pmin(0, s) == 0"""
    if (s_type == "double" and np.isnan(s)) or (s_type != "double" and int(s) == NA_integer):
        return False
    return bool(s >= 0) if op == "pmin" else bool(s <= 0)


def kept(v):
    return (v != 0) | (np.isnan(v) if v.dtype == np.float64 else False)


# ---------------------------------------------------------------------------
# expectations on CSC triples
# ---------------------------------------------------------------------------
def expect_merge(op, na_rm, nrow, ncol, kx, vx, tx, ky, vy, ty):
    """((col_ptr, row_idx, val), type) of pmin / pmax of two operands given by ascending linear keys"""
    t = out_type(tx, ty)
    keys = np.union1d(kx, ky)
    dx, dy = np.zeros(keys.size, dtype=vx.dtype), np.zeros(keys.size, dtype=vy.dtype)
    dx[np.searchsorted(keys, kx)] = vx
    dy[np.searchsorted(keys, ky)] = vy
    v = formula(op, na_rm, widen(dx, t), widen(dy, t))
    keep = kept(v)
    return ac._csc(keys[keep], v[keep], nrow, ncol), t


def _filter(cp, ri, v):
    ncol = cp.size - 1
    col = np.repeat(np.arange(ncol), np.diff(cp))
    keep = kept(v)
    out_cp = np.zeros(ncol + 1, np.int64)
    np.cumsum(np.bincount(col[keep], minlength=ncol), out=out_cp[1:])
    return out_cp, ri[keep], v[keep]


def expect_map(op, na_rm, csc, tx, s, s_type):
    cp, ri, val = csc
    t = out_type(tx, s_type)
    y = widen(np.full(val.shape, s, dtype=np_dtype(s_type)), t)
    return _filter(cp, ri, formula(op, na_rm, widen(val, t), y)), t


def expect_sweep(op, na_rm, csc, tx, dim, margin, stats, s_type):
    cp, ri, val = csc
    t = out_type(tx, s_type)
    col = np.repeat(np.arange(cp.size - 1), np.diff(cp))
    s = np.asarray(stats).reshape(-1, order="F")[sw.index_of(dim, margin)[ri, col]]
    return _filter(cp, ri, formula(op, na_rm, widen(val, t), widen(s, t))), t


def expect_isfun(fn, csc):
    cp, ri, val = csc
    return _filter(cp, ri, isfun_values(fn, val))


def same(got, want, what):
    """CSC triples bit for bit: col_ptr, row_idx and the values as integers"""
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    assert got[2].dtype == want[2].dtype, f"{what}: {got[2].dtype} values, expected {want[2].dtype}"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{what}: values"


# ---------------------------------------------------------------------------
# the value table as one small operand pair
# ---------------------------------------------------------------------------
def table_pair(tx, ty):
    """(nrow, ncol, kx, vx, ky, vy): cell (i, j) of the first len(Y) columns holds X[i] on x's side and Y[j] on y's, so
    every combination is a cell; one more column is stored by x alone and one by y alone (the other side an implicit
    zero); a last column is stored by neither."""
    X, Y = TABLE[tx], TABLE[ty]
    n, m = X.size, Y.size
    nrow, ncol = max(n, m), m + 3
    kx = np.concatenate([j * nrow + np.arange(n) for j in range(m + 1)])
    vx = np.tile(X, m + 1)
    ky = np.concatenate([j * nrow + np.arange(n) for j in range(m)] + [(m + 1) * nrow + np.arange(m)])
    vy = np.concatenate([np.repeat(Y, n), Y])
    return nrow, ncol, kx.astype(np.int64), vx, ky.astype(np.int64), vy


# ---------------------------------------------------------------------------
# placement around the tile T
# ---------------------------------------------------------------------------
def tracer(n, t, seed, specials=True):
    """distinct magnitudes, both signs, never 0; ``specials``: NA (and NaN for doubles) on every 37th entry"""
    rng = np.random.default_rng(seed)
    if t == "double":
        v = (np.arange(n) * 0.5 + 1.25) * rng.choice([-1.0, 1.0], size=n)
        if specials:
            v[5::37] = NA_real
            v[11::74] = NAN_PAYLOAD
    else:
        v = ((np.arange(n) % 997 + 1) * rng.choice([-1, 1], size=n)).astype(np.int32)
        if t == "logical":
            v = (v > 0).astype(np.int32)
        if specials:
            v[5::37] = NA_integer
    return v


@functools.lru_cache(maxsize=None)
def placement_keys(T):
    """(nrow, ncol, kx, ky) of a pair whose merged sequence has 3T + 5 places: an empty first leaf; short leaves of three
    places (x, y, x on rows 1, 2, 4) up to place T - 1, so that the boundary T falls strictly inside the next one; 300
    empty leaves at place T + 2; one long leaf of 2T + 1 places -- a place per row, x on the even rows and y on the odd
    ones, holding the boundary 2T, but for the row that both sides store, whose x entry is place 3T - 1 and whose y entry
    place 3T: the pair straddles the boundary; a leaf of two places; an empty last leaf."""
    nrow = 2 * T + 64
    kx, ky, leaf, places = [], [], 1, 0
    lead = (T - 1) % 3
    if lead:                                                # a leaf of one or two x entries, so that 3 divides the rest
        kx += [leaf * nrow + r for r in range(lead)]
        leaf, places = leaf + 1, places + lead
    while places < T + 2:
        kx += [leaf * nrow + 1, leaf * nrow + 4]
        ky += [leaf * nrow + 2]
        leaf, places = leaf + 1, places + 3
    assert places == T + 2
    leaf += 300
    long_leaf, row = leaf, 0
    while places < 3 * T + 3:
        if places == 3 * T - 1:
            kx.append(leaf * nrow + row)
            ky.append(leaf * nrow + row)
            places += 2
        else:
            (kx if row % 2 == 0 else ky).append(leaf * nrow + row)
            places += 1
        row += 1
    assert row <= nrow
    leaf += 1
    kx.append(leaf * nrow + 7)
    ky.append(leaf * nrow + 9)
    ncol = leaf + 2
    return nrow, ncol, np.array(kx, np.int64), np.array(ky, np.int64), long_leaf


@functools.lru_cache(maxsize=None)
def placement_pair(T, tx, ty):
    nrow, ncol, kx, ky, _ = placement_keys(T)
    vx, vy = tracer(kx.size, tx, 41), tracer(ky.size, ty, 42)
    if tx != "logical":
        vx[3::50] = 0                                       # stored zeros are ordinary values
    return nrow, ncol, kx, vx, ky, vy


def small_pairs(T):
    """name -> (nrow, ncol, kx, vx, ky, vy) for the empty shapes and an N-d operand (2 x 3 x 2: six leaves of two rows)"""
    nrow, ncol, kx, ky, _ = placement_keys(T)
    some = kx[kx < 40 * nrow]
    none = np.zeros(0, np.int64)
    nd = np.array([0, 1, 3, 4, 6, 9, 11], np.int64)
    return {"x_empty": (nrow, 40, none, np.zeros(0), some, tracer(some.size, "double", 43)),
            "y_empty": (nrow, 40, some, tracer(some.size, "double", 44), none, np.zeros(0)),
            "both_empty": (nrow, 40, none, np.zeros(0), none, np.zeros(0)),
            "ncol_0": (nrow, 0, none, np.zeros(0), none, np.zeros(0)),
            "nd_2x3x2": (2, 6, nd, tracer(nd.size, "double", 45, False), nd[1:] - 1, tracer(nd.size - 1, "double", 46, False))}


def random_pair(seed=7, nrow=300, ncol=60, n=3000):
    """a seeded pair of double operands, a few thousand entries each, NAs and NaNs sprinkled in, no stored zero and no
    -0.0; about a third of the cells of one are cells of the other"""
    rng = np.random.default_rng(seed)
    kx = np.sort(rng.choice(nrow * ncol, size=n, replace=False))
    shared = rng.choice(kx, size=n // 3, replace=False)
    free = np.setdiff1d(np.arange(nrow * ncol), kx)
    ky = np.sort(np.concatenate([shared, rng.choice(free, size=n - shared.size, replace=False)]))
    vals = []
    for k in range(2):
        v = np.round(rng.uniform(-50.0, 50.0, size=n), 2)
        v[v == 0] = 1.0
        v[rng.choice(n, size=40, replace=False)] = NA_real
        v[rng.choice(n, size=40, replace=False)] = NAN_PAYLOAD
        vals.append(v)
    return nrow, ncol, kx.astype(np.int64), vals[0], ky.astype(np.int64), vals[1]


def isfun_operand(T, t):
    """(nrow, (col_ptr, row_idx, val)): T + 300 entries in leaves of up to 700, the special values on both sides of the
    tile boundary"""
    lengths = [0, 700, 700, 0, 700, T + 300 - 2100, 0]
    cp, ri, val = sw.from_lengths(sw.NROW, lengths, "double" if t == "double" else "integer", 51, specials=False)
    table = ([NA_real, NAN_PAYLOAD, np.inf, -np.inf, 0.0, float("nan")] if t == "double" else [NA_integer, 0, 1])
    for k, spot in enumerate(list(range(3, 60, 5)) + list(range(T - 6, T + 6))):
        val[spot] = table[k % len(table)]
    if t == "logical":
        val = np.where(val == NA_integer, NA_integer, (val > 0).astype(np.int32)).astype(np.int32)
    return sw.NROW, (cp, ri, val)
