"""Operands, vectors and expectations for sweep(x, MARGIN, STATS, FUN) -- Arith and Compare between a sparse operand and
a vector with one element per row, per leaf or per row of a group of leaves -- shared by tests/test_zzzzzz_sweep_cpu.py
(the builder's own proofs, the Session's checks, the index derivation, the host predicates) and
tests/test_zzzzzz_sweep_hip.py (the device kernels and the host entry points).

THE EXPECTATION is R's definition of sweep() on the dense array: STATS, the column-major array of the margin's extents,
is broadcast along the margin with numpy (``index_of``: np.unravel_index of every cell, np.ravel_multi_index of its
margin coordinates) and the operator is applied element-wise by the rules of tests/arith_cases.py (``_int_arith``, the
double rules) and tests/compare_cases.py (``compare_values``).  A position is stored in the result exactly when it is
stored in the operand and the result there is not ``== 0``.  Values are compared as bits and the stored mask exactly,
under the classes of arith_cases (EXACT, NAN_SIGN, ANY_NAN).  The hand-built cases do not expect ``^`` here: its
yardstick is the correctly rounded power, and the sweep calls the very device function of the scalar map, against which
they compare it bit for bit instead.  ``element_results`` states it all the same, in the class ULPS, for the seeded
random cases of tests/random_cases.py.

Every vector built here holds a DISTINCT value at every index, so an element read from a wrong index changes bits.
"""
from __future__ import annotations

import functools

import numpy as np

import arith_cases as ac
import compare_cases as cc
from sparsearray_amd import NA_integer, NA_real

ARITH_OPS = ("*", "/", "^", "%%", "%/%")
COMPARE_OPS = tuple(cc.COMPARE_OPS)
MARGINS_4D = (1, 2, 3, 4, (1, 2), (2, 3), (3, 4), (2, 3, 4))
DIM_4D = (5, 4, 3, 2)


# ---------------------------------------------------------------------------
# the index and the expectation
# ---------------------------------------------------------------------------
def as_margin(margin):
    return (int(margin),) if np.ndim(margin) == 0 else tuple(int(k) for k in margin)


def index_of(dim, margin):
    """k[row, leaf]: the index into STATS (column-major over the margin's extents) of every cell of the array of
    extents ``dim``, shaped nrow x leaves -- by numpy's own coordinate functions"""
    dim, m = tuple(int(d) for d in dim), [k - 1 for k in as_margin(margin)]
    nrow, nleaves = dim[0], int(np.prod(dim[1:], dtype=np.int64))
    if nrow * nleaves == 0:
        return np.zeros((nrow, nleaves), np.int64)
    coords = np.unravel_index(np.arange(nrow * nleaves), dim, order="F")
    k = np.ravel_multi_index([coords[a] for a in m], [dim[a] for a in m], order="F")
    return k.reshape((nrow, nleaves), order="F")


def stats_length(dim, margin):
    return int(np.prod([dim[k - 1] for k in as_margin(margin)], dtype=np.int64))


def element_results(op, val, s, s_type):
    """x op s element-wise on 1-D arrays: (values, cls, kept, type of the result, overflow flag); ``^`` gives the
    correctly rounded power in the class ULPS of arith_cases (the seeded random cases hold it to MAX_ULPS["^"])"""
    x_type = "double" if val.dtype == np.float64 else "integer"
    if op in cc.COMPARE_OPS:
        v, cls, t, over = cc.compare_values(op, val, s), np.zeros(val.shape, np.int8), "logical", False
    else:
        t = ac.out_type("scalar", op, x_type, s_type)
        if t == "integer":
            (v, over), cls = ac._int_arith(op, val, s), np.zeros(val.shape, np.int8)
        else:
            (v, cls), over = ac._double_arith(op, ac.as_double(val), ac.as_double(np.asarray(s))), False
    kept = (v != 0) | (np.isnan(v) if v.dtype == np.float64 else False)
    return v, cls, kept, t, over


def expect_csc(op, nrow, csc, dim, margin, stats, s_type):
    """The result of the sweep on a CSC triple: ((col_ptr, row_idx, val), cls of the kept entries, type, overflow)."""
    cp, ri, val = csc
    ncol = cp.size - 1
    col = np.repeat(np.arange(ncol), np.diff(cp))
    k = index_of(dim, margin)[ri, col]
    v, cls, kept, t, over = element_results(op, val, np.asarray(stats).reshape(-1, order="F")[k], s_type)
    out_cp = np.zeros(ncol + 1, np.int64)
    np.cumsum(np.bincount(col[kept], minlength=ncol), out=out_cp[1:])
    return (out_cp, ri[kept], v[kept]), cls[kept], t, over


def expect_session(op, x, stats, s_type, margin):
    """The expectation for Session.sweep(x, margin, stats, op): an arith_cases.Expected, or a compare_cases.Expected."""
    dx, sx = ac.dense_nd(x)
    s = np.asarray(stats).reshape(-1, order="F")[index_of(x.dim, margin)]
    v, cls, _, t, over = element_results(op, dx.reshape(-1, order="F"), s.reshape(-1, order="F"), s_type)
    v, cls = v.reshape(dx.shape, order="F"), cls.reshape(dx.shape, order="F")
    return cc.Expected(v, sx) if t == "logical" else ac.Expected(t, v, cls, sx, over)


# ---------------------------------------------------------------------------
# vectors: a distinct value at every index, every one of them keeping the result sparse
# ---------------------------------------------------------------------------
def stats_for(op, n, s_type, seed=0):
    k = np.random.default_rng(1000 + seed).permutation(n)
    if op in cc.COMPARE_OPS:
        # 0 op s must be FALSE: == takes any s != 0, <= and < take negative ones, >= and > positive ones; != takes
        # s == 0 alone -- the one operator whose vector cannot hold distinct values
        sign = 0 if op == "!=" else -1 if op in ("<=", "<") else 1
        v = sign * (k + 1)
    else:
        v = k + 2
    if s_type == "integer":
        return v.astype(np.int32)
    return v.astype(np.float64) * 0.75 + (0.125 if op not in cc.COMPARE_OPS else 0.0)


# ---------------------------------------------------------------------------
# device level: CSC triples placed around the tile T
# ---------------------------------------------------------------------------
def _rows(rng, nrow, n):
    return np.sort(rng.choice(nrow, size=n, replace=False)).astype(np.int32)


def _values(n, type, seed):
    """tracer values, distinct in magnitude, both signs, never 0 or NA"""
    rng = np.random.default_rng(seed)
    if type == "integer":
        return ((np.arange(n) % 997 + 1) * rng.choice([-1, 1], size=n)).astype(np.int32)
    return (np.arange(n) * 0.5 + 1.25) * rng.choice([-1.0, 1.0], size=n)


def from_lengths(nrow, lengths, type, seed, specials=True):
    """(col_ptr, row_idx, val) with leaf q holding lengths[q] entries on seeded ascending rows; ``specials``: NaN, NA,
    +-Inf and a stored zero (NA and a stored zero for integers) put on fixed entries"""
    rng = np.random.default_rng(seed)
    cp = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=cp[1:])
    ri = np.concatenate([_rows(rng, nrow, n) for n in lengths] + [np.zeros(0, np.int32)]).astype(np.int32)
    val = _values(int(cp[-1]), type, seed + 1)
    if specials and val.size >= 64:
        spots = np.linspace(3, val.size - 4, 10).astype(int)
        table = ([NA_integer, 0] * 5 if type == "integer" else
                 [NA_real, float("nan"), np.inf, -np.inf, 0.0, -0.0, NA_real, np.inf, float("nan"), 0.0])
        val[spots] = np.array(table, dtype=val.dtype)
    return cp, ri, val


NROW = 2500


@functools.lru_cache(maxsize=None)
def placement_lengths(T):
    """The leaf lengths of the placement operand, 3T + 5 entries: an empty first leaf; leaves of 1-3 entries across
    the boundary T; 300 empty leaves in a row; a leaf longer than T, which holds the boundary 2T; leaves of 1-3 entries
    across the boundary 3T; an empty last leaf."""
    lengths, small = [0], (1, 2, 3, 3, 2)

    def across(boundary, end):
        """leaves of 1-3 entries up to `end` entries in all, one of 3 entries over [boundary - 1, boundary + 2)"""
        total = sum(lengths)
        while total < end:
            n = 3 if total == boundary - 1 else min(small[len(lengths) % 5], end - total)
            if total < boundary - 1:
                n = min(n, boundary - 1 - total)
            lengths.append(n)
            total += n

    across(T, T + 40)
    lengths.extend([0] * 300)
    lengths.append(T + 300)
    across(3 * T, 3 * T + 5)
    lengths.append(0)
    return tuple(lengths)


@functools.lru_cache(maxsize=None)
def device_operands(T):
    """name -> (nrow, (col_ptr, row_idx, val)) for a double and an integer operand of every shape"""
    out = {}
    for type in ("double", "integer"):
        out[f"placement_{type}"] = (NROW, from_lengths(NROW, placement_lengths(T), type, 11))
        out[f"nnz_0_{type}"] = (NROW, from_lengths(NROW, (0,) * 7, type, 12))
        out[f"nnz_T_{type}"] = (NROW, from_lengths(NROW, (T // 2, 0, T - T // 2 - 3, 3), type, 13))
        out[f"ncol_1_{type}"] = (NROW, from_lengths(NROW, (T + 300,), type, 14))
    return out


def dense_4d(type, seed=5):
    """a (5, 4, 3, 2) array as (nrow, (col_ptr, row_idx, val)), about 60 % of its cells stored, some with a zero"""
    rng = np.random.default_rng(seed)
    nrow, nl = DIM_4D[0], int(np.prod(DIM_4D[1:]))
    mask = rng.random((nrow, nl)) < 0.6
    mask[:, [0, 7, nl - 1]] = False
    lengths = mask.sum(axis=0)
    cp = np.zeros(nl + 1, np.int64)
    np.cumsum(lengths, out=cp[1:])
    ri = np.nonzero(mask.T)[1].astype(np.int32)
    val = _values(int(cp[-1]), type, seed + 1)
    val[::9] = 0
    return nrow, (cp, ri, val)


# ---------------------------------------------------------------------------
# host level: Session.sweep on the shared operands of arith_cases / compare_cases
# ---------------------------------------------------------------------------
# (name, operand, margin, op, type of STATS)
SESSION_CASES = (
    [(f"{x}_{m}_{op}_{st}", x, m, op, st) for x in ("d1", "i1", "d1s", "i1s", "d1l") for m in (1, 2)
     for op, st in (("*", "double"), ("/", "integer"), ("%%", "integer"), ("%/%", "double"), (">", "double"), ("<=", "integer"))] +
    [(f"{x}_{'_'.join(map(str, sc_m))}_{op}", x, sc_m, op, "double") for x in ("d3d", "i3d")
     for sc_m in ((1,), (2,), (3,), (1, 2), (2, 3), (1, 2, 3)) for op in ("*", ">")] +
    [("l1_2_eq", "l1", 2, "==", "integer"), ("empty_1", "d_empty", 1, "*", "double"), ("ncol_0", "d_ncol0", 2, "/", "double"),
     ("nrow_0", "d_nrow0", 1, "*", "double"), ("int_overflow", "i_big1", 2, "*", "integer")])
SESSION_NAMES = [c[0] for c in SESSION_CASES]
SESSION_BY_NAME = {c[0]: c for c in SESSION_CASES}
assert len(SESSION_BY_NAME) == len(SESSION_CASES)


def session_stats(name):
    _, xn, margin, op, st = SESSION_BY_NAME[name]
    x = cc.operand(xn)
    n = stats_length(x.dim, margin)
    s = stats_for(op, n, st, seed=len(name))
    if name == "int_overflow":
        s = (s.astype(np.int64) * 40000).astype(np.int32)           # 65536 * 40000 and INT_MAX * anything overflow
    return x, s
