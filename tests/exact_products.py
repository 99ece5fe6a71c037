"""Exact results of the product kernels and the rounding bounds a double-precision kernel must meet.

A *cell* is one entry of a product: ``(c, k)`` of ``crossprod(x, Y)`` (leaf ``c`` of the sparse operand against dense
column ``k``) or ``(i, j)`` of a sparse x sparse product.  A finite double is ``m * 2**e`` with an integer ``m``
(exact_stats.ExactVec), so every term ``a_i * y_i`` is an integer after scaling by one power of two, and ``np.add.at``
adds the terms of a cell into object arrays of Python ints without rounding.  Per cell three things are kept:

    E   the exact value                       sum a_i y_i
    M   the magnitude of the terms            sum |a_i| |y_i|
    n   the number of terms                   sparse x dense: the nonzeros of the leaf;
                                              sparse x sparse: the rows where both operands hold a nonzero

The rule for finite operands (``u = 2**-53``, ``gamma(k) = k u / (1 - k u)``, Higham ch. 3):

    |got - E| <= gamma(n) M     for every cell with n >= 1,          got == 0 exactly for n == 0.

Derivation.  Every term is one rounded product, ``fl(a y) = a y (1 + d)``, or no rounding at all where the kernel uses
a fused multiply-add.  The ``n`` terms are then added in SOME tree (lanes, batches, row splits, row chunks, rounds,
the reduce kernels in split order): in a tree over ``n`` leaves a leaf passes through at most ``n - 1`` additions, each
``(1 + d)``.  A term therefore carries at most ``n`` factors ``(1 + d_i)``, i.e. ``1 + t`` with ``|t| <= gamma(n)``
(Lemma 3.1), and ``|got - E| <= sum |a_i y_i| gamma(n)``.  What the layouts add to the tree rounds nothing: a zero
padding record adds ``0 * y`` (exact for finite ``y``) to an accumulator, and ``s + 0 == s`` exactly; an accumulator
starts from an exact zero; the partial sum of a row split or row chunk that holds no nonzero of the leaf is an exact
zero, and adding it is exact.  So the bound holds for every order, for FMA or separate multiply and add, and for any
number of splits, chunks and rounds.  The constant is a count of roundings; there is no slack factor.

Ranges.  The palettes scale by at most 2**+-400 and their values lie within 2**+-60 of 1, so ``assert_ranges`` holds
every operand's exponent within +-480 and ``Product`` holds ``M < 2**1000``: no product underflows (its exponent is
above -960, so ``(1 + d)`` is the whole error of a product) and no partial sum overflows, in any order.

Integer-exact rule.  When every operand is an integer and ``n max|a| max|y| < 2**53`` every product and every
partial sum in every order is an integer below 2**53, hence exact: ``got`` must be IDENTICAL to ``E``
(``check_identical_product``).

Non-finite dense operand (``check_with_nonfinite``): a cell is expected non-finite exactly where the reference's result
is, with the reference's class (NaN / NA / +-Inf); every other cell obeys the finite rule over the leaf's nonzeros
(the non-finite entries sit on rows the leaf does not hold, and count as zeros there).
"""
from __future__ import annotations

import numpy as np

from exact_stats import ExactVec, U_BITS, Verdict, gamma
from sparsearray_amd import is_NA_real


def _zeros(shape):
    out = np.empty(shape, dtype=object)
    out[...] = 0
    return out


def _exact(values):
    values = np.asarray(values)
    if values.dtype.kind in "iu":
        return ExactVec.from_int(values)
    return ExactVec.from_float(values)


def assert_ranges(*operands, limit=480):
    """Every nonzero operand has its exponent within +-limit (the palettes' promise)."""
    for v in operands:
        v = np.asarray(v, dtype=np.float64)
        v = v[v != 0]
        assert np.all(np.isfinite(v)), "assert_ranges: finite operands only"
        if v.size:
            e = np.frexp(v)[1]
            assert e.min() >= -limit and e.max() <= limit + 1, "operand exponent outside the palette's range"


class Product:
    """E, M (ExactVec over the cells, flattened in C order of ``shape``) and n (int64, same order)."""

    def __init__(self, E, M, n, shape):
        self.E, self.M, self.n, self.shape = E, M, np.asarray(n, dtype=np.int64).reshape(-1), tuple(shape)
        top = (int(M.num.max()).bit_length() if len(M.num) else 0) + M.exp      # (every M >= 0)
        assert top < 1000, "M >= 2**1000: a partial sum may overflow"

    def E_float(self):
        """E rounded to double (for the demonstrations; never the yardstick)."""
        from fractions import Fraction
        s = Fraction(2) ** self.E.exp
        return np.array([float(Fraction(int(v)) * s) for v in self.E.num]).reshape(self.shape)


def exact_sparse_dense(col_ptr, row_idx, val, Y):
    """crossprod(x, Y): cells (c, k), shape (ncol, K).  ``Y``: (nrow, K), finite."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    row_idx = np.asarray(row_idx, dtype=np.int64)
    Y = np.asarray(Y)
    ncol, K = len(col_ptr) - 1, Y.shape[1]
    Yg = Y[row_idx, :]                                      # (only the rows some nonzero meets take part)
    assert_ranges(val, Yg)
    a, y = _exact(val), _exact(Yg)
    leaf = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(col_ptr))
    terms = a.num[:, None] * y.num if len(row_idx) else _zeros((0, K))
    E, M = _zeros((ncol, K)), _zeros((ncol, K))
    np.add.at(E, leaf, terms)
    np.add.at(M, leaf, np.abs(terms))
    n = np.repeat(np.diff(col_ptr)[:, None], K, axis=1)
    e = a.exp + y.exp
    return Product(ExactVec(E.reshape(-1), e), ExactVec(M.reshape(-1), e), n, (ncol, K))


def _by_row(nrow, col_ptr, row_idx, val):
    """The nonzeros of a CSC operand sorted by row: (row_ptr, col, val)."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    row_idx = np.asarray(row_idx, dtype=np.int64)
    col = np.repeat(np.arange(len(col_ptr) - 1, dtype=np.int64), np.diff(col_ptr))
    order = np.argsort(row_idx, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(row_idx, minlength=nrow))]).astype(np.int64)
    return rp, col[order], np.asarray(val)[order]


def exact_sparse_sparse(nrow, x, y):
    """crossprod(x, y) of two CSC operands ``(col_ptr, row_idx, val)`` with ``nrow`` rows each: cells (i, j), shape
    (ncol(x), ncol(y)); n = rows where column i of x and column j of y both hold a nonzero."""
    ni, nj = len(x[0]) - 1, len(y[0]) - 1
    assert_ranges(x[2], y[2])
    xp, xc, xv = _by_row(nrow, *x)
    yp, yc, yv = _by_row(nrow, *y)
    cy = np.diff(yp)
    xrow = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(xp))
    rep = cy[xrow]                                          # partners of every nonzero of x
    ix = np.repeat(np.arange(len(xc), dtype=np.int64), rep)
    start = np.cumsum(rep) - rep
    iy = yp[xrow][ix] + (np.arange(len(ix), dtype=np.int64) - start[ix])
    a, b = _exact(xv), _exact(yv)
    terms = a.num[ix] * b.num[iy]
    cell = xc[ix] * nj + yc[iy]
    E, M = _zeros(ni * nj), _zeros(ni * nj)
    np.add.at(E, cell, terms)
    np.add.at(M, cell, np.abs(terms))
    n = np.bincount(cell, minlength=ni * nj)
    e = a.exp + b.exp
    return Product(ExactVec(E, e), ExactVec(M, e), n, (ni, nj))


def transpose_csc(nrow, col_ptr, row_idx, val):
    """CSC arrays of t(x) (exact: a permutation)."""
    rp, col, v = _by_row(nrow, col_ptr, row_idx, val)
    return rp, col.astype(np.int32), v


def exact_matmul_sparse(nrow_x, x, y):
    """x %*% y of two CSC operands, x with ``nrow_x`` rows: cells (i, j), shape (nrow(x), ncol(y)) -- crossprod(t(x), y)."""
    return exact_sparse_sparse(len(x[0]) - 1, transpose_csc(nrow_x, *x), y)


def tracer_sparse_dense(col_ptr, row_idx, val, Y):
    """The same for integer operands as an int64 computation (scipy.sparse): for operands too large for object
    arrays.  Returns (E, M, n) as int64 arrays of shape (ncol, K)."""
    import scipy.sparse as sp
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    Y = np.asarray(Y)
    nrow, ncol = Y.shape[0], len(col_ptr) - 1
    a = np.asarray(val).astype(np.int64)
    yi = Y.astype(np.int64)
    assert np.array_equal(a, np.asarray(val)) and np.array_equal(yi, Y), "tracer operands are integers"
    nmax = int(np.diff(col_ptr).max(initial=0))
    assert nmax * int(np.abs(a).max(initial=0)) * int(np.abs(yi).max(initial=0)) < 2 ** U_BITS
    A = sp.csc_matrix((a, np.asarray(row_idx, dtype=np.int64), col_ptr), shape=(nrow, ncol))
    E = np.asarray((A.T @ yi))
    M = np.asarray((abs(A).T @ np.abs(yi)))
    n = np.repeat(np.diff(col_ptr)[:, None], Y.shape[1], axis=1)
    return E.astype(np.int64), M.astype(np.int64), n


def integer_exact(p: Product, max_a, max_y):
    """The integer-exact rule applies: n max|a| max|y| < 2**53 (operands integers: the caller's palette)."""
    return int(p.n.max(initial=0)) * int(max_a) * int(max_y) < 2 ** U_BITS


# ---------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------
def check_product(got, p: Product, what="product", mask=None):
    """The finite rule on every cell (``mask``: on those cells only -- the non-finite rule's use, never a way to
    leave a cell out).  ``got``: array of p.shape.  Returns the Verdict (ncompared = cells with n >= 1)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == p.shape, f"{what}: shape {got.shape} != {p.shape}"
    got = got.reshape(-1)
    m = np.ones(len(got), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1).copy()
    assert np.all(np.isfinite(got[m])), f"{what}: a non-finite result where every term is finite"
    empty = m & (p.n == 0)
    assert np.all(got[empty] == 0.0), f"{what}: a cell without terms is not exactly zero"
    m &= p.n > 0
    g = ExactVec.from_float(got[m])
    return Verdict(abs(g - p.E[m]), gamma(p.n[m]) * p.M[m], m, what)


def check_identical_product(got, E, what="product"):
    """The integer-exact rule: every cell identical to the exact integer."""
    got = np.asarray(got, dtype=np.float64)
    E = np.asarray(E)
    if E.dtype == object:
        E = E.astype(np.int64)
    assert got.shape == E.shape, f"{what}: shape {got.shape} != {E.shape}"
    assert np.abs(E).max(initial=0) < 2 ** U_BITS
    bad = np.flatnonzero(got.reshape(-1) != E.reshape(-1).astype(np.float64))
    assert bad.size == 0, (f"{what}: {bad.size} cells differ from the exact integer, first at "
                           f"{np.unravel_index(bad[0], got.shape)}: {got.reshape(-1)[bad[0]]!r} != {E.reshape(-1)[bad[0]]}")


def exact_int(p: Product):
    """E of an integer product as an int64 array of p.shape."""
    if p.E.exp >= 0:
        return (p.E.num * (1 << p.E.exp)).astype(np.int64).reshape(p.shape)
    d = 1 << -p.E.exp
    assert not np.any(p.E.num % d), "exact_int: not an integer product"
    return (p.E.num // d).astype(np.int64).reshape(p.shape)


def check_with_nonfinite(got, want, col_ptr, row_idx, val, Y, what="product"):
    """The non-finite rule: ``want`` is the reference's result for the same operands.  Returns the Verdict of the
    finite cells."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape"
    nf = ~np.isfinite(want)
    assert np.array_equal(~np.isfinite(got), nf), f"{what}: the non-finite cells are not the reference's"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    assert np.array_equal(is_NA_real(got), is_NA_real(want)), f"{what}: NA / NaN class"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: sign of an infinity"
    Yf = np.where(np.isfinite(Y), Y, 0.0)
    return check_product(got, exact_sparse_dense(col_ptr, row_idx, val, Yf), what, mask=~nf)
