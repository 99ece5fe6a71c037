"""Exact statistics of the cells of a sparse array, and the rounding bounds a double-precision kernel must meet.

A *cell* is whatever one result is reduced from: a generalized column (a run of ``inner`` leaves), a row cell of a
row statistic, a (group, column) cell of rowsum().  The stored values come as one flat array with the id of the cell
each belongs to; the implicit zeros (or implicit NAs of an NaArray) are given by the cell's length alone.

Everything here is exact: a finite double is ``m * 2**e`` with an integer ``m``, so sums, sums of squares and the
centred sums are integers after scaling by a power of two, and a quotient is a pair of integers.  ``ExactVec`` holds
one such rational per cell in object-dtype numpy arrays of Python ints (``np.add.at`` adds them without rounding).
``np.longdouble`` would only move the rounding, it would not remove it.

Notation of the bounds (Higham, *Accuracy and Stability of Numerical Algorithms*, 2nd ed., ch. 3 and 4):
``u = 2**-53``; ``gamma(k) = k u / (1 - k u)``; a product of ``k`` factors ``(1 + d_i)**(+-1)`` with ``|d_i| <= u`` is
``1 + t`` with ``|t| <= gamma(k)`` (Lemma 3.1).  ``n`` = stored values that take part after the NA rule, ``N`` = the
effective count (implicit zeros included), ``Z = N - n`` implicit zeros, ``A = sum |x_i|``.  The bounds hold for ANY
summation tree (lanes, wavefronts, chunks, atomics in arrival order): in a tree over ``m`` leaves a leaf passes through at
most ``m - 1`` additions, and adding an exact zero (an accumulator's start) rounds nothing.  They are theorems about the
formulas the kernels state, the constants are counts of roundings, there is no slack factor anywhere.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from sparsearray_amd import NA_integer, is_NA_real

U_BITS = 53


def _obj(a):
    return np.asarray(a).astype(object)


class ExactVec:
    """A vector of rationals ``num * 2**exp / den``: ``num`` and ``den`` object arrays of Python ints (``den`` > 0,
    or None for 1), ``exp`` one Python int for the whole vector."""

    def __init__(self, num, exp=0, den=None):
        self.num = num if isinstance(num, np.ndarray) and num.dtype == object else _obj(num)
        self.exp = int(exp)
        self.den = den

    @classmethod
    def from_float(cls, x):
        """Exact value of every (finite) double of ``x``; subnormals included (frexp normalises them)."""
        x = np.asarray(x, dtype=np.float64)
        assert np.all(np.isfinite(x)), "ExactVec.from_float: finite values only"
        if x.size == 0:
            return cls(np.zeros(x.shape, dtype=object))
        m, e = np.frexp(x)
        mant = np.ldexp(m, U_BITS).astype(np.int64)        # |m| < 1: an integer below 2**53, exactly
        sh = e.astype(np.int64) - U_BITS
        sh[mant == 0] = 0
        lo = int(sh.min())
        return cls(_obj(mant) << _obj(sh - lo), lo)

    @classmethod
    def from_int(cls, k):
        return cls(_obj(np.asarray(k, dtype=np.int64)))

    def __len__(self):
        return len(self.num)

    def __getitem__(self, idx):
        return ExactVec(self.num[idx], self.exp, None if self.den is None else self.den[idx])

    def _d(self):
        return 1 if self.den is None else self.den

    @staticmethod
    def _coerce(o):
        if isinstance(o, ExactVec):
            return o
        if isinstance(o, (int, np.integer)):
            return ExactVec(np.array([int(o)], dtype=object))
        if isinstance(o, Fraction):
            return ExactVec(np.array([o.numerator], dtype=object), 0, np.array([o.denominator], dtype=object))
        if isinstance(o, float):
            return ExactVec.from_float(np.array([o]))
        raise TypeError(type(o))

    def _aligned(self, o):
        e = min(self.exp, o.exp)
        return self.num * (1 << (self.exp - e)), o.num * (1 << (o.exp - e)), e

    def __add__(self, o):
        o = self._coerce(o)
        a, b, e = self._aligned(o)
        if self.den is None and o.den is None:
            return ExactVec(a + b, e)
        return ExactVec(a * o._d() + b * self._d(), e, self._d() * o._d())

    __radd__ = __add__

    def __neg__(self):
        return ExactVec(-self.num, self.exp, self.den)

    def __sub__(self, o):
        return self + (-self._coerce(o))

    def __mul__(self, o):
        o = self._coerce(o)
        den = None if self.den is None and o.den is None else self._d() * o._d()
        return ExactVec(self.num * o.num, self.exp + o.exp, den)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._coerce(o)
        num, den = self.num * o._d(), self._d() * o.num
        sign = np.where(den < 0, -1, 1).astype(object)
        return ExactVec(num * sign, self.exp - o.exp, den * sign)

    def __abs__(self):
        return ExactVec(np.abs(self.num), self.exp, self.den)

    def scale2(self, k):
        return ExactVec(self.num, self.exp + int(k), self.den)

    def _cross(self, o):
        o = self._coerce(o)
        a, b, _ = self._aligned(o)
        return a * o._d(), b * self._d()

    def le(self, o):
        a, b = self._cross(o)
        return np.asarray(a <= b, dtype=bool)

    def ratio(self, o):
        """self / o as floats (0/0 -> 0, x/0 -> inf): the err / bound figures of the record."""
        a, b = self._cross(o)
        a, b = np.broadcast_arrays(a, b)
        out = np.zeros(a.shape, dtype=np.float64)
        nz = np.asarray(b != 0, dtype=bool)
        out[nz] = (a[nz] / b[nz]).astype(np.float64)        # int / int: correctly rounded, whatever the sizes
        out[~nz & np.asarray(a != 0, dtype=bool)] = math.inf
        return out

    def to_fractions(self):
        d = np.broadcast_to(self._d(), self.num.shape)
        s = Fraction(2) ** self.exp
        return [Fraction(int(p), int(q)) * s for p, q in zip(self.num, d)]


def gamma(k):
    """gamma(k) = k u / (1 - k u) for an integer array ``k`` (k u < 1)."""
    k = _obj(np.asarray(k, dtype=np.int64))
    return ExactVec(k, 0, (1 << U_BITS) - k)


# ---------------------------------------------------------------------------
# exact moments of the cells
# ---------------------------------------------------------------------------
class Cells:
    """What a statistic of every cell is made of, after the NA rule.

    vals, cell: the stored values and the cell of each; length: elements per cell, implicit ones included (a scalar or
    one per cell).  ``na_bg``: the implicit elements are NAs (NaArray) instead of zeros.

    n      stored values taking part (not missing, or all of them when nothing is missing and na_rm is off)
    r      missing stored values (NA or NaN; ints: NA_integer)
    N, Z   effective count and implicit zeros after the NA rule
    na, nan   the cell sees an NA / a NaN that is not NA when na_rm is off (implicit NAs of an NaArray included)
    S, A, Q   sum x, sum |x|, sum x**2 over the values taking part (ExactVec)
    mn, mx    extremes of the values taking part as doubles (+Inf / -Inf for none), implicit zeros NOT included
    """

    def __init__(self, vals, cell, ncell, length, na_rm=False, na_bg=False):
        vals = np.asarray(vals)
        self.is_int = vals.dtype != np.float64
        cell = np.asarray(cell, dtype=np.int64)
        self.ncell, self.na_rm, self.na_bg = int(ncell), bool(na_rm), bool(na_bg)
        self.length = np.broadcast_to(np.asarray(length, dtype=np.int64), (ncell,)).copy()
        if self.is_int:
            miss = vals == NA_integer
            isna = miss
        else:
            miss = np.isnan(vals)
            isna = is_NA_real(vals)
        cnt = lambda mask: np.bincount(cell[mask], minlength=ncell).astype(np.int64)
        self.stored = np.bincount(cell, minlength=ncell).astype(np.int64)
        self.r = cnt(miss)
        self.n = self.stored - self.r
        implicit = self.length - self.stored
        assert np.all(implicit >= 0)
        self.implicit_na = implicit if na_bg else np.zeros_like(implicit)
        self.na = (cnt(isna) > 0) | (self.implicit_na > 0)
        self.nan = cnt(miss & ~isna) > 0
        self.Z = np.zeros_like(implicit) if na_bg else implicit
        removed = self.r + self.implicit_na if na_rm else 0
        self.N = self.length - removed
        # cells whose result is decided by a missing value (na_rm off)
        self.poisoned = (self.na | self.nan) & (not na_rm)
        keep = ~miss
        self.keep, self.cell, self.vals = keep, cell, vals
        fin = vals[keep].astype(np.float64)
        self.inf = np.zeros(ncell, dtype=bool)
        nonfin = ~np.isfinite(fin)
        if nonfin.any():
            self.inf[np.unique(cell[keep][nonfin])] = True
            fin = np.where(nonfin, 0.0, fin)
        self.x = ExactVec.from_float(fin)                   # the values taking part, element-wise
        self.xcell = cell[keep]
        self.S = self._per_cell(self.x.num, self.x.exp)
        self.A = self._per_cell(np.abs(self.x.num), self.x.exp)
        self.Q = self._per_cell(self.x.num * self.x.num, 2 * self.x.exp)
        v = vals[keep].astype(np.float64)
        self.mn = np.full(ncell, np.inf)
        self.mx = np.full(ncell, -np.inf)
        np.minimum.at(self.mn, self.xcell, v)
        np.maximum.at(self.mx, self.xcell, v)

    def _per_cell(self, num, exp):
        out = np.zeros(self.ncell, dtype=object)
        out[:] = 0
        np.add.at(out, self.xcell, num)
        return ExactVec(out, exp)

    # sum over the values taking part of |x| * |x - 2 c|, c one ExactVec entry per cell (row centred sums)
    def sum_abs_x_x2c(self, c):
        cc = c[self.xcell]
        t = abs(self.x) * abs(self.x - cc.scale2(1))
        a, d = t.num, t._d()
        if t.den is None:
            out = np.zeros(self.ncell, dtype=object)
            out[:] = 0
            np.add.at(out, self.xcell, a)
            return ExactVec(out, t.exp)
        # one denominator per cell (that of c): add the numerators, keep it
        out = np.zeros(self.ncell, dtype=object)
        out[:] = 0
        np.add.at(out, self.xcell, a)
        # den of t is den(c[cell]) (x has none): constant within a cell
        return ExactVec(out, t.exp, np.broadcast_to(c._d(), (self.ncell,)).astype(object) if c.den is not None else None)


def _flat(got):
    return np.asarray(got, dtype=np.float64).reshape(-1, order="F")


def _nan_class(got, cells, strict_na, what):
    """Cells decided by a missing value: NaN in ``got`` (NA where ``strict_na`` and the cell saw an NA).  Returns the
    mask of the cells still to be compared by value."""
    got = _flat(got)
    p = cells.poisoned
    assert np.all(np.isnan(got[p])), f"{what}: a cell with a missing value and na.rm=FALSE is not NaN"
    if strict_na:
        want_na = p & cells.na
        assert np.array_equal(is_NA_real(got[p]), want_na[p]), f"{what}: NA / NaN class differs"
    return ~p


class Verdict:
    """err / bound of every compared cell (``ratio``; 0 where both are 0) and whether every one is within its bound."""

    def __init__(self, err, bound, mask, what):
        self.what = what
        self.ok = bool(np.all(err.le(bound))) if len(err) else True
        self._err, self._bound = err, bound
        self.ncompared = int(mask.sum())

    @property
    def worst(self):
        return float(np.max(self._err.ratio(self._bound))) if len(self._err) else 0.0

    def require(self):
        assert self.ok, f"{self.what}: err / bound = {self.worst:.3g} > 1"
        return self


def _finite_got(got, mask, what):
    got = _flat(got)
    assert np.all(np.isfinite(got[mask])), f"{what}: a non-finite result where every input is finite"
    return ExactVec.from_float(got[mask])


# ---------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------
def check_sum(got, c: Cells, what="sum"):
    """computed = sum x_i (1 + t_i), |t_i| <= gamma(n - 1): n - 1 additions on the longest path of any tree, the
    additions of exact zeros free.  |got - S| <= gamma(n - 1) A.  (n <= 1: exact.)"""
    m = _nan_class(got, c, False, what) & ~c.inf
    g = _finite_got(got, m, what)
    return Verdict(abs(g - c.S[m]), gamma(np.maximum(c.n[m] - 1, 0)) * c.A[m], m, what)


def check_mean(got, c: Cells, what="mean"):
    """got = fl(sum) / N (1 + d): one rounding more than the sum, N exact.  |got - S / N| <= gamma(n) A / N.
    N == 0 (everything removed): 0 / 0, NaN."""
    got = _flat(got)
    m = _nan_class(got, c, False, what) & ~c.inf
    empty = m & (c.N == 0)
    assert np.all(np.isnan(got[empty])), f"{what}: mean of nothing is not NaN"
    m &= c.N > 0
    g = _finite_got(got, m, what)
    N = ExactVec.from_int(c.N[m])
    return Verdict(abs(g * N - c.S[m]), gamma(c.n[m]) * c.A[m], m, what)


def prod_safe(c: Cells, limit=1000.0):
    """Cells whose every partial product, in any order, stays in the normal range: sum |log2 |x_i|| <= limit."""
    v = np.abs(c.vals[c.keep].astype(np.float64))
    with np.errstate(divide="ignore"):
        lg = np.abs(np.log2(v))
    tot = np.zeros(c.ncell)
    np.add.at(tot, c.xcell, lg)
    return (tot <= limit) & ~c.inf


def check_prod(got, c: Cells, what="prod"):
    """n factors from an exact 1: at most n - 1 roundings when no partial product leaves the normal range (prod_safe);
    relative error <= gamma(n) as the issue states it (gamma(n - 1) would do).  With an implicit zero the result is the
    product times 0.0, a zero.  Cells that are not safe are left out: their result depends on the order."""
    got = _flat(got)
    m = _nan_class(got, c, False, what) & prod_safe(c)
    z = m & (c.Z > 0)
    assert np.all(got[z] == 0.0), f"{what}: a cell with an implicit zero is not 0"
    m &= c.Z == 0
    idx = np.flatnonzero(m)
    order = np.argsort(c.xcell, kind="stable")
    xs, bounds = c.x.num[order], np.searchsorted(c.xcell[order], np.arange(c.ncell + 1))
    exact = np.empty(len(idx), dtype=object)
    for k, i in enumerate(idx):
        p = 1
        for f in xs[bounds[i]:bounds[i + 1]]:
            p *= f
        exact[k] = p
    P = ExactVec(exact, 0)
    # every factor carries 2**x.exp
    ex = [Fraction(2) ** (c.x.exp * int(c.n[i])) for i in idx]
    P = P * ExactVec(np.array([f.numerator for f in ex], dtype=object), 0,
                     np.array([f.denominator for f in ex], dtype=object)) if len(idx) else P
    g = _finite_got(got, m, what)
    return Verdict(abs(g - P), gamma(c.n[m]) * abs(P), m, what)


def check_identical(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    if want.dtype.kind == "f":
        got = got.astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
        assert np.array_equal(is_NA_real(got), is_NA_real(want)), f"{what}: NA / NaN class"
        k = ~np.isnan(want)
        assert np.array_equal(got[k], want[k]), f"{what}: values differ"
        assert np.array_equal(np.signbit(got[k])[want[k] != 0], np.signbit(want[k])[want[k] != 0])
    else:
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), f"{what}: values differ"


def exact_minmax(c: Cells, is_min, as_int=False):
    """min / max: NA wins, else NaN (na_rm off), else the extremum with the implicit zero joining when there is one
    (src/Rvector_summarization.c:1078-1128).  Doubles: nothing to look at gives +Inf / -Inf; ints: NA_integer."""
    from sparsearray_amd import NA_real
    m = c.mn.copy() if is_min else c.mx.copy()
    z = c.Z > 0
    m[z] = np.minimum(m[z], 0.0) if is_min else np.maximum(m[z], 0.0)
    if as_int:
        none = (c.n == 0) & ~z
        out = np.where(none, 0.0, m).astype(np.int64)
        out[none] = NA_integer
        out[c.poisoned] = NA_integer
        return out.astype(np.int32)
    m[c.poisoned & c.nan] = np.nan
    m[c.poisoned & c.na] = NA_real
    return m


def exact_int_no_value(c: Cells):
    """Integer min / max warn ("NAs introduced by coercion of infinite values to integers") exactly when some cell has
    nothing to look at -- no value taking part, no implicit zero -- and no missing value decides it first
    (src/Rvector_summarization.c:1108-1128)."""
    return bool(np.any((c.n == 0) & (c.Z == 0) & ~c.poisoned))


def exact_count_nas(c: Cells):
    return (c.r + c.implicit_na).astype(np.float64)


def exact_any_all(c: Cells, is_any):
    """any / all of an int or logical array (src/Rvector_summarization.c:260-313 and :1100-1106)."""
    v = c.vals[c.keep]
    true = np.bincount(c.xcell[v != 0], minlength=c.ncell) > 0
    zero = (np.bincount(c.xcell[v == 0], minlength=c.ncell) > 0) | (c.Z > 0)
    brk = c.na & (not c.na_rm)
    if is_any:
        return np.where(true, 1, np.where(brk, NA_integer, 0)).astype(np.int32)
    return np.where(zero, 0, np.where(brk, NA_integer, 1)).astype(np.int32)


def _center_error(c: Cells, m):
    """Delta = gamma(n) A / N, the bound of check_mean on the centre the kernel computes for itself."""
    return gamma(c.n[m]) * c.A[m] / ExactVec.from_int(c.N[m])


def check_col_centered(got, c: Cells, center=None, op="centered_X2_sum", dgc=False, what=None):
    """Two-pass column form (src/SparseArray_summarization.c:70-109): got = fl( sum fl(fl(x - c)**2) + fl(fl(c c) Z) ).

    A term of the sum: one rounding for the difference, which the square doubles, one for the product, n - 1 additions,
    the final addition: n + 3.  The zeros' term: two products and the final addition.  All terms are >= 0, so
    |got - Q(c)| <= gamma(n + 3) Q(c) with Q(c) = sum over all N elements of (x - c)**2, exact at the c the kernel
    used.  var1 divides once (N - 1 exact): n + 4.  sd1 takes a root, (1 + d); its square carries two more: n + 6, so sd
    is checked as sd**2 against the bound of the variance.  The issue states every one of them with gamma(n + 6).

    A caller's centre is the c the kernel used: |got - Q(c)| <= gamma(n + 6) Q(c).
    Without one the kernel's c is its own mean, |c - mu| <= Delta = gamma(n) A / N (check_mean), and
    Q(c) = T + N (c - mu)**2 <= T + N Delta**2 with T = Q(mu) = sum x**2 - S**2 / N, hence
    |got - T| <= gamma(n + 6) (T + N Delta**2) + N Delta**2;  var1: both sides / (N - 1).
    N <= 1 for var1 / sd1: NA (dgc: the IEEE quotient, not compared)."""
    what = what or op
    got = _flat(got)
    m = _nan_class(got, c, False, what) & ~c.inf
    if op != "centered_X2_sum":
        few = m & (c.N <= 1)
        if not dgc:
            assert np.all(np.isnan(got[few])), f"{what}: fewer than two values is not NA"
        m &= c.N > 1
    elif center is None:
        m &= c.N > 0
    g = _finite_got(got, m, what)
    if op == "sd1":
        g = g * g
    N = ExactVec.from_int(c.N[m])
    S, Q = c.S[m], c.Q[m]
    gam = gamma(c.n[m] + 6)
    if center is not None:
        cc = ExactVec.from_float(np.broadcast_to(np.asarray(center, dtype=np.float64), (c.ncell,))[m])
        T = Q - cc.scale2(1) * S + N * cc * cc             # sum over all N elements of (x - c)**2
        bound = gam * T
    else:
        T = Q - S * S / N
        D = _center_error(c, m)
        ND2 = N * D * D
        bound = gam * (T + ND2) + ND2
    if op != "centered_X2_sum":
        N1 = ExactVec.from_int(c.N[m] - 1)
        g = g * N1
    return Verdict(abs(g - T), bound, m, what)


def check_row_centered(got, c: Cells, center=None, op="centered_X2_sum", what=None):
    """Expanded row form (src/SparseArray_matrixStats.c:636-696): a cell starts at fl(fl(c c) nstrata), every value
    adds fl(x fl(x - 2 c)) (2 c is exact), every value removed by na.rm adds -fl(c c):
    got = fl( c c nstrata + sum x (x - 2 c) - r c c ), in exact arithmetic T(c) = sum over the N = nstrata - r elements
    of (x - c)**2.  The tree has n + r + 1 leaves of at most two roundings each: n + r + 2 roundings on a path,
    |got - T(c)| <= gamma(n + r + 2) M(c),  M(c) = (nstrata + r) c c + sum |x| |x - 2 c|  (the terms' magnitudes; the
    terms cancel, which is why M and not T carries the error).  var1 divides (n + r + 3), sd1 is checked squared
    (n + r + 5).  The issue's constant is gamma(n + 6): it is a theorem for r <= 4 (centred sum), 3 (var1), 1 (sd1), and
    the cases plant at most one missing value per row cell; more is refused here rather than bounded by something else.

    With a caller's centre that is the whole bound.  Without one (rowVars / rowSds) the centre is the kernel's own mean,
    |c - mu| <= Delta = gamma(n) A / N: T(c) = T + N (c - mu)**2 and, term by term, c c <= mu mu + Delta (2 |mu| + Delta),
    |x - 2 c| <= |x - 2 mu| + 2 Delta, so with K = nstrata + r (= N when nothing is removed)
    |got - T| <= gamma(n + 6) M + N Delta**2,  M = K mu mu + sum |x| |x - 2 mu| + 2 Delta A + K Delta (2 |mu| + Delta).
    A plain centered_X2_sum without a centre is sum x**2 (c = 0)."""
    what = what or op
    got = _flat(got)
    m = _nan_class(got, c, False, what) & ~c.inf
    r = c.r if c.na_rm else np.zeros_like(c.r)
    extra = {"centered_X2_sum": 2, "var1": 3, "sd1": 5}[op]
    assert np.all(r[m] + extra <= 6), f"{what}: more removed values in a row cell than gamma(n + 6) covers"
    if op != "centered_X2_sum":
        assert np.all(c.N[m] > 1)
    g = _finite_got(got, m, what)
    if op == "sd1":
        g = g * g
    N = ExactVec.from_int(c.N[m])
    K = ExactVec.from_int((c.length + r)[m])
    S, Q, A = c.S[m], c.Q[m], c.A[m]
    gam = gamma(c.n[m] + 6)
    sub = _subset(c, m)
    if center is not None or op == "centered_X2_sum":
        cen = np.zeros(c.ncell) if center is None else np.broadcast_to(np.asarray(center, dtype=np.float64).reshape(-1),
                                                                       (c.ncell,))
        cc = ExactVec.from_float(cen[m])
        T = Q - cc.scale2(1) * S + N * cc * cc
        bound = gam * (K * cc * cc + sub.sum_abs_x_x2c(cc))
    else:
        mu = S / N
        T = Q - S * S / N
        D = _center_error(c, m)
        M = K * mu * mu + sub.sum_abs_x_x2c(mu) + D.scale2(1) * A + K * D * (abs(mu).scale2(1) + D)
        bound = gam * M + N * D * D
    if op != "centered_X2_sum":
        g = g * ExactVec.from_int(c.N[m] - 1)
    return Verdict(abs(g - T), bound, m, what)


class _subset:
    """The values of the cells in ``mask``, renumbered 0.. (for Cells.sum_abs_x_x2c on a selection)."""

    def __init__(self, c: Cells, mask):
        new_id = np.cumsum(mask) - 1
        sel = mask[c.xcell]
        self.x = c.x[sel]
        self.xcell = new_id[c.xcell[sel]]
        self.ncell = int(mask.sum())

    sum_abs_x_x2c = Cells.sum_abs_x_x2c


# ---------------------------------------------------------------------------
# cells of the entry points, from the CSC arrays
# ---------------------------------------------------------------------------
def column_cells(col_ptr, val, nrow, inner=1, na_rm=False, na_bg=False):
    """Generalized columns: runs of ``inner`` leaves."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    nleaf = len(col_ptr) - 1
    leaf = np.repeat(np.arange(nleaf, dtype=np.int64), np.diff(col_ptr))
    return Cells(val, leaf // inner, nleaf // inner, inner * nrow, na_rm, na_bg)


def row_cells(col_ptr, row_idx, val, nrow, inner=1, na_rm=False, na_bg=False):
    """Row cells: cell = (leaf % inner) * nrow + row, each reduced over the nleaf / inner strata."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    nleaf = len(col_ptr) - 1
    leaf = np.repeat(np.arange(nleaf, dtype=np.int64), np.diff(col_ptr))
    cell = (leaf % inner) * nrow + np.asarray(row_idx, dtype=np.int64)
    return Cells(val, cell, inner * nrow, nleaf // inner, na_rm, na_bg)


def rowsum_cells(col_ptr, row_idx, val, group0, ngroup, na_rm=False):
    """rowsum(): cell (g, j) = g + ngroup * j holds the rows of column j in group g (0-based ``group0``)."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    ncol = len(col_ptr) - 1
    col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(col_ptr))
    group0 = np.asarray(group0, dtype=np.int64)
    cell = group0[np.asarray(row_idx, dtype=np.int64)] + ngroup * col
    size = np.bincount(group0, minlength=ngroup).astype(np.int64)
    return Cells(val, cell, ngroup * ncol, np.tile(size, ncol), na_rm, False)


def colsum_cells(col_ptr, row_idx, val, group0, ngroup, nrow, na_rm=False):
    """colsum(): cell (i, g) = i + nrow * g holds row i of the columns in group g (0-based ``group0``, one per column)."""
    col_ptr = np.asarray(col_ptr, dtype=np.int64)
    ncol = len(col_ptr) - 1
    col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(col_ptr))
    group0 = np.asarray(group0, dtype=np.int64)
    cell = np.asarray(row_idx, dtype=np.int64) + nrow * group0[col]
    size = np.bincount(group0, minlength=ngroup).astype(np.int64)
    return Cells(val, cell, nrow * ngroup, np.repeat(size, nrow), na_rm, False)
