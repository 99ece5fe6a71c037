"""Seeded random cases for nine kernel families -- subset, Arith / Math, the count / select order statistics, the ranks,
Compare / Logic, sweep(), pmin / pmax and is.na / is.nan / is.infinite, subassignment by N-index, and subsetting and
subassignment by L-index and M-index -- shared by tests/test_random_cases_cpu.py (the generators and expectations
themselves, through the oracle session where it offers the operation) and tests/test_hip_random_cases.py (the device).

Pure numpy, ``np.random.default_rng([seed, k])`` with one k per family; one seed is one case.  Each generator returns
the operand arrays, the calls and, per call, the DENSE expectation.  Structure is drawn from the constants the kernels
cut by, read from the library (subset_tile(), arith_tile(), colranks_form_limits(), subassign_tile(),
lindex_sort_passes()), never copied here.  Nothing is filtered, skipped or retried: what a seed draws is what is
compared.  The five later families are rules on the merge, map and sweep tile kernels of the Arith family (and two
placement stages in front of them); their element-wise expectations are those of their own case modules
(compare_cases, sweep_cases, pminmax_cases, subassign_cases, lindex_cases), and their keys are PairKeys' or
draw_columns'.

Columns (subset, Arith): a total of T-1, T, T+1, 2T, 2T+1 or 3T+-k nonzeros for the family's tile T; with
probability 0.6 one column holds 50 to 95 % of them; the others come in runs -- empty runs of 1 to 600 columns, runs of
lengths 0 to 3, runs of binomial lengths -- and the last non-empty ones are trimmed to the total.  ncol is drawn from
1, 3, 40, 700, 5000 among those that keep the dense matrix of the reference under 2^23 cells (a rule of the draw, stated
here: the reference is a dense matrix).  Every fifth seed has a full column (nrow = the longest column).
"""
from __future__ import annotations

import numpy as np

import arith_cases as ac
import compare_cases as cc
import lindex_cases as lc
import pminmax_cases as pc
import subassign_cases as sa
import subset_cases as sc
import sweep_cases as sw
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from test_mads_cpu import dense_colmads
from test_medians import dense_colmedians
from test_quantiles_cpu import dense_colquantiles
from test_hip_ranks import expand as expand_ranks        # (the dense ranks of the compact form; needs no GPU)
from test_ranks_cpu import TIES, dense_colranks

SEEDS = list(range(8))
NCOLS = (1, 3, 40, 700, 5000)
CELLS = 1 << 23
INT_MAX = 2 ** 31 - 1


def tiles():
    """(subset tile, Arith tile, (f0, f1) of the ranks' forms): the library's own figures, no GPU needed"""
    from sparsearray_amd.device import arith_tile, colranks_form_limits, subset_tile
    return subset_tile(), arith_tile(), colranks_form_limits()


def more_tiles():
    """(tile of the subassignment's placement, the function nrow, ncol -> 8-bit passes of the L-index sort): the further
    figures of the library, no GPU needed"""
    from sparsearray_amd.device import lindex_sort_passes, subassign_tile
    return subassign_tile(), lindex_sort_passes


# ---------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------
def draw_total(rng, T):
    k = int(rng.integers(1, 200))
    return int(rng.choice([T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T - k, 3 * T + k]))


def draw_columns(rng, total, full_column):
    """-> (nrow, lens int64[ncol]) with lens.sum() == total"""
    heavy = int(round(rng.uniform(0.5, 0.95) * total)) if rng.random() < 0.6 else 0
    fits = [n for n in NCOLS if max(heavy, 64) * n <= CELLS]
    weight = np.array([1.0, 1.0, 2.0, 3.0, 3.0][:len(fits)])      # (one and three columns are the rarer draws)
    ncol = int(rng.choice(fits, p=weight / weight.sum()))
    if ncol == 1:
        lens = np.array([total], dtype=np.int64)
    else:
        lens = np.zeros(ncol, dtype=np.int64)
        at = int(rng.integers(0, ncol))                     # where the heavy column sits (none: an ordinary column)
        rest, j = total - heavy, 0
        while j < ncol:
            kind, run = int(rng.integers(0, 3)), 0
            if kind == 0:                                   # an empty run
                run = int(rng.integers(1, 601))
            elif kind == 1:                                 # lengths 0 to 3
                run = int(rng.integers(1, 51))
                lens[j:j + run] = rng.integers(0, 4, size=min(run, ncol - j))
            else:                                           # binomial lengths around what is left per column
                run = int(rng.integers(1, 51))
                mean = max(1.0, (rest - lens[:j].sum()) / max(1, ncol - j))
                lens[j:j + run] = rng.binomial(int(2 * mean) + 1, 0.5, size=min(run, ncol - j))
            j += run
        lens[at] = 0
        over = int(lens.sum()) - rest                       # trim the last non-empty columns to the total ...
        for j in np.flatnonzero(lens)[::-1]:
            if over <= 0:
                break
            cut = min(over, int(lens[j]))
            lens[j] -= cut
            over -= cut
        lens[at] = heavy
        if lens.sum() < total:                              # ... or give what is missing to one column
            lens[at if heavy else int(np.flatnonzero(lens)[-1]) if lens.any() else ncol - 1] += total - int(lens.sum())
    longest = int(lens.max())
    nrow = longest if full_column else max(longest, 50) + int(rng.integers(1, 100))
    assert lens.sum() == total and nrow * ncol <= 4 * CELLS, (total, nrow, ncol)
    return nrow, lens


def place(rng, nrow, lens):
    """(col_ptr, row_idx) with ascending random rows in every column"""
    cp = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=cp[1:])
    ri = np.concatenate([np.sort(rng.choice(nrow, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return cp, ri.astype(np.int32)


def mixed_values(rng, n, type, share=0.1):
    """ordinary values (never zero) with ``share`` of them from the specials table of the type"""
    if type == "double":
        v = np.round(rng.uniform(0.5, 100.0, size=n), 3) * rng.choice([-1.0, 1.0], size=n)
        table = sc.SPECIALS_F64
    elif type == "integer":
        v = (rng.integers(1, 1000, size=n) * rng.choice([-1, 1], size=n)).astype(np.int32)
        table = np.concatenate([sc.SPECIALS_I32, np.array([INT_MAX - 1, -INT_MAX, 46341, 65536], dtype=np.int32)])
    else:
        return sc.SPECIALS_LGL[rng.integers(0, len(sc.SPECIALS_LGL), size=n)]
    at = rng.random(n) < share
    v[at] = table[rng.integers(0, len(table), size=int(at.sum()))]
    return v


def svt_of(nrow, type, cp, ri, val):
    return SVT_SparseArray.from_csc((nrow, cp.size - 1), type, cp, ri, val)


# ---------------------------------------------------------------------------
# subset
# ---------------------------------------------------------------------------
ROW_KINDS = ("none", "increasing_half", "single", "all", "empty", "permutation", "repeats_longer_than_the_axis")
COL_KINDS = ("none", "reversed", "repeats", "empty")
SUBSET_TYPES = ("double", "integer", "logical")


def _rows(rng, kind, nrow):
    if kind == "none":
        return None
    if kind == "increasing_half":
        return np.flatnonzero(rng.random(nrow) < 0.5).astype(np.int32)
    if kind == "single":
        return rng.integers(0, nrow, size=1).astype(np.int32)
    if kind == "all":
        return np.arange(nrow, dtype=np.int32)
    if kind == "empty":
        return np.zeros(0, np.int32)
    if kind == "permutation":
        return rng.permutation(nrow).astype(np.int32)
    return rng.integers(0, nrow, size=nrow + nrow // 5 + 1).astype(np.int32)


def _cols(rng, kind, lens):
    ncol = lens.size
    if kind == "none":
        return None
    if kind == "reversed":
        return np.arange(ncol, dtype=np.int32)[::-1].copy()
    if kind == "empty":
        return np.zeros(0, np.int32)
    # repeats: a permutation, then the longest column and an empty one (when there is one) many times over, shuffled
    longest = int(np.argmax(lens))
    empty = np.flatnonzero(lens == 0)
    extra = [np.full(int(rng.integers(2, 6)), longest)]
    if empty.size:
        extra.append(np.full(int(rng.integers(2, 301)), empty[int(rng.integers(0, empty.size))]))
    c = np.concatenate([rng.permutation(ncol)] + extra)
    return rng.permutation(c).astype(np.int32) if rng.random() < 0.5 else c.astype(np.int32)


class SubsetCase:
    """.nrow .type .cp .ri .val; .calls: [(rows, cols)], 0-based or None; expected(call) -> (col_ptr, row_idx, val)"""

    def __init__(self, seed, T):
        rng = np.random.default_rng([seed, 1])
        self.seed, self.type = seed, SUBSET_TYPES[seed % 3]
        self.total = draw_total(rng, T)
        self.nrow, self.lens = draw_columns(rng, self.total, seed % 5 == 0)
        self.cp, self.ri = place(rng, self.nrow, self.lens)
        self.val = mixed_values(rng, self.total, self.type)
        # the kinds go round with the seed, so that eight seeds meet every one of them
        self.row_kinds = (ROW_KINDS[1 + seed % 6], ROW_KINDS[(seed + 3) % 7])
        self.col_kind = ("repeats", "reversed", "repeats", "empty")[seed % 4]
        r0, r1 = (_rows(rng, kind, self.nrow) for kind in self.row_kinds)
        c = _cols(rng, self.col_kind, self.lens)
        self.calls = [(r0, None), (None, c), (r1, c)]

    def expected(self, call):
        """np.ix_ on the dense matrix of tracers (entry number + 1, 0 where nothing is stored)"""
        rows, cols = call
        ncol = self.lens.size
        tracer = np.zeros((self.nrow, ncol), dtype=np.int32, order="F")
        tracer[self.ri, np.repeat(np.arange(ncol), self.lens)] = np.arange(self.total, dtype=np.int32) + 1
        r = np.arange(self.nrow) if rows is None else rows.astype(np.int64)
        c = np.arange(ncol) if cols is None else cols.astype(np.int64)
        assert r.size * c.size <= 8 * CELLS
        flat = np.asfortranarray(tracer[np.ix_(r, c)]).reshape(-1, order="F")
        at = np.flatnonzero(flat)
        cp = np.zeros(c.size + 1, dtype=np.int64)
        if r.size:
            np.cumsum(np.bincount(at // r.size, minlength=c.size), out=cp[1:])
        return cp, (at % max(r.size, 1)).astype(np.int32), self.val[flat[at] - 1]


def same_csc(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    assert got[2].dtype == want[2].dtype and np.array_equal(sc.bits(got[2]), sc.bits(want[2])), f"{what}: val as bits"


# ---------------------------------------------------------------------------
# Arith / Math
# ---------------------------------------------------------------------------
SHARES = (0.0, 0.01, 0.5, 0.99, 1.0)
TYPE_PAIRS = (("double", "double"), ("integer", "integer"), ("integer", "double"), ("double", "integer"))
SCALARS = ((3, "integer"), (2.5, "double"), (0.0, "double"), (-3, "integer"), (0.5, "double"), (2, "integer"))


class PairKeys:
    """The key bookkeeping of two operands x and y on one grid (nrow, ncol), as linear keys column * nrow + row: the
    merged sequence of the two has ``merged`` places, a figure drawn around the tile T of the merge; ``share`` of y's
    positions are x's too, and where the operands share positions at all, a pair is planted across every tile edge.
    Shared by every family of the merge kernels (Arith, Compare / Logic, pmin / pmax)."""

    def _draw_keys(self, rng, T, full_column, share=None, shift_pairs=False):
        """.T .share .merged .nrow .ncol .kx .ky; ``share``: given (a family whose shares go round with the seed) or
        drawn from SHARES; ``shift_pairs``: see _plant_pairs_across_tiles"""
        self.T, self.shift_pairs = T, shift_pairs
        self.share = SHARES[int(rng.integers(0, 5))] if share is None else share
        self.merged = M = draw_total(rng, T)
        y0 = M / (2 + self.share)
        both = int(round(self.share * y0))
        npos = M - both
        ny = both if self.share == 1.0 else min(npos, max(both, int(round(y0))))
        self.nrow, lens = draw_columns(rng, npos, full_column)
        cp, ri = place(rng, self.nrow, lens)
        self.ncol = lens.size
        keys = np.repeat(np.arange(self.ncol, dtype=np.int64), lens) * self.nrow + ri
        pick = rng.permutation(npos)
        in_both, y_only = pick[:both], pick[both:ny]
        is_y = np.zeros(npos, bool)
        is_y[pick[:ny]] = True
        is_x = np.ones(npos, bool)
        is_x[y_only] = False
        if both:
            self._plant_pairs_across_tiles(is_x, is_y)
        self.kx, self.ky = keys[is_x], keys[is_y]
        assert self.kx.size + self.ky.size == M and np.intersect1d(self.kx, self.ky).size == both == in_both.size

    def _plant_pairs_across_tiles(self, is_x, is_y):
        """Where operands share positions at all: the position whose entry sits at the last merged place of a tile is
        made a shared one, so that its pair straddles the boundary (x's entry closes the tile, y's opens the next);
        a shared position further on becomes a single one, which keeps the merged length and the count of pairs.
        Under ``shift_pairs`` (the families after Arith, whose plain draw left a pair across an edge in three seeds of
        eight) a pair that ends on the last place of a tile is moved one place on as well: it hands its y entry to the
        single position behind it, or, where a pair stands there, the nearest single position in front of it is made
        a shared one at the price above."""
        for b in range(self.T, self.merged, self.T):
            width = is_x.astype(np.int64) + is_y
            start = np.cumsum(width) - width                # the first merged place of every position
            j = int(np.searchsorted(start, b - 1, side="right")) - 1
            later = np.flatnonzero(width[j + 1:] == 2)
            if self.shift_pairs and width[j] == 2 and start[j] == b - 2:
                single = np.flatnonzero(width[:j] == 1)
                if j + 1 < width.size and width[j + 1] == 1:
                    is_x[j], is_y[j] = True, False
                    is_x[j + 1] = is_y[j + 1] = True
                elif single.size and later.size:
                    is_x[single[-1]] = is_y[single[-1]] = True
                    is_y[j + 1 + later[-1]] = False
                continue
            if width[j] != 1 or later.size == 0:
                continue                                    # (a pair is there already: it straddles, or ends at b - 1)
            is_x[j] = is_y[j] = True
            is_y[j + 1 + later[-1]] = False

    def csc(self, which):
        k, v = (self.kx, self.vx) if which == "x" else (self.ky, self.vy)
        return ac._csc(k, v, self.nrow, self.ncol)

    def straddling_keys(self):
        """the keys of the pairs (an x entry and a y entry of one position) whose two merged places lie in different
        tiles"""
        keys, _ = ac.merged_places(self.kx, self.ky)
        first = np.flatnonzero(keys[1:] == keys[:-1])      # the place of a pair's x entry; y's is the next
        return keys[first[(first + 1) % self.T == 0]]

    def pairs_straddling_a_tile(self):
        return int(self.straddling_keys().size)

    def shared(self):
        """(places in x, places in y) of the positions that both operands store"""
        both = np.intersect1d(self.kx, self.ky)
        return np.searchsorted(self.kx, both), np.searchsorted(self.ky, both)


class ArithCase(PairKeys):
    """x op y, x op scalar, -x and Math on the keys of PairKeys, the share drawn"""

    def __init__(self, seed, T):
        rng = np.random.default_rng([seed, 2])
        self.seed = seed
        self.types = TYPE_PAIRS[seed % 4]
        self._draw_keys(rng, T, seed % 5 == 0)
        self.vx = mixed_values(rng, self.kx.size, self.types[0])
        self.vy = mixed_values(rng, self.ky.size, self.types[1])
        self.scalar_op = ac.SCALAR_OPS[(seed + int(rng.integers(0, 5))) % 5]
        self.scalar = SCALARS[int(rng.integers(0, len(SCALARS)))]
        self.math_op = ac.MATH_OPS[(seed + int(rng.integers(0, 8))) % 8]
        # (name, kind, arguments): the three merges, one scalar operation, unary minus; Math where x is a double
        self.calls = [(f"x {op} y", "merge", op) for op in ac.MERGE_OPS]
        self.calls += [(f"x {self.scalar_op} {self.scalar[0]}", "scalar", (self.scalar_op,) + self.scalar), ("-x", "neg", None)]
        if self.types[0] == "double":
            self.calls.append((f"{self.math_op}(x)", "math", self.math_op))

    def expected(self, call):
        """R's rule on the positions stored in an operand (everywhere else 0 op 0 is an implicit zero): (keys, Expected
        over those keys, the result's type); the element-wise functions are arith_cases' own"""
        _, kind, arg = call
        tx, ty = self.types
        if kind == "merge":
            keys = np.union1d(self.kx, self.ky)
            dx, dy = np.zeros(keys.size, dtype=self.vx.dtype), np.zeros(keys.size, dtype=self.vy.dtype)
            dx[np.searchsorted(keys, self.kx)] = self.vx
            dy[np.searchsorted(keys, self.ky)] = self.vy
            t = ac.out_type("merge", arg, tx, ty)
            if t == "integer":
                v, over = ac._int_arith(arg, dx, dy)
                return keys, ac.Expected(t, v, None, np.ones(keys.size, bool), over), None
            v, cls = ac._double_arith(arg, ac.as_double(dx), ac.as_double(dy))
            return keys, ac.Expected(t, v, cls, np.ones(keys.size, bool)), None
        keys, x, on = self.kx, self.vx, np.ones(self.kx.size, bool)
        if kind == "neg":
            v = np.where(x == NA_integer, NA_integer, -x.astype(np.int64)).astype(np.int32) if tx == "integer" else np.negative(x)
            return keys, ac.Expected(tx, v, None, on), None
        if kind == "math":
            v, cls = ac._math(arg, x)
            return keys, ac.Expected("double", v, cls, on, from_na=ac.is_NA_real(x)), arg if arg in ac.ULPS_MATH else None
        op, s, st = arg
        t = ac.out_type("scalar", op, tx, st)
        if t == "integer":
            v, over = ac._int_arith(op, x, np.int32(s))
            return keys, ac.Expected(t, v, None, on, over), None
        xd = ac.as_double(x)
        v, cls = ac._double_arith(op, xd, np.float64(s))
        return keys, ac.Expected(t, v, cls, on, from_na=ac.is_NA_real(xd)), "^" if op == "^" else None

    def compare(self, call, got, max_ulps=0):
        """``got``: the result's (col_ptr, row_idx, val) and overflow word against expected(call)"""
        (cp, ri, val), overflow = got
        keys, e, _ = self.expected(call)
        what = f"seed {self.seed}: {call[0]}"
        assert cp.size == self.ncol + 1 and cp[0] == 0 and cp[-1] == ri.size == val.size, f"{what}: col_ptr"
        gk = np.repeat(np.arange(self.ncol, dtype=np.int64), np.diff(cp)) * self.nrow + ri
        assert np.all(np.diff(gk) > 0), f"{what}: the entries do not ascend"
        assert ri.size == 0 or (ri.min() >= 0 and ri.max() < self.nrow), f"{what}: a row outside [0, nrow)"
        assert np.isin(gk, keys).all(), f"{what}: an entry where neither operand stores one"
        dense = np.zeros(keys.size, dtype=val.dtype)
        stored = np.zeros(keys.size, bool)
        at = np.searchsorted(keys, gk)
        dense[at], stored[at] = val, True
        assert bool(overflow) == e.overflow, f"{what}: the overflow word"
        return ac.compare(dense, stored, e, what, max_ulps)


# ---------------------------------------------------------------------------
# order statistics and ranks: value classes of a column
# ---------------------------------------------------------------------------
CLASSES = ("normal", "few_distinct", "last_bits", "mostly_negative", "huge", "inf", "missing", "stored_zeros")
FILLS = (0.02, 0.4, 0.6, 1.0)


def class_column(rng, cls, nrow, n, type):
    """(rows, values) of ``n`` stored entries of a column of the class; the values are doubles, integer-valued and
    with NaN for NA where ``type`` is integer.  few_distinct: at most 3 values (more than 1024 copies each in a
    5000-row column); last_bits: 1 + k 2^-52, k < 1024 (integers: 2^30 + k)."""
    rows = np.sort(rng.choice(nrow, size=n, replace=False))
    if cls == "few_distinct":
        v = rng.choice(np.array([-1.5, 2.5, 7.0])[: int(rng.integers(1, 4))], size=n)
    elif cls == "last_bits":
        k = rng.integers(0, 1024, size=n)
        v = 1.0 + k * 2.0 ** -52 if type == "double" else 2.0 ** 30 + k
    elif cls == "mostly_negative":
        v = np.where(rng.random(n) < 0.9, -np.abs(rng.normal(size=n)) - 0.5, np.abs(rng.normal(size=n)) + 0.5)
    elif cls == "huge":
        v = rng.normal(size=n) * (1e200 if type == "double" else 1e9)
    else:
        v = np.round(rng.normal(size=n), 2)
    if type == "integer" and cls != "last_bits":
        v = np.round(v * (1 if cls == "huge" else 1000)).clip(-2e9, 2e9)
    if cls != "stored_zeros":
        v[v == 0] = 1.0
    if n:
        some = rng.choice(n, size=min(n, int(rng.integers(1, 6))), replace=False)
        if cls == "inf":
            v[some] = rng.choice([np.inf, -np.inf], size=some.size) if type == "double" else rng.choice([INT_MAX, -INT_MAX], size=some.size)
        elif cls == "missing":
            v[some] = np.nan
            if type == "double":
                v = v.copy()
                v[some[0]] = NA_real
        elif cls == "stored_zeros":
            v[some] = 0.0
            if type == "double":
                v[some[::2]] = -0.0
    return rows, v


class ColumnsCase:
    """a CSC operand built column by column from (class, stored length): .nrow .type .cp .ri .val (int32 with
    NA_integer for an integer operand) .dense (doubles, NaN = missing) .classes"""

    def _build(self, rng, nrow, type, columns):
        self.nrow, self.type, self.classes = nrow, type, [c for c, _ in columns]
        parts = [class_column(rng, c, nrow, n, type) for c, n in columns]
        self.cp = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([r.size for r, _ in parts], out=self.cp[1:])
        self.ri = np.concatenate([r for r, _ in parts]).astype(np.int32)
        v = np.concatenate([v for _, v in parts])
        self.dense = np.zeros((nrow, len(parts)), order="F")
        self.dense[self.ri, np.repeat(np.arange(len(parts)), np.diff(self.cp))] = v
        self.val = v if type == "double" else np.where(np.isnan(v), NA_integer, v).astype(np.int32)

    def svt(self):
        return svt_of(self.nrow, self.type, self.cp, self.ri, self.val)


class OrderStatCase(ColumnsCase):
    """``tall``: the 40 000-row operand of the seed (two columns) instead of the 5000-row one (16 columns)"""

    def __init__(self, seed, tall=False):
        rng = np.random.default_rng([seed, 3, int(tall)])
        self.seed, type = seed, ("double", "integer")[seed % 2]
        nrow = 40_000 if tall else 5000
        if tall:
            columns = [("normal", int(0.6 * nrow)), (CLASSES[1 + seed % 7], nrow)]
        else:
            order = rng.permutation(16)
            columns = [(CLASSES[j % 8], int(round(FILLS[int(rng.integers(0, 4))] * nrow))) for j in order]
        self._build(rng, nrow, type, columns)
        ncol = len(columns)
        pool = [0.0, 1.0, 0.5, 1 / 3, int(rng.integers(0, nrow)) / (nrow - 1)] + rng.random(3).tolist()
        self.probs = tuple(float(p) for p in rng.choice(pool, size=int(rng.integers(1, 8))))
        cen = np.round(rng.normal(size=ncol), 1) * (1000 if type == "integer" else 1)
        cen[int(rng.integers(0, ncol))] = [np.nan, np.inf][seed % 2]
        self.center = cen
        # (name, function, arguments)
        self.calls = [(f"{f} na_rm={na_rm}", f, na_rm) for f in ("colmedians", "colquantiles", "colmads", "colmads_center")
                      for na_rm in (False, True)]

    def expected(self, call):
        _, f, na_rm = call
        if f == "colmedians":
            return dense_colmedians(self.dense, na_rm)
        if f == "colquantiles":
            return dense_colquantiles(self.dense, self.probs, na_rm)
        return dense_colmads(self.dense, self.center if f == "colmads_center" else None, 1.4826, na_rm)


class RanksCase(ColumnsCase):
    def __init__(self, seed, limits):
        rng = np.random.default_rng([seed, 4])
        f0, f1 = limits
        self.seed, type = seed, ("double", "integer")[(seed // 2) % 2]
        self.stored_zeros = bool(seed % 2)
        nrow = int(rng.integers(f1 + 1, f1 + 3001))
        lengths = [f0, f0 + 1, f1, max(1, f0 - 1), int(rng.integers(0, 4)), int(rng.integers(f0 + 2, f1)), 0,
                   int(rng.integers(1, f0 + 1))]
        if rng.random() < 0.75:
            lengths.append(f1 + 1)                          # the one long column of the seed
        lengths = [lengths[j] for j in rng.permutation(len(lengths))]
        pool = [c for c in CLASSES if c != "stored_zeros"]
        classes = [pool[int(rng.integers(0, len(pool)))] for _ in lengths]
        if self.stored_zeros:
            for j in rng.choice(len(lengths), size=3, replace=False):
                classes[j] = "stored_zeros"
        self.lengths = lengths
        self._build(rng, nrow, type, list(zip(classes, lengths)))
        self.calls = [(f"colranks {t}", t) for t in TIES]

    def expected(self, call):
        return dense_colranks(self.dense, call[1])

    def expand(self, rank_nz, zero_rank):
        return expand_ranks(self.nrow, self.cp, self.ri, rank_nz, zero_rank)


# ---------------------------------------------------------------------------
# shared by the five families on the merge, map and sweep tile kernels
# ---------------------------------------------------------------------------
TYPE_ORDER = ("logical", "integer", "double")
ZERO_SHARES = (0.3, 1.0, 0.0)


def round_share(seed):
    """the share of y's positions that are x's too, going round with the seed: 1, 0.99, 0.5, 0.01, 0, 1, 0.99, 0.5"""
    return SHARES[(4 - seed) % 5]


def keys_of(csc, nrow):
    cp, ri, _ = csc
    return np.repeat(np.arange(cp.size - 1, dtype=np.int64), np.diff(cp)) * nrow + ri


def draw_scalar(rng, signs, vx):
    """(s, its R type) with sign(s) drawn from ``signs``: a Python bool (logical; 0 or 1, so never where the sign
    drawn is negative), int (integer) or float (double); the magnitude is that of an ordinary value of x seven times
    in ten (so that == and the ties of <= and >= meet something), else an integer below 60"""
    sign = int(signs[int(rng.integers(0, len(signs)))])
    st = TYPE_ORDER[int(rng.integers(0, 3))]
    if st == "logical" and sign < 0:
        st = "integer"
    if st == "logical":
        return bool(sign), st
    xd = ac.as_double(np.asarray(vx))
    ordinary = np.abs(xd[np.isfinite(xd) & (xd != 0)])
    if ordinary.size and rng.random() < 0.7:
        mag = float(ordinary[int(rng.integers(0, ordinary.size))])
    else:
        mag = float(rng.integers(1, 60))
    if st == "integer":
        return sign * max(1, int(mag)), st
    return float(sign * mag), st


def with_zeros(rng, v, share):
    v = v.copy()
    v[rng.random(v.size) < share] = 0
    return v


def factorise(rng, n, k):
    """n as a product of k extents: its prime factors dealt to them at random (an extent of 1 is an extent)"""
    ext, m, p = [1] * k, int(n), 2
    while m > 1:
        while m % p == 0:
            ext[int(rng.integers(0, k))] *= p
            m //= p
        p += 1
    return tuple(ext)


def same_csc_by_class(got, want, cls, what, max_ulps=0):
    """CSC triples: col_ptr and row_idx exactly, the values by their class of arith_cases (bits; a NaN's payload; NaN-ness;
    ulps from the correctly rounded value, an NA staying NA); returns the largest ULPS distance seen"""
    assert np.array_equal(got[0], want[0]), f"{what}: col_ptr"
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: row_idx"
    t = "double" if want[2].dtype == np.float64 else "integer"
    on = np.ones(want[2].shape, bool)
    e = ac.Expected(t, want[2], cls, on, from_na=ac.is_NA_real(want[2]) if t == "double" else None)
    assert np.array_equal(e.stored, on), f"{what}: the expectation stores a zero"
    return ac.compare(got[2], on, e, what, max_ulps)


# ---------------------------------------------------------------------------
# Compare / Logic: the merge and map kernels under ARI_RULE_COMPARE and ARI_RULE_LOGIC
# ---------------------------------------------------------------------------
COMPARE_TYPE_PAIRS = (("double", "double"), ("logical", "logical"), ("integer", "double"), ("double", "integer"),
                      ("integer", "integer"), ("logical", "logical"), ("logical", "integer"), ("double", "logical"))
EQUAL_SHARES = (1.0, 0.5, 0.1)
# the signs of a scalar s under which 0 op s is FALSE: == takes any s != 0, != takes s == 0 alone, <= takes s < 0,
# >= takes s > 0, < takes s <= 0, > takes s >= 0
SCALAR_SIGNS = {"==": (-1, 1), "!=": (0,), "<=": (-1,), ">=": (1,), "<": (-1, 0), ">": (0, 1)}


class CompareCase(PairKeys):
    """x op y for the three merge operators (and & | where both are logical), x op s for the six operators with a scalar
    per operator under which zero compares FALSE (SCALAR_SIGNS), and one scalar that breaks that rule (.refused).  The
    keys are PairKeys'; the share goes round with the seed (round_share), and so do the type pair and ``equal``, the
    share of the shared positions at which y's value is x's (widened to the wider type of the two): there != < and >
    give FALSE, and a pair that closes a tile is dropped.  The rest is mixed_values: an NA gives an NA, which is kept."""

    def __init__(self, seed, T):
        rng = np.random.default_rng([seed, 5])
        self.seed = seed
        self.types = tx, ty = COMPARE_TYPE_PAIRS[seed % 8]
        self.equal = EQUAL_SHARES[seed % 3]
        self._draw_keys(rng, T, seed % 5 == 0, share=round_share(seed), shift_pairs=True)
        self.vx = mixed_values(rng, self.kx.size, tx)
        self.vy = mixed_values(rng, self.ky.size, ty)
        ix, iy = self.shared()
        same = rng.random(ix.size) < self.equal
        if TYPE_ORDER.index(ty) >= TYPE_ORDER.index(tx):
            self.vy[iy[same]] = pc.widen(self.vx[ix[same]], ty)
        else:
            self.vx[ix[same]] = pc.widen(self.vy[iy[same]], tx)
        self.calls = [(f"x {op} y", "merge", op) for op in cc.MERGE_OPS]
        if self.types == ("logical", "logical"):
            self.calls += [(f"x {op} y", "logic", op) for op in cc.LOGIC_OPS]
        for op in cc.COMPARE_OPS:
            s, st = draw_scalar(rng, SCALAR_SIGNS[op], self.vx)
            self.calls.append((f"x {op} {s!r}", "scalar", (op, s, st)))
        op = tuple(cc.COMPARE_OPS)[int(rng.integers(0, 6))]
        self.refused = (op,) + draw_scalar(rng, tuple(k for k in (-1, 0, 1) if k not in SCALAR_SIGNS[op]), self.vx)

    def expected(self, call):
        """(col_ptr, row_idx, int32 values 1 / NA) by compare_cases' own element-wise rules"""
        _, kind, arg = call
        if kind == "scalar":
            op, s, st = arg
            return cc.map_expect(op, *self.csc("x"), s, st, self.ncol)
        return cc.device_expect("compare" if kind == "merge" else "logic", arg, self.kx, self.vx, self.ky, self.vy,
                                self.nrow, self.ncol)

    def positions(self, call):
        """the positions a call looks at: the union of the keys, or x's"""
        return self.kx.size if call[1] == "scalar" else np.union1d(self.kx, self.ky).size

    def straddling_pairs_dropped(self, call):
        return int((~np.isin(self.straddling_keys(), keys_of(self.expected(call), self.nrow))).sum())


# ---------------------------------------------------------------------------
# pmin / pmax and is.na / is.nan / is.infinite: the merge and map kernels under ARI_RULE_PMINMAX, the map under _ISFUN
# ---------------------------------------------------------------------------
PMINMAX_TYPE_PAIRS = (("double", "double"), ("integer", "logical"), ("logical", "double"), ("double", "integer"),
                      ("integer", "integer"), ("logical", "logical"), ("integer", "double"), ("double", "logical"))
PMINMAX_VARIANTS = tuple((op, na_rm) for op in pc.OPS for na_rm in (False, True))
# pmin(0, s) == 0 takes s >= 0, pmax(0, s) == 0 takes s <= 0
PMINMAX_SIGNS = {"pmin": (0, 1), "pmax": (-1, 0)}


class PminmaxCase(PairKeys):
    """pmin and pmax with both na_rm values against an operand (keys and shares as in CompareCase) and against a scalar
    that keeps the result sparse, and the three is*() on x.  A double x carries a specials share of 0.1 (NA, NaNs of
    two payloads, both infinities, zeros of both signs); an integer or logical x gives an empty is.nan and an empty
    is.infinite."""

    def __init__(self, seed, T):
        rng = np.random.default_rng([seed, 7])
        self.seed = seed
        self.types = tx, ty = PMINMAX_TYPE_PAIRS[seed % 8]
        self._draw_keys(rng, T, seed % 5 == 0, share=round_share(seed), shift_pairs=True)
        self.vx = mixed_values(rng, self.kx.size, tx, share=0.1)
        self.vy = mixed_values(rng, self.ky.size, ty)
        self.calls = [(f"{op}(x, y, na_rm={na_rm})", "merge", (op, na_rm)) for op, na_rm in PMINMAX_VARIANTS]
        for op, na_rm in PMINMAX_VARIANTS:
            s, st = draw_scalar(rng, PMINMAX_SIGNS[op], self.vx)
            assert pc.keeps_sparse(op, s, st)
            self.calls.append((f"{op}(x, {s!r}, na_rm={na_rm})", "scalar", (op, na_rm, s, st)))
        self.calls += [(f"{fn}(x)", "isfun", fn) for fn in pc.ISFUNS]

    def expected(self, call):
        """((col_ptr, row_idx, val), the result's type) by pminmax_cases' closed formula"""
        _, kind, arg = call
        tx, ty = self.types
        if kind == "merge":
            return pc.expect_merge(*arg, self.nrow, self.ncol, self.kx, self.vx, tx, self.ky, self.vy, ty)
        if kind == "scalar":
            op, na_rm, s, st = arg
            return pc.expect_map(op, na_rm, self.csc("x"), tx, s, st)
        return pc.expect_isfun(arg, self.csc("x")), "logical"


# ---------------------------------------------------------------------------
# sweep(): arith_sweep_* under ARI_RULE_ARITH, _COMPARE and _PMINMAX
# ---------------------------------------------------------------------------
SWEEP_ARITH_ST = ("double", "integer", "double", "integer", "integer", "integer", "double", "integer")
SWEEP_ST = ("logical", "double", "integer")


def align_tile_on_leaf(lens, T, nrow):
    """Rearranges ``lens`` in place, keeping its sum and its size, so that the second tile of T entries starts on the
    first entry of a leaf that stands behind an empty leaf: the first empty leaf after the leaf j that holds entry
    T - 1 is moved right behind j, and what j holds past entry T - 1 goes to the leaf after that.  False, and nothing
    changed, where there is no second tile, no empty leaf after j, or no room in that leaf."""
    cp = np.concatenate([[0], np.cumsum(lens)])
    if cp[-1] <= T:
        return False
    j = int(np.searchsorted(cp, T, side="left")) - 1          # cp[j] < T <= cp[j + 1]
    spill = int(cp[j + 1]) - T
    empty = np.flatnonzero(lens[j + 1:] == 0)
    if empty.size == 0 or j + 2 >= lens.size:
        return False
    z = j + 1 + int(empty[0])
    after = int(lens[j + 1] if z > j + 1 else lens[j + 2])
    if after + spill > nrow:
        return False
    lens[j + 1:z + 1] = np.roll(lens[j + 1:z + 1], 1)
    lens[j] -= spill
    lens[j + 2] += spill
    return True


class SweepCase:
    """One operand from draw_columns around the Arith tile, read as the array of extents ``dim`` = (nrow, ...): ncol
    factorised into 1 + seed % 3 trailing extents; ``margin``: a drawn run of consecutive dimensions.  Three calls, the
    operations going round with the seed: one of * / ^ %% %/%, one of the six comparisons, pmin or pmax with one of the
    na_rm values; the type of STATS goes round double, integer and logical (logical for Compare and pmin / pmax only,
    and never for <= and <, which take negative elements).  STATS is sweep_cases.stats_for's -- for pmin what > takes,
    for pmax what < takes; a logical one is its sign (its parity too for pmin).  ``refused``: one of the three calls
    again with two invalid elements planted.

    A rule added because the plain draw missed the condition in all eight seeds: on the odd seeds align_tile_on_leaf
    moves entries so that the second tile starts exactly on a leaf boundary behind an empty leaf, where the columns
    drawn allow it."""

    def __init__(self, seed, T):
        from sparsearray_amd.device import sweep_form
        rng = np.random.default_rng([seed, 6])
        self.seed, self.T = seed, T
        self.type = ("double", "integer")[seed % 2]
        self.total = draw_total(rng, T)
        self.nrow, self.lens = draw_columns(rng, self.total, seed % 5 == 0)
        self.aligned = bool(seed % 2) and align_tile_on_leaf(self.lens, T, self.nrow)
        self.cp, self.ri = place(rng, self.nrow, self.lens)
        self.val = mixed_values(rng, self.total, self.type)
        self.ncol = self.lens.size
        self.dim = (self.nrow,) + factorise(rng, self.ncol, 1 + seed % 3)
        first = 1 + int(rng.integers(0, len(self.dim)))
        self.margin = tuple(range(first, first + 1 + int(rng.integers(0, len(self.dim) - first + 1))))
        self.with_rows, self.stride, self.len = sweep_form(self.dim, self.margin)
        n = sw.stats_length(self.dim, self.margin)
        p_op, na_rm = PMINMAX_VARIANTS[seed % 4]
        # (name, rule, op, na_rm, the type of STATS, STATS)
        self.calls = [self._call("arith", sw.ARITH_OPS[seed % 5], False, SWEEP_ARITH_ST[seed], n),
                      self._call("compare", sw.COMPARE_OPS[seed % 6], False, SWEEP_ST[seed % 3], n),
                      self._call("pminmax", p_op, na_rm, SWEEP_ST[(seed + 1) % 3], n)]
        name, rule, op, na_rm, st, stats = self.calls[seed % 3]
        at = rng.choice(n, size=min(2, n), replace=False)
        bad = stats.copy()
        # zero fills the result under / ^ %% %/%; NA does under every other operation
        bad[at] = 0 if op in ("/", "^", "%%", "%/%") else NA_real if st == "double" else NA_integer
        self.refused = (name, rule, op, na_rm, st, bad), int(at.min())

    def _call(self, rule, op, na_rm, st, n):
        like = {"pmin": ">", "pmax": "<"}.get(op, op)
        v = sw.stats_for(like, n, "integer" if st == "logical" else st, seed=self.seed)
        if st == "logical":
            v = ((v > 0) & ((v % 2 == 1) | (op != "pmin"))).astype(np.int32)
        return f"sweep {op} {st} margin {self.margin}" + (f" na_rm={na_rm}" if rule == "pminmax" else ""), rule, op, na_rm, st, v

    def csc(self):
        return self.cp, self.ri, self.val

    def expected(self, call):
        """((col_ptr, row_idx, val), classes of arith_cases or None, the result's type, the overflow flag or None) by
        sweep_cases.expect_csc or pminmax_cases.expect_sweep"""
        _, rule, op, na_rm, st, stats = call
        if rule == "pminmax":
            want, t = pc.expect_sweep(op, na_rm, self.csc(), self.type, self.dim, self.margin, stats, st)
            return want, None, t, None
        want, cls, t, over = sw.expect_csc(op, self.nrow, self.csc(), self.dim, self.margin, stats, st)
        return want, cls, t, (over if rule == "arith" else None)

    def tiles(self):
        """per tile of T entries: (first leaf, last leaf, non-empty leaves that start in it, whether it starts on a
        leaf's first entry behind an empty leaf)"""
        col = np.repeat(np.arange(self.ncol), self.lens)
        out = []
        for b in range(0, self.total, self.T):
            e = min(b + self.T, self.total)
            q0, q1 = int(col[b]), int(col[e - 1])
            starts = int(((self.cp[:-1] >= b) & (self.cp[:-1] < e) & (self.lens > 0)).sum())
            out.append((q0, q1, starts, bool(b > 0 and self.cp[q0] == b and q0 > 0 and self.lens[q0 - 1] == 0)))
        return out


# ---------------------------------------------------------------------------
# subassignment by N-index: the placement of kernels_subassign.hip, then the merge under ARI_RULE_ASSIGN
# ---------------------------------------------------------------------------
ASSIGN_TYPE_PAIRS = (("double", "double"), ("integer", "double"), ("double", "integer"), ("logical", "integer"),
                     ("integer", "logical"), ("logical", "double"), ("double", "logical"), ("integer", "integer"))
ASSIGN_ROW_KINDS = ("whole_axis", "increasing", "permutation", "repeats", "single", "empty")
ASSIGN_LEAF_KINDS = ("whole_axis", "reversed", "repeats", "empty")
_ROWS_AS = {"whole_axis": "none", "increasing": "increasing_half", "permutation": "permutation",
            "repeats": "repeats_longer_than_the_axis", "single": "single", "empty": "empty"}


def _size(sub, extent):
    return extent if sub is None else sub.size


def _divisor(rng, n):
    d = [k for k in range(1, n + 1) if n % k == 0] if n else [1]
    return d[int(rng.integers(0, len(d)))]


class SubassignCase:
    """x from draw_columns around the Arith tile (the merge's); ``cover``: a number of cells drawn around the tile P of
    the placement, which the subscripts of a call cover about.  The row kind and the leaf kind go round with the seed;
    a call takes one of them and fits the other subscript -- increasing, drawn, the longest leaf among the leaves --
    to the cover.  Calls: (name, rows, leaves, value), 0-based subscripts or None, the value a vector of the value type
    or, for the SVT form, (nrow, col_ptr, row_idx, val):
      delete       rows of the kind: scalar 0 -- a pure deletion, an empty placed operand over x
      scalar       leaves of the kind: a scalar that is not zero
      vector       rows of the kind: a vector recycled over them (its length a drawn divisor; as long as the subscript
                   for the repeats, whose last occurrence wins) with a zeros share of 0.3, 1 or 0
      empty_cover  leaves that x leaves empty (where it has some): x has no entry under the cover
      svt          rows strictly increasing, up to 40 leaves without repeats in a drawn order, a value operand with
                   stored zeros"""

    def __init__(self, seed, T, P):
        rng = np.random.default_rng([seed, 8])
        self.seed = seed
        self.types = tx, tv = ASSIGN_TYPE_PAIRS[seed % 8]
        self.total = draw_total(rng, T)
        self.nrow, self.lens = draw_columns(rng, self.total, seed % 5 == 0)
        self.cp, self.ri = place(rng, self.nrow, self.lens)
        self.val = mixed_values(rng, self.total, tx)
        self.ncol = ncol = self.lens.size
        self.cover = draw_total(rng, P)
        self.row_kind, self.leaf_kind = ASSIGN_ROW_KINDS[seed % 6], ASSIGN_LEAF_KINDS[seed % 4]
        self.zeros = ZERO_SHARES[seed % 3]
        rows = _rows(rng, _ROWS_AS[self.row_kind], self.nrow)
        leaves = _cols(rng, {"whole_axis": "none"}.get(self.leaf_kind, self.leaf_kind), self.lens)
        few_leaves = self._fit(rng, ncol, _size(rows, self.nrow), keep=int(np.argmax(self.lens)))
        few_rows = self._fit(rng, self.nrow, _size(leaves, ncol))
        nvals = _size(rows, self.nrow) if self.row_kind == "repeats" else _divisor(rng, _size(rows, self.nrow))
        one = np.ones(1, np.int32) if tv == "logical" else mixed_values(rng, 1, tv, share=0.0)
        unused = np.flatnonzero(self.lens == 0)
        no_entry = np.sort(rng.choice(unused, size=min(3, unused.size), replace=False)).astype(np.int32) if unused.size else few_leaves
        svt_leaves = rng.permutation(ncol)[:min(ncol, int(rng.integers(1, 41)))].astype(np.int32)
        if int(np.argmax(self.lens)) not in svt_leaves:
            svt_leaves[int(rng.integers(0, svt_leaves.size))] = int(np.argmax(self.lens))
        svt_rows = self._fit(rng, self.nrow, svt_leaves.size)
        v_lens = rng.binomial(svt_rows.size, 0.6, size=svt_leaves.size).astype(np.int64)
        v_cp, v_ri = place(rng, svt_rows.size, v_lens)
        v_val = with_zeros(rng, mixed_values(rng, int(v_lens.sum()), tv), 0.1)
        self.calls = [("delete", rows, few_leaves, np.zeros(1, sc.NP_DTYPE[tv])),
                      ("scalar", few_rows, leaves, one),
                      ("vector", rows, few_leaves, with_zeros(rng, mixed_values(rng, nvals, tv), self.zeros)),
                      ("empty_cover", few_rows, no_entry, with_zeros(rng, mixed_values(rng, _divisor(rng, few_rows.size), tv), 0.3)),
                      ("svt", svt_rows, svt_leaves, (svt_rows.size, v_cp, v_ri, v_val))]

    def _fit(self, rng, extent, other, keep=None):
        """an increasing subscript of about cover / other elements of the axis"""
        n = min(extent, max(1, self.cover // max(other, 1)))
        s = rng.choice(extent, size=n, replace=False)
        if keep is not None and keep not in s:
            s[0] = keep
        return np.sort(s).astype(np.int32)

    def csc(self):
        return self.cp, self.ri, self.val

    def expected(self, call):
        """((col_ptr, row_idx, val), the result's type): subassign_cases.restate, the rule leaf by leaf"""
        _, rows, leaves, value = call
        tx, tv = self.types
        x = svt_of(self.nrow, tx, self.cp, self.ri, self.val)
        if isinstance(value, tuple):
            value = SVT_SparseArray.from_csc((value[0], value[1].size - 1), tv, *value[1:])
        index = [None if s is None else s.astype(np.int64) + 1 for s in (rows, leaves)]
        res = sa.restate(x, index, value, tv)
        assert res.type == sa.wider(tx, tv) and res.dim == (self.nrow, self.ncol)
        return res.to_csc(), res.type

    def entries_under(self, call):
        """x's entries on a selected row of a selected leaf"""
        _, rows, leaves, _ = call
        col = np.repeat(np.arange(self.ncol), self.lens)
        on = np.ones(self.total, bool) if rows is None else np.isin(self.ri, rows)
        return int((on & (np.ones(self.total, bool) if leaves is None else np.isin(col, leaves))).sum())

    def repeated_rows_ending_in_zero(self, call):
        """rows that occur more than once in the subscript and whose last occurrence takes a zero"""
        _, rows, leaves, value = call
        if rows is None or isinstance(value, tuple) or rows.size == 0 or _size(leaves, self.ncol) == 0:
            return 0
        last = {int(r): p for p, r in enumerate(rows)}
        counts = np.bincount(rows, minlength=self.nrow)
        return sum(1 for r, p in last.items() if counts[r] > 1 and value[p % value.size] == 0)


# ---------------------------------------------------------------------------
# L-index and M-index: the gather and the placement of kernels_lindex.hip, then the merge under ARI_RULE_ASSIGN_CELLS
# ---------------------------------------------------------------------------
CELL_KINDS = ("increasing", "shuffled", "repeats")


class CellIndexCase:
    """.op: a lindex_cases.Operand from draw_columns around the Arith tile T (the merge's, and the figure the sort's
    tile shares; the library has no accessor for the latter), its leaves read as 1 + seed % 2 trailing extents (one
    leaf: a 1-d array, L-index only).  ``K`` is drawn from 1, 255, 256, 257 and T -+ k, at most the cells there are;
    half of the K distinct cells are stored ones where the array is not nearly full.  Kinds, going round with the seed:
    increasing (what nzwhich() gives: the sorted route), shuffled, repeats (the K cells and T + k copies of one stored
    cell, shuffled: a run of equal keys longer than a tile).  ``gather``: the index with LINDEX_NA spliced in on the odd
    seeds.  ``value``: 1, 3 or len(L) values going round, with a zeros share; the repeats take len(L) values, and on
    an even seed the last occurrence of the repeated cell takes a zero: it deletes a stored entry."""

    def __init__(self, seed, T, passes):
        rng = np.random.default_rng([seed, 9])
        self.seed, self.T = seed, T
        self.types = tx, tv = ASSIGN_TYPE_PAIRS[(seed + 3) % 8]
        total = draw_total(rng, T)
        nrow, lens = draw_columns(rng, total, seed % 5 == 0)
        cp, ri = place(rng, nrow, lens)
        ncol = lens.size
        dim = (nrow,) if ncol == 1 else (nrow,) + factorise(rng, ncol, 1 + seed % 2)
        cells = np.repeat(np.arange(ncol, dtype=np.int64), lens) * nrow + ri
        self.op = op = lc.Operand(dim, tx, cells, mixed_values(rng, total, tx))
        self.passes = passes(nrow, ncol)
        k = int(rng.integers(1, 200))
        self.K = K = min(int(rng.choice([1, 255, 256, 257, T - k, T + k])), op.ncells)
        self.kind = CELL_KINDS[seed % 3]
        if op.ncells <= 4 * K:
            L = np.sort(rng.choice(op.ncells, size=K, replace=False)).astype(np.int64)
        else:
            L = rng.choice(cells, size=min(K // 2, cells.size), replace=False)
            while L.size < K:                               # (distinct cells: top up what the draw repeated)
                L = np.unique(np.concatenate([L, rng.integers(0, op.ncells, size=K - L.size)]))
        self.repeated = None
        if self.kind == "shuffled":
            L = rng.permutation(L)
        elif self.kind == "repeats":
            self.repeated = int(cells[int(rng.integers(0, cells.size))])
            L = rng.permutation(np.concatenate([L, np.full(T + k, self.repeated, dtype=np.int64)]))
        self.L = np.ascontiguousarray(L, dtype=np.int64)
        self.gather = self.L.copy()
        if seed % 2:
            self.gather[rng.random(self.L.size) < 0.05] = lc.LINDEX_NA
        nvals = self.L.size if self.kind == "repeats" else (1, 3, self.L.size)[(seed // 3) % 3]
        self.value = with_zeros(rng, mixed_values(rng, nvals, tv), ZERO_SHARES[seed % 3])
        if self.kind == "repeats" and seed % 2 == 0:
            self.value[np.flatnonzero(self.L == self.repeated)[-1]] = 0
        self.sorted_route = bool(np.all(np.diff(self.L) > 0))
        self.with_mindex = len(dim) in (2, 3)

    def expected_gather(self, with_na=True):
        return lc.expect_subset(self.op, self.gather if with_na else self.L)

    def expected_assign(self):
        """(the result's type, the sorted stored cells, their values): lindex_cases.expect_subassign"""
        return lc.expect_subassign(self.op, self.L, self.value, self.types[1])

    def last_value_deletes_a_stored_entry(self):
        if self.repeated is None:
            return False
        last = np.flatnonzero(self.L == self.repeated)[-1]
        return bool(np.isin(self.repeated, self.op.cells) and self.value[last % self.value.size] == 0)


def same_cells(got, want, what):
    """(type, cells, values) of a result against lindex_cases.expect_subassign's: the cells exactly, the values as bits"""
    assert got[0] == want[0], f"{what}: the result is {got[0]}, expected {want[0]}"
    assert np.array_equal(got[1], want[1]), f"{what}: the stored cells differ"
    assert got[2].dtype == want[2].dtype and np.array_equal(sc.bits(got[2]), sc.bits(want[2])), f"{what}: values as bits"
