"""Seeded random cases for the four newest kernel families -- subset, Arith / Math, the count / select order statistics
and the ranks -- shared by tests/test_random_cases_cpu.py (the generators and expectations themselves, through the
oracle session where it offers the operation) and tests/test_hip_random_cases.py (the device).

Pure numpy, ``np.random.default_rng(seed)``; one seed is one case.  Each generator returns the operand arrays, the calls
and, per call, the DENSE expectation.  Structure is drawn from the constants the kernels cut by, read from the library
(subset_tile(), arith_tile(), colranks_form_limits()), never copied here.  Nothing is filtered, skipped or retried:
what a seed draws is what is compared.

Columns (subset, Arith): a total of T-1, T, T+1, 2T, 2T+1 or 3T+-k nonzeros for the family's tile T; with
probability 0.6 one column holds 50 to 95 % of them; the others come in runs -- empty runs of 1 to 600 columns, runs of
lengths 0 to 3, runs of binomial lengths -- and the last non-empty ones are trimmed to the total.  ncol is drawn from
1, 3, 40, 700, 5000 among those that keep the dense matrix of the reference under 2^23 cells (a rule of the draw, stated
here: the reference is a dense matrix).  Every fifth seed has a full column (nrow = the longest column).
"""
from __future__ import annotations

import numpy as np

import arith_cases as ac
import subset_cases as sc
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


class ArithCase:
    """x and y on one grid (nrow, ncol) as linear keys column * nrow + row; the merged sequence of the two has
    ``merged`` places, a figure drawn around the Arith tile; ``share`` of y's positions are x's too."""

    def __init__(self, seed, T):
        rng = np.random.default_rng([seed, 2])
        self.seed, self.T = seed, T
        self.types = TYPE_PAIRS[seed % 4]
        self.share = SHARES[int(rng.integers(0, 5))]
        self.merged = M = draw_total(rng, T)
        y0 = M / (2 + self.share)
        both = int(round(self.share * y0))
        npos = M - both
        ny = both if self.share == 1.0 else min(npos, max(both, int(round(y0))))
        self.nrow, lens = draw_columns(rng, npos, seed % 5 == 0)
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

    def _plant_pairs_across_tiles(self, is_x, is_y):
        """Where operands share positions at all: the position whose entry sits at the last merged place of a tile is
        made a shared one, so that its pair straddles the boundary (x's entry closes the tile, y's opens the next);
        a shared position further on becomes a single one, which keeps the merged length and the count of pairs."""
        for b in range(self.T, self.merged, self.T):
            width = is_x.astype(np.int64) + is_y
            start = np.cumsum(width) - width                # the first merged place of every position
            j = int(np.searchsorted(start, b - 1, side="right")) - 1
            later = np.flatnonzero(width[j + 1:] == 2)
            if width[j] != 1 or later.size == 0:
                continue                                    # (a pair is there already: it straddles, or ends at b - 1)
            is_x[j] = is_y[j] = True
            is_y[j + 1 + later[-1]] = False

    def csc(self, which):
        k, v = (self.kx, self.vx) if which == "x" else (self.ky, self.vy)
        return ac._csc(k, v, self.nrow, self.ncol)

    def pairs_straddling_a_tile(self):
        """pairs (an x entry and a y entry of one position) whose two merged places lie in different tiles"""
        keys, _ = ac.merged_places(self.kx, self.ky)
        first = np.flatnonzero(keys[1:] == keys[:-1])      # the place of a pair's x entry; y's is the next
        return int(((first + 1) % self.T == 0).sum())

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
