"""Operands for the branches of the sparse-result product (kernels_spgemm.hip and the table of run bounds of
kernels_rowstats.hip) that the cases of tests/spgemm_cases.py leave unrun, shared by
tests/test_zzzzzzzzzz_spgemm_branches_cpu.py (every case proved to have the property it is named for, the expectation
proved against ``spgemm_cases.expect`` and against the exact product) and tests/test_zzzzzzzzzz_spgemm_branches_hip.py
(the device kernels).  ``device_cases(P)`` of spgemm_cases stays below 31 stored entries in a column of B, 600 in a leaf
of A, 1000 in ``nnz(A) // ncol(A)``, 1000 in magnitude of an integer and 3 P + 50 rows.

THE SELECTION RULES the cases are named for, each read off the code and asserted from the shape, never observed:

  metadata batches    the wavefront of an item fetches the pairs (j, b, run bounds) of its column of B 64 at a time
                      (``for (c0 = bb; c0 < be; c0 += 64)``) and hands them round in groups of SPGEMM_U = 4; a batch
                      holds ``np = min(64, be - c0)`` pairs, and the lanes past ``np`` hold ``len == 0``.
  run lengths         a run is the part of a leaf of A inside one panel of P rows; its first 64 elements are fetched
                      ahead, the rest go through ``for (x = 64; x < plen; x += 64)``.
  split               ``rowpanel_split(ncol, nnz)``: 1 when ``nnz // ncol < 2048``; else the sp of 1, 2, 4 with the
                      smallest ``rounds / sp``, ``rounds = ceil(ceil(ncol * sp / 16) / 512)``, the first on a tie:
                      4 for ncol <= 2048, 2 for 2048 < ncol <= 4096.  Segment sg of a leaf is
                      ``[beg + len * sg // sp, beg + len * (sg + 1) // sp)`` and starts from the panel of the element
                      before it; only the last segment writes the bounds past the leaf's end.
  value scan          inside the table kernel a workgroup of NT = 1024 lanes looks at the values of a leaf
                      4 * NT = 4096 per trip: position 4096 of a leaf is the first of the second trip.
  LDS table form      taken while ``(npan + 1) * 16 * 4 <= 64 KiB``, npan <= 1023, i.e. nrow <= 1023 * P.  Past it
                      ``launch_rowpanel_table_scan`` returns false: the plain table kernel runs with a workgroup per
                      leaf when ``(nnz // ncol >= 1024 and ncol > 1) or ncol == 1``, else a wavefront per leaf, and
                      ``spgemm_scan_values`` looks at A's values in a pass of its own.
  integer operands    ``(double) a * (double) b``, rounded, then added in ascending j: values near 2^31 tell it from a
                      product formed in int32 and from a sum kept in int64.

THE EXPECTATION is ``expect_csc``: the rule of spgemm_cases.expect stated on CSC triples, with one float64 and one bool
vector of nrow reused for every nonempty column of B.  Neither the dense operand nor the dense result is formed: the
tall operands (``SparseOp``) exist as CSC only.

Everything but the names is built on first use, per panel height P (``case(P, name)``).
"""
from __future__ import annotations

import functools

import numpy as np

import arith_cases as ac
from sparsearray_amd import NA_integer, NA_real
from spgemm_cases import Op, _vals

INT_MAX = 2 ** 31 - 1
SPLIT_AT = 2048             # rowpanel_split: leaves are split from nnz // ncol >= 2048
SCAN_TRIP = 4096            # values of a leaf the table kernel's scan looks at per trip
WIDE_AT = 1024              # plain table kernel: a workgroup per leaf from nnz // ncol >= 1024
LDS_PANELS = 1023           # the LDS table form ends past 1023 panels


# ---------------------------------------------------------------------------
# operands that exist as CSC only, and the expectation on CSC triples
# ---------------------------------------------------------------------------
class SparseOp:
    """a 2-D operand as (col_ptr int64, row_idx int32, val float64 | int32), read-only; rows ascend inside a leaf"""

    def __init__(self, shape, col_ptr, row_idx, val):
        self.shape = (int(shape[0]), int(shape[1]))
        cp, ri = np.ascontiguousarray(col_ptr, np.int64), np.ascontiguousarray(row_idx, np.int32)
        val = np.ascontiguousarray(val)
        assert val.dtype in (np.float64, np.int32) and cp.size == self.shape[1] + 1
        assert cp[0] == 0 and cp[-1] == ri.size == val.size and np.all(np.diff(cp) >= 0)
        if ri.size:
            assert ri.min() >= 0 and ri.max() < self.shape[0]
            inner = np.ones(ri.size, bool)
            inner[cp[:-1][cp[:-1] < ri.size]] = False                    # the first entry of every leaf
            assert np.all(np.diff(ri.astype(np.int64))[inner[1:]] > 0), "rows do not ascend inside a leaf"
        for a in (cp, ri, val):
            a.setflags(write=False)
        self.csc = (cp, ri, val)

    @classmethod
    def of_leaves(cls, nrow, leaves, vals):
        """``leaves``: one array of rows per leaf; ``vals``: the values in CSC order"""
        leaves = [np.unique(np.asarray(l, np.int64)) for l in leaves]
        cp = np.zeros(len(leaves) + 1, np.int64)
        np.cumsum([l.size for l in leaves], out=cp[1:])
        ri = np.concatenate(leaves) if leaves else np.zeros(0, np.int64)
        return cls((nrow, len(leaves)), cp, ri, vals)

    @property
    def type(self):
        return "double" if self.csc[2].dtype == np.float64 else "integer"

    @property
    def nnz(self):
        return int(self.csc[1].size)

    def with_val(self, val):
        return SparseOp(self.shape, self.csc[0], self.csc[1], val)


def sparse(op) -> SparseOp:
    """an Op or a SparseOp as a SparseOp"""
    return op if isinstance(op, SparseOp) else SparseOp(op.shape, *op.csc)


def expect_csc(shapeA, cscA, shapeB, cscB):
    """THE RULE of spgemm_cases.expect on CSC triples: for every nonempty column k of B, for j ascending over its stored
    entries, ``acc[rows of A[:, j]] += A[rows, j] * b`` into one float64 vector of nrow starting from +0.0 (an integer
    value goes over as.double()), ``reached[rows] = True``; kept where ``reached & ((acc != 0) | isnan(acc))``.  The
    two vectors are put back to zero at the touched rows and reused.  Returns ((col_ptr, row_idx, val), the class of
    every kept entry (EXACT, or ANY_NAN where the value is a NaN), not_finite)."""
    (m, n), (n2, K) = shapeA, shapeB
    assert n == n2
    acp, ari, av = cscA
    bcp, bri, bv = cscB
    avd, bvd = ac.as_double(np.asarray(av)), ac.as_double(np.asarray(bv))
    acc, reached = np.zeros(m), np.zeros(m, bool)
    cp, ris, vals = np.zeros(K + 1, np.int64), [], []
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(np.diff(bcp) > 0):
            js = bri[bcp[k]:bcp[k + 1]]
            assert np.all(np.diff(js.astype(np.int64)) > 0)             # ascending j
            for t in range(int(bcp[k]), int(bcp[k + 1])):
                lo, hi = int(acp[bri[t]]), int(acp[bri[t] + 1])
                rows = ari[lo:hi]
                acc[rows] += avd[lo:hi] * bvd[t]
                reached[rows] = True
            rows = np.flatnonzero(reached)
            a = acc[rows]
            keep = (a != 0) | np.isnan(a)
            ris.append(rows[keep])
            vals.append(a[keep])
            cp[k + 1] = int(keep.sum())
            acc[rows], reached[rows] = 0.0, False
    np.cumsum(cp, out=cp)
    ri = np.concatenate(ris).astype(np.int32) if ris else np.zeros(0, np.int32)
    vv = np.concatenate(vals) if vals else np.zeros(0)
    cls = np.where(np.isnan(vv), ac.ANY_NAN, ac.EXACT).astype(np.int8)
    not_finite = bool((~np.isfinite(avd)).any() or (~np.isfinite(bvd)).any())
    return (cp, ri, vv), cls, not_finite


class ExpectedCSC:
    """what spgemm_cases.expected_mask_check reads of an expectation: ``csc``, ``csc_cls``, ``not_finite``"""

    def __init__(self, A, B):
        self.shape = (A.shape[0], B.shape[1])
        self.csc, self.csc_cls, self.not_finite = expect_csc(A.shape, A.csc, B.shape, B.csc)

    def column(self, k):
        """(rows, values) of result column k"""
        cp, ri, vv = self.csc
        return ri[cp[k]:cp[k + 1]], vv[cp[k]:cp[k + 1]]

    def cell(self, i, k):
        """the stored value of cell (i, k), or None"""
        rows, vals = self.column(k)
        at = np.searchsorted(rows, i)
        return float(vals[at]) if at < rows.size and rows[at] == i else None


class Case:
    def __init__(self, A, B, note=""):
        self.A, self.B, self.note = A, B, note

    @functools.cached_property
    def want(self):
        return ExpectedCSC(self.A, self.B)


def leaf(op, j):
    """(first position in CSC order, rows) of leaf j"""
    cp, ri, _ = op.csc
    return int(cp[j]), ri[cp[j]:cp[j + 1]]


def runs(op, j, P):
    """the lengths of the runs of leaf j: its entries per panel of P rows, the nonempty panels only"""
    n = np.bincount(leaf(op, j)[1] >> int(P).bit_length() - 1)
    return n[n > 0].tolist()


def referred(B):
    """the leaves of A an entry of B refers to"""
    return np.unique(B.csc[1])


# ---------------------------------------------------------------------------
# 1. metadata batches: columns of B with more than 64 entries
# ---------------------------------------------------------------------------
B_COLUMN_N = (63, 64, 65, 66, 67, 68, 127, 128, 129, 200)
B_COLUMN_INT = (67, 200)                        # B integer
B_COLUMN_NA = ((65, 64), (129, 128), (200, 64))  # (n, position in column 0 of an NA_integer_)


def _b_column(P, n, b_type="double", na_at=None):
    rng = np.random.default_rng(3000 + n)
    stored = rng.random((P + 9, n)) < 0.03
    stored[[P - 1, P], :] = True                 # every pair meets on either side of the panel edge
    dense = np.zeros((P + 9, n))
    dense[stored] = _vals(int(stored.sum()), 3100 + n)
    marks = sorted({j for j in (0, 63, 64, n - 1) if 0 <= j < n})
    rows = np.concatenate([np.arange(n), marks])
    cols = np.concatenate([np.zeros(n, int), np.full(len(marks), 2)])
    vals = _vals(rows.size, 3200 + n, b_type)
    if na_at is not None:
        vals[na_at] = NA_integer
    return Case(Op(dense, stored), Op.of(n, 3, rows, cols, vals, ac.sc.NP_DTYPE[b_type]))


# ---------------------------------------------------------------------------
# 2. the order of j across a batch edge and across a U-group edge
# ---------------------------------------------------------------------------
ORDER_ZERO, ORDER_ONE = (1e16, 1.0, -1e16), (1e16, -1e16, 1.0)     # in ascending order: 0.0 (not stored) and 1.0
# (row, the three j, the pattern).  Rows 11 .. 14 hold all three j inside ONE U-group: exchanging the first two terms
# of a sum changes nothing (a + b == b + a), so a group visited backwards shows only where it holds all three.
ORDER_ROWS = lambda P: (            # noqa: E731
    (5, (10, 70, 130), ORDER_ZERO), (6, (10, 70, 130), ORDER_ONE), (P, (10, 70, 130), ORDER_ZERO),
    (7, (2, 3, 4), ORDER_ZERO), (8, (2, 3, 4), ORDER_ONE), (9, (62, 63, 64), ORDER_ZERO), (10, (62, 63, 64), ORDER_ONE),
    (11, (4, 5, 6), ORDER_ZERO), (12, (4, 5, 6), ORDER_ONE), (13, (64, 65, 66), ORDER_ZERO), (14, (64, 65, 66), ORDER_ONE))


def _order_across_batches(P):
    rows, cols, vals = [], [], []
    for r, js, pattern in ORDER_ROWS(P):
        rows += [r] * 3
        cols += list(js)
        vals += list(pattern)
    A = Op.of(P + 5, 200, rows, cols, vals)
    return Case(A, Op.of(200, 1, np.arange(200), np.zeros(200, int), np.ones(200)))


# ---------------------------------------------------------------------------
# 3. run lengths at the lane count
# ---------------------------------------------------------------------------
RUN_N = (63, 64, 65, 128, 129)


def _run(P, n):
    first = P - n // 2
    rows = np.concatenate([np.arange(P - n, P), np.arange(P, P + n), np.arange(first, first + n)])
    A = Op.of(2 * P + 3, 3, rows, np.repeat([0, 1, 2], n), _vals(3 * n, 3300 + n))
    return Case(A, Op.of(3, 2, [0, 1, 2, 0, 1, 2], [0, 0, 0, 1, 1, 1], _vals(6, 3400 + n)))


# ---------------------------------------------------------------------------
# 4. the split forms of the table pass, and the second trip of its value scan
# ---------------------------------------------------------------------------
def _random_leaves(nrow, densities, seed, bands=None):
    """stored mask: leaf j at density densities[j], inside rows bands[j] = (lo, hi) where given"""
    rng = np.random.default_rng(seed)
    stored = np.zeros((nrow, len(densities)), bool)
    for j, d in enumerate(densities):
        lo, hi = (bands or {}).get(j, (0, nrow))
        stored[lo:hi, j] = rng.random(hi - lo) < d
    return stored


def _filled(stored, seed, type="double"):
    dense = np.zeros(stored.shape, ac.sc.NP_DTYPE[type])
    dense[stored] = _vals(int(stored.sum()), seed, type)
    return Op(dense, stored)


def _split4(P):
    A = _filled(_random_leaves(3 * P, [0.75] * 6, 3500), 3501)
    # leaf 2 is referred to by no entry of B
    return Case(A, Op.of(6, 4, [0, 1, 3, 4, 5, 0, 5, 1, 3, 4], [0, 0, 0, 0, 0, 2, 2, 3, 3, 3], _vals(10, 3502)))


def _split4_ragged(P):
    """leaf 1 empty; leaf 2 three entries, one on either side of a panel edge (segments of 0, 1, 1, 1 entries: a
    segment's carry is the panel of the entry before it); leaf 3 in the last panel only, leaf 4 in the first only; a
    seventh leaf of ONE entry, so that three of its four segments are empty; leaves 0 and 5 dense enough to keep the
    mean at 2048"""
    stored = _random_leaves(3 * P, [0.95, 0.0, 0.0, 0.9, 0.9, 0.95, 0.0], 3510, bands={3: (2 * P, 3 * P), 4: (0, P)})
    stored[[P - 1, P, 3 * P - 1], 2] = True
    stored[P, 6] = True
    rows = list(range(7)) + [1, 2, 3, 6] + [2, 4, 5, 6]
    return Case(_filled(stored, 3511), Op.of(7, 4, rows, [0] * 7 + [2] * 4 + [3] * 4, _vals(15, 3512)))


SPLIT2_NCOL = 2050


def _split2(P):
    A = _filled(_random_leaves(2 * P + 3, [0.55] * SPLIT2_NCOL, 3520), 3521)
    rng = np.random.default_rng(3522)
    rows, cols = [], []
    for k in range(3):
        js = set(rng.choice(SPLIT2_NCOL - 10, size=70, replace=False).tolist())     # (the last ten: see below)
        if k == 2:
            js |= {0, SPLIT2_NCOL - 1}           # the first and the last leaf of A
        rows += sorted(js)
        cols += [k] * len(js)
    # leaves ncol - 10 .. ncol - 2 are referred to by no entry of B
    return Case(A, Op.of(SPLIT2_NCOL, 3, rows, cols, _vals(len(rows), 3523)))


LONG_LEAF = 3


def _long_leaf_unsplit(P):
    stored = _random_leaves(3 * P, [10.0 / (3 * P)] * 8, 3530)
    stored[:, LONG_LEAF] = np.random.default_rng(3531).random(3 * P) < 0.8
    for j in range(8):
        stored[[j, P + j], j] = True             # no leaf is empty
    # leaves 2, 5 and 6 are referred to by no entry of B
    return Case(_filled(stored, 3532), Op.of(8, 3, [0, 3, 7, 1, 3, 4, 7], [0, 0, 0, 2, 2, 2, 2], _vals(7, 3533)))


FLAG_FORMS = ("split4", "split2", "long_leaf_unsplit")
SPECIALS = {"double": (("Inf", np.inf), ("NaN", np.nan), ("NA_real", NA_real)), "integer": (("NA_integer", NA_integer),)}


def flag_places(case):
    """where one special value goes, as (what, leaf, position inside the leaf): in a long leaf that B refers to at
    positions 0, 4095, 4096 (the last of the scan's first trip and the first of its second, where the leaf is that
    long), at the two sides of the middle (the edge of a segment of a leaf split in two or four) and at the last
    position; in the last leaf of A; in a leaf no entry of B refers to (at position 4096 or its last)"""
    A, B = case.A, case.B
    lens = np.diff(A.csc[0])
    ref = referred(B)
    long_leaf = int(ref[np.argmax(lens[ref])])
    n = int(lens[long_leaf])
    at = sorted({p for p in (0, SCAN_TRIP - 1, SCAN_TRIP, n // 2 - 1, n // 2, n - 1) if 0 <= p < n})
    places = [(f"long leaf, position {p}", long_leaf, p) for p in at]
    last = A.shape[1] - 1
    places.append(("the last leaf of A, its last position", last, int(lens[last]) - 1))
    unref = np.setdiff1d(np.arange(A.shape[1]), ref)
    j = int(unref[np.argmax(lens[unref])])
    places.append(("a leaf nobody refers to", j, min(SCAN_TRIP, int(lens[j]) - 1)))
    return places


def with_special(A, j, pos, value):
    """A as a SparseOp with ``value`` at position ``pos`` of leaf j; also the index of that value in CSC order"""
    A = sparse(A)
    at = int(A.csc[0][j]) + pos
    assert A.csc[0][j] <= at < A.csc[0][j + 1]
    val = A.csc[2].copy()
    val[at] = value
    return A.with_val(val), at


def as_integer(A, seed):
    """the same stored entries with integer values"""
    A = sparse(A)
    return A.with_val(_vals(A.nnz, seed, "integer"))


# ---------------------------------------------------------------------------
# 5. very tall A: CSC only
# ---------------------------------------------------------------------------
TALL = ("tall_last_lds", "tall_narrow", "tall_wide", "tall_wide_empty_leaf", "tall_one_leaf")


def tall_marks(P, nrow):
    return [0, P - 1, P, LDS_PANELS * P - 1, nrow - 1]


def _tall_rows(P, nrow, n, rng, marked):
    """n rows out of three bands of panels (0 and 1; 500; the last two), plus the marks: long stretches of empty
    panels in between"""
    bands = np.concatenate([np.arange(0, 2 * P), np.arange(500 * P, 501 * P), np.arange((LDS_PANELS - 1) * P, nrow)])
    rows = rng.choice(bands, size=n, replace=False)
    return np.unique(np.concatenate([rows, tall_marks(P, nrow)])) if marked else np.unique(rows)


def _tall(P, nrow, lens, seed):
    """leaf j holds about lens[j] entries (0: empty); the first and the last nonempty leaf hold the marks"""
    rng = np.random.default_rng(seed)
    full = [j for j, n in enumerate(lens) if n > 0]
    leaves = [_tall_rows(P, nrow, n, rng, j in (full[0], full[-1])) if n > 0 else np.zeros(0, np.int64) for j, n in enumerate(lens)]
    A = SparseOp.of_leaves(nrow, leaves, _vals(sum(l.size for l in leaves), seed + 1))
    n = len(lens)
    rows = list(range(n)) + ([n - 1] if n < 3 else [1, n - 1])           # column 0 full, column 1 empty
    cols = [0] * n + [2] * (len(rows) - n)
    return Case(A, sparse(Op.of(n, 3, rows, cols, _vals(len(rows), seed + 2))))


def _tall_case(P, name):
    return {"tall_last_lds": lambda: _tall(P, LDS_PANELS * P, [40, 40, 0, 40, 40], 3600),
            "tall_narrow": lambda: _tall(P, LDS_PANELS * P + 1, [40, 40, 0, 40, 40], 3610),
            "tall_wide": lambda: _tall(P, LDS_PANELS * P + 1, [1500, 1500], 3620),
            "tall_wide_empty_leaf": lambda: _tall(P, LDS_PANELS * P + 1, [2300, 0, 2300], 3630),
            "tall_one_leaf": lambda: _tall(P, LDS_PANELS * P + 1, [300], 3640)}[name]()


def tall_flag_places(case):
    """a special at the first and at the last value of A"""
    A = case.A
    lens = np.diff(A.csc[0])
    full = np.flatnonzero(lens > 0)
    return [("the first value of A", int(full[0]), 0), ("the last value of A", int(full[-1]), int(lens[full[-1]]) - 1)]


def ws_least(P, nrow, ninner, K):
    """the layout of the kernel's header: head 256, the table int32[(npan + 1) * n], counts and bases
    int64[K * npan + 1], each part at a multiple of 256 bytes (the scan's scratch comes on top)"""
    npan = (nrow + P - 1) // P
    up = lambda b: (b + 255) // 256 * 256        # noqa: E731
    return 256 + up((npan + 1) * max(ninner, 1) * 4) + up((K * npan + 1) * 8)


# ---------------------------------------------------------------------------
# 6. integers near 2^31
# ---------------------------------------------------------------------------
LARGE = tuple(s * v for v in (INT_MAX, INT_MAX - 1, 46341, 65536, 1) for s in (1, -1))
LARGE_TYPES = (("integer", "integer"), ("integer", "double"), ("double", "integer"))


def _large_integers(P, ta, tb):
    rng = np.random.default_rng(3700)
    sa = rng.random((P + 9, 12)) < 0.4
    sa[[P - 1, P], :] = True
    a = np.zeros(sa.shape, ac.sc.NP_DTYPE[ta])
    a[sa] = rng.choice(LARGE, size=int(sa.sum()))
    sb = rng.random((12, 4)) < 0.5
    sb[:, 0] = True
    b = np.zeros(sb.shape, ac.sc.NP_DTYPE[tb])
    b[sb] = rng.choice(LARGE, size=int(sb.sum()))
    b[:, 0] = INT_MAX                            # one column of B is all 2^31 - 1
    return Case(Op(a, sa), Op(b, sb))


# ---------------------------------------------------------------------------
# the names (built at import) and the cases (built on first use, per P)
# ---------------------------------------------------------------------------
def _builders():
    b = {}
    for n in B_COLUMN_N:
        b[f"b_column_{n}"] = lambda P, n=n: _b_column(P, n)
    for n in B_COLUMN_INT:
        b[f"b_column_{n}_integer_B"] = lambda P, n=n: _b_column(P, n, "integer")
    for n, at in B_COLUMN_NA:
        b[f"b_column_{n}_NA_integer_at_{at}"] = lambda P, n=n, at=at: _b_column(P, n, "integer", at)
    b["order_across_batches"] = _order_across_batches
    for n in RUN_N:
        b[f"run_{n}"] = lambda P, n=n: _run(P, n)
    b["split4"], b["split4_ragged"], b["split2"], b["long_leaf_unsplit"] = _split4, _split4_ragged, _split2, _long_leaf_unsplit
    for name in TALL:
        b[name] = lambda P, name=name: _tall_case(P, name)
    for ta, tb in LARGE_TYPES:
        b[f"large_integers_{ta}_x_{tb}"] = lambda P, ta=ta, tb=tb: _large_integers(P, ta, tb)
    return b


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
SMALL = [n for n in NAMES if n not in TALL]                                 # built as dense Ops: expect() applies
NA_NAMES = [f"b_column_{n}_NA_integer_at_{at}" for n, at in B_COLUMN_NA]
FINITE_SMALL = [n for n in SMALL if n not in NA_NAMES and n != "order_across_batches"]


@functools.lru_cache(maxsize=None)
def case(P, name):
    return _BUILDERS[name](P)
