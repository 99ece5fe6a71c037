"""Operands and expectations for the sparse x sparse products with a sparse result (include/svt_hip.h, svt_dev_spgemm;
Session.matmul_sparse / crossprod_sparse / tcrossprod_sparse), shared by tests/test_zzzzzzzz_spgemm_cpu.py (the case
builder's own proofs, the Session checks) and tests/test_zzzzzzzz_spgemm_hip.py (the device kernels).

THE EXPECTATION is numpy on dense arrays, stated once in ``expect(A, B)``: for every result column k, for j ascending
over the stored entries of B[:, k], ``acc[rows of A[:, j], k] += A[rows, j] * b`` -- one vectorised statement per pair;
the rows of one leaf are distinct, so every cell gets its products in ascending order of the inner index, each rounded
and then added (numpy fuses nothing), the accumulator starting from +0.0; an integer value goes over as.double()
(NA_integer_ -> NA_real_).  ``reached[rows, k] = True``; a cell is kept where ``reached & ((acc != 0) | isnan(acc))``.

HOW VALUES ARE COMPARED (the classes of tests/arith_cases.py): the stored mask exactly; the values as bits (EXACT),
except where the expected value is a NaN -- a NaN or an NA operand took part, or Inf - Inf / 0 * Inf happened on the
way -- where only "is NaN" is compared (ANY_NAN: which payload and which sign survive an addition of two NaNs is the
hardware's choice).

An operand is a dense array plus the mask of its stored entries (a stored zero is an entry like any other); ``csc``
gives the device layout.  The device cases are built for a panel height P, like ``device_cases(T)`` of arith_cases.
"""
from __future__ import annotations

import functools

import numpy as np

import arith_cases as ac
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray

PANELS = (1024, 2048, 4096)             # the heights the kernel can be built for; the library answers one of them


class Op:
    """a 2-D operand: ``dense`` (float64 or int32, column-major) and ``stored`` (bool), read-only"""

    def __init__(self, dense, stored):
        self.dense, self.stored = np.asfortranarray(dense), np.asfortranarray(stored, dtype=bool)
        assert self.dense.shape == self.stored.shape and self.dense.ndim == 2
        assert self.dense.dtype in (np.float64, np.int32)
        assert not np.any((self.dense != 0) & ~self.stored) and not np.any(_isnan(self.dense) & ~self.stored)
        self.dense.setflags(write=False)
        self.stored.setflags(write=False)

    @classmethod
    def of(cls, nrow, ncol, rows, cols, vals, dtype=np.float64):
        dense, stored = np.zeros((nrow, ncol), dtype, order="F"), np.zeros((nrow, ncol), bool, order="F")
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        assert rows.size == cols.size == np.asarray(vals).size
        assert np.unique(rows + cols * max(nrow, 1)).size == rows.size, "an entry twice"
        dense[rows, cols] = np.asarray(vals, dtype)
        stored[rows, cols] = True
        return cls(dense, stored)

    @classmethod
    def random(cls, nrow, ncol, density, seed, type="double"):
        rng = np.random.default_rng(seed)
        stored = rng.random((nrow, ncol)) < density
        dense = np.zeros((nrow, ncol), ac.sc.NP_DTYPE[type])
        dense[stored] = _vals(int(stored.sum()), seed + 1000, type)
        return cls(dense, stored)

    @property
    def shape(self):
        return self.dense.shape

    @property
    def type(self):
        return "double" if self.dense.dtype == np.float64 else "integer"

    @functools.cached_property
    def csc(self):
        """(col_ptr int64, row_idx int32, val)"""
        nrow, ncol = self.shape
        cp = np.zeros(ncol + 1, np.int64)
        np.cumsum(self.stored.sum(axis=0), out=cp[1:])
        cols, rows = np.nonzero(self.stored.T)
        return cp, rows.astype(np.int32), np.ascontiguousarray(self.dense.T[cols, rows])

    @property
    def nnz(self):
        return int(self.stored.sum())

    def t(self):
        return Op(self.dense.T, self.stored.T)

    def not_finite(self):
        v = ac.as_double(self.dense[self.stored])
        return bool((~np.isfinite(v)).any())

    def svt(self, dimnames=None):
        cp, ri, vv = self.csc
        return SVT_SparseArray.from_csc(self.shape, self.type, cp, ri, vv, dimnames=dimnames)


def _isnan(a):
    return np.isnan(a) if a.dtype == np.float64 else np.zeros(a.shape, bool)


def _vals(n, seed, type="double"):
    """values that do not cancel by accident: three decimals between 1 and 100 in magnitude, both signs (a sum of a
    few products of them is zero only when the products are equal and opposite)"""
    return ac._vals(n, seed, type)


class Expected:
    """dense values, stored mask, comparison classes, the flag"""

    def __init__(self, acc, kept, not_finite):
        self.dense, self.stored = np.asfortranarray(acc), np.asfortranarray(kept)
        self.cls = np.where(np.isnan(self.dense), ac.ANY_NAN, ac.EXACT).astype(np.int8)
        self.not_finite = bool(not_finite)

    @functools.cached_property
    def csc(self):
        return Op(np.where(self.stored, self.dense, 0.0), self.stored).csc

    @property
    def csc_cls(self):
        cols, rows = np.nonzero(self.stored.T)
        return self.cls.T[cols, rows]


def expect(A: Op, B: Op) -> Expected:
    """THE EXPECTATION of the module docstring"""
    (m, n), (n2, K) = A.shape, B.shape
    assert n == n2
    Ad, Bd = ac.as_double(A.dense), ac.as_double(B.dense)
    acc, reached = np.zeros((m, K), order="F"), np.zeros((m, K), bool, order="F")
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(B.stored.any(axis=0)):
            for j in np.flatnonzero(B.stored[:, k]):            # ascending j
                rows = np.flatnonzero(A.stored[:, j])
                acc[rows, k] += Ad[rows, j] * Bd[j, k]
                reached[rows, k] = True
    kept = reached & ((acc != 0) | np.isnan(acc))
    return Expected(acc, kept, A.not_finite() or B.not_finite())


def expected_mask_check(got_csc, want: Expected, what):
    """a CSC triple against the expectation: col_ptr and row_idx exactly, rows ascending inside a column, values by class"""
    wcp, wri, wv = want.csc
    cp, ri, vv = got_csc
    assert np.array_equal(cp, wcp), f"{what}: col_ptr {cp[:8]}, want {wcp[:8]}"
    assert ri.dtype == np.int32 and np.array_equal(ri, wri), f"{what}: row_idx"
    assert vv.dtype == np.float64 and vv.shape == wv.shape, what
    cls = want.csc_cls
    m = cls == ac.EXACT
    gb, wb = ac.sc.bits(vv), ac.sc.bits(wv)
    assert np.array_equal(gb[m], wb[m]), f"{what}: values differ as bits at {np.flatnonzero(m & (gb != wb))[:5].tolist()}"
    assert np.all(np.isnan(vv[~m])), f"{what}: not NaN where a NaN is due"


# ---------------------------------------------------------------------------
# device cases around the panel height P
# ---------------------------------------------------------------------------
class Case:
    def __init__(self, A, B, edges=(), note=""):
        self.A, self.B, self.edges, self.note = A, B, tuple(edges), note

    @functools.cached_property
    def want(self):
        return expect(self.A, self.B)


def straddles(case, P):
    """whether the result has, in one column, a stored cell in the last row of a panel of P rows and one in the first
    row of the next -- on both sides of every edge the case names"""
    kept = case.want.stored
    return all(e % P == 0 and 0 < e < kept.shape[0] and (kept[e - 1] & kept[e]).any() for e in case.edges) and len(case.edges) > 0


def _boundary(P, nrow, seed):
    """A nrow x 7 with random entries and, in the leaves 1 and 4, an entry in every row next to a panel edge, the first
    row and the last; B 7 x 5 with leaves 1 and 4 referred to by every column"""
    rng = np.random.default_rng(seed)
    stored = rng.random((nrow, 7)) < 0.02
    marks = [r for e in range(P, nrow + P, P) for r in (e - 2, e - 1, e, e + 1) if 0 <= r < nrow] + [0, nrow - 1]
    for j in (1, 4):
        stored[marks, j] = True
    dense = np.zeros((nrow, 7))
    dense[stored] = _vals(int(stored.sum()), seed + 1)
    bs = rng.random((7, 5)) < 0.4
    bs[[1, 4], :] = True
    bd = np.zeros((7, 5))
    bd[bs] = _vals(int(bs.sum()), seed + 2)
    return Case(Op(dense, stored), Op(bd, bs), edges=[e for e in range(P, nrow, P)])


def _special_cases(P):
    """NA_integer_, NA_real_, NaN, +Inf, -Inf: in a value a pair reads, and in a leaf of A no entry of B refers to"""
    out = {}
    nan2 = np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0]
    for name, v, type in (("NA_integer", NA_integer, "integer"), ("NA_real", NA_real, "double"), ("NaN", nan2, "double"),
                          ("plus_Inf", np.inf, "double"), ("minus_Inf", -np.inf, "double")):
        for where in ("read_by_a_pair", "in_a_leaf_nobody_refers_to"):
            A = Op.random(P + 9, 6, 0.05, 40 + len(out), type)
            dense, stored = A.dense.copy(), A.stored.copy()
            j = 2 if where == "read_by_a_pair" else 5
            for r in (3, P - 1, P):
                dense[r, j], stored[r, j] = v, True
            dense[P + 1, 2], stored[P + 1, 2] = 7, True
            bs = np.zeros((6, 4), bool)
            bs[[0, 2, 3], 0] = bs[[1, 2], 1] = bs[[2, 4], 3] = True     # leaf 5 of A: no entry of B in row 5
            bd = np.zeros((6, 4))
            bd[bs] = _vals(int(bs.sum()), 77)
            out[f"{name}_{where}"] = Case(Op(dense, stored), Op(bd, bs))
    # the special on B's side: an Inf in B meets A's entries, and an Inf in a row of B whose leaf of A is empty
    A = Op.random(P + 9, 6, 0.05, 60)
    dense, stored = A.dense.copy(), A.stored.copy()
    dense[:, 4], stored[:, 4] = 0.0, False
    for j, tag in ((2, "read_by_a_pair"), (4, "against_an_empty_leaf")):
        bs = np.zeros((6, 3), bool)
        bs[[0, 2, 4], 1] = True
        bd = np.zeros((6, 3))
        bd[bs] = _vals(3, 78)
        bd[j, 1] = np.inf
        out[f"Inf_in_B_{tag}"] = Case(Op(dense, stored), Op(bd, bs))
    return out


RANDOM_SHAPES = 20


@functools.lru_cache(maxsize=None)
def device_cases(P):
    """The cases around the panel height P.  Their extents: at most 30 pairs in a column of B, leaves of A below 600
    entries, ``nnz(A) // ncol(A)`` below 1000, integers below 1000 in magnitude, at most 3 P + 50 rows.  The branches of
    the kernels past those extents (a second batch of 64 pairs, runs of 64 and more, split leaves, the second trip of
    the value scan, operands past 1023 panels, integers near 2^31) are run by the cases of tests/spgemm_branch_cases.py."""
    cases = {}
    for nrow, tag in ((P - 1, "P-1"), (P, "P"), (P + 1, "P+1"), (2 * P + 3, "2P+3")):
        cases[f"nrow_{tag}"] = _boundary(P, nrow, 100 + nrow % 7)
    # one result column that receives everything: K = 1, B's column full
    A = Op.random(2 * P + 3, 30, 0.10, 1)
    cases["one_column_receives_everything"] = Case(A, Op.of(30, 1, np.arange(30), np.zeros(30, int), _vals(30, 2)))
    # runs that end exactly at a panel edge, start exactly at one, and cross one
    rows = np.concatenate([np.arange(P - 5, P), np.arange(P, P + 5), np.arange(P - 2, P + 3), np.arange(2 * P - 3, 2 * P)])
    cols = np.repeat([0, 1, 2, 3], [5, 5, 5, 3])
    A = Op.of(2 * P + 3, 4, rows, cols, _vals(rows.size, 3))
    cases["runs_at_a_panel_edge"] = Case(A, Op.of(4, 3, [0, 1, 2, 3, 0, 2, 1], [0, 0, 0, 0, 1, 1, 2], _vals(7, 4)), edges=[P])
    # 100 003 columns of B of which five hold entries
    A = Op.random(P + 5, 6, 0.05, 5)
    K = 100_003
    bc = np.repeat([0, 5, 50_000, 70_000, K - 1], 2)
    br = np.array([0, 3, 1, 2, 2, 5, 0, 4, 3, 5])
    cases["100000_empty_columns"] = Case(A, Op.of(6, K, br, bc, _vals(10, 6)))
    # empty leaves of A that B refers to
    A = Op.random(P + 5, 8, 0.05, 7)
    dense, stored = A.dense.copy(), A.stored.copy()
    dense[:, [2, 4]], stored[:, [2, 4]] = 0.0, False
    cases["empty_leaves_referred_to"] = Case(Op(dense, stored), Op.of(8, 3, [2, 4, 1, 2, 4, 7, 4], [0, 0, 1, 1, 1, 1, 2], _vals(7, 8)))
    # empty operands and empty extents
    full_A, full_B = Op.random(P + 5, 8, 0.05, 9), Op.random(8, 5, 0.3, 10)
    empty_A, empty_B = Op(np.zeros((P + 5, 8)), np.zeros((P + 5, 8), bool)), Op(np.zeros((8, 5)), np.zeros((8, 5), bool))
    cases["empty_A"] = Case(empty_A, full_B)
    cases["empty_B"] = Case(full_A, empty_B)
    cases["empty_both"] = Case(empty_A, empty_B)
    cases["K_0"] = Case(full_A, Op(np.zeros((8, 0)), np.zeros((8, 0), bool)))
    cases["n_0"] = Case(Op(np.zeros((P + 5, 0)), np.zeros((P + 5, 0), bool)), Op(np.zeros((0, 4)), np.zeros((0, 4), bool)))
    cases["nrow_0"] = Case(Op(np.zeros((0, 8)), np.zeros((0, 8), bool)), full_B)
    # THE ORDER MATTERS: row 5 gets 1e16, 1.0, -1e16 at ascending j (0.0: not stored), row 6 gets 1e16, -1e16, 1.0 (1.0)
    A = Op.of(P + 5, 3, [5, 5, 5, 6, 6, 6, P, P, P], [0, 1, 2] * 3, [1e16, 1.0, -1e16, 1e16, -1e16, 1.0, 1.0, 1e16, -1e16])
    c = Case(A, Op.of(3, 1, [0, 1, 2], [0, 0, 0], [1.0, 1.0, 1.0]))
    assert c.want.dense[5, 0] == 0.0 and not c.want.stored[5, 0] and c.want.dense[6, 0] == 1.0 and c.want.stored[6, 0]
    assert c.want.dense[P, 0] == 0.0            # (1.0 + 1e16) - 1e16: the order again, across the panel edge
    cases["order_matters"] = c
    # a tile in which every reached cell cancels: equal and opposite products
    rows = np.sort(np.random.default_rng(11).choice(2 * P, size=300, replace=False))
    v = _vals(300, 12)
    A = Op.of(2 * P + 3, 2, np.concatenate([rows, rows]), np.repeat([0, 1], 300), np.concatenate([v, v]))
    cases["every_cell_cancels"] = Case(A, Op.of(2, 1, [0, 1], [0, 0], [2.5, -2.5]))
    # stored zeros in A and in B: reached, the sum is 0, nothing stored; next to cells that are stored
    A = Op.of(P + 5, 3, [1, 2, 3, P - 1, P, 2, 3], [0, 0, 0, 0, 0, 1, 2], [0.0, 4.0, 5.0, 0.0, 6.0, 0.0, 7.0])
    cases["stored_zeros"] = Case(A, Op.of(3, 2, [0, 1, 0, 2], [0, 0, 1, 1], [3.0, 9.0, 0.0, 0.0]))
    # products that are -0.0, a subnormal product, a product that underflows to zero
    A = Op.of(P + 5, 2, [0, 1, 2, P, 0, 1], [0, 0, 0, 0, 1, 1], [-3.0, 1e-200, 1e-200, -0.0, 0.0, 2.0])
    cases["minus_zero_and_subnormal"] = Case(A, Op.of(2, 3, [0, 0, 0, 1], [0, 1, 2, 2], [0.0, 1e-120, 1e-200, -0.0]))
    # integer operands: integer-valued results below 2^53
    for ta, tb in (("integer", "integer"), ("integer", "double"), ("double", "integer")):
        A, B = Op.random(P + 70, 12, 0.1, 13, ta), Op.random(12, 9, 0.3, 14, tb)
        if ta == "double":
            A = Op(np.trunc(A.dense), A.stored)
        if tb == "double":
            B = Op(np.trunc(B.dense), B.stored)
        cases[f"{ta}_x_{tb}"] = Case(A, B)
    cases.update(_special_cases(P))
    # a seeded random family
    rng = np.random.default_rng(2024)
    for s in range(RANDOM_SHAPES):
        m, n, K = int(rng.integers(1, 3 * P + 50)), int(rng.integers(1, 51)), int(rng.integers(1, 41))
        da, db = (float(np.exp(rng.uniform(np.log(0.001), np.log(0.3)))) for _ in range(2))
        ta, tb = (("double", "integer")[int(rng.integers(0, 4) == 0)] for _ in range(2))
        cases[f"random_{s:02d}"] = Case(Op.random(m, n, da, 500 + s, ta), Op.random(n, K, db, 600 + s, tb))
    return cases


DEVICE_NAMES = list(device_cases(2048))
INTEGER_VALUED = ("integer_x_integer", "integer_x_double", "double_x_integer")
BOUNDARY = ("nrow_P+1", "nrow_2P+3", "runs_at_a_panel_edge")


# ---------------------------------------------------------------------------
# host level: small named operands
# ---------------------------------------------------------------------------
def names(prefix, n):
    return [f"{prefix}{i}" for i in range(n)]


@functools.lru_cache(maxsize=None)
def host_operand(name):
    return {
        "x": lambda: Op.random(41, 29, 0.3, 21),
        "y": lambda: Op.random(29, 17, 0.2, 22),                # x %*% y
        "y_int": lambda: Op.random(29, 17, 0.2, 23, "integer"),
        "z": lambda: Op.random(41, 13, 0.3, 24),                # crossprod(x, z)
        "w": lambda: Op.random(23, 29, 0.3, 25, "integer"),     # tcrossprod(x, w)
    }[name]()
