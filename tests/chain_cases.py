"""Chains: operands MADE ON THE DEVICE (by subset, Arith / Math, t() and aperm()) as inputs of every consumer.  Shared by
tests/test_chain_cases_cpu.py (walks every chain with the dense rules alone and asserts what the chains claim) and
tests/test_hip_chains.py (runs them on the GPU).

A chain is data: INPUTS (named host operands), STEPS (producers, each ``(result, kind, source, *arguments)``) and
CONSUMERS (``(operand, consumer)`` pairs).  Every link is checked on its own: the expectation of a step is its dense
rule applied to the ACTUAL arrays of its source(s), so that a 1-ulp log1p leaves the next link's expectation certain.

The dense rules (nothing here walks leaves or tiles):
  Arith merge / scalar / unary minus / Math   arith_cases.expect_* and arith_cases.compare (bits, the NaN classes; ulps
                                              for log1p, expm1 and ^ with the caller's measured bound)
  subset                                      np.ix_ on (dense, stored), values and the stored mask as bits
  t(), aperm()                                numpy transposition of (dense, stored), as bits
  colstats sum / mean / var1, rowsums         exact_stats cells and its rounding bounds
  colstats min / max / countNAs               exact_stats, identical
  colmedians / colquantiles / colmads         the dense rules of test_medians / test_quantiles_cpu / test_mads_cpu, tol 0
  colranks                                    test_ranks_cpu.dense_colranks on the expanded compact form, tol 0
  crossprod(z, Y)                             exact_products.exact_sparse_dense and its bound
"""
from __future__ import annotations

import functools

import numpy as np

import arith_cases as ac
import exact_products as ep
import exact_stats as ex
import stats_cases as stc
import subset_cases as sc
from helpers import assert_equal
from sparsearray_amd import NA_integer, SVT_SparseArray
from test_mads_cpu import dense_colmads
from test_medians import dense_colmedians
from test_quantiles_cpu import dense_colquantiles
from test_hip_ranks import expand as expand_ranks        # (the dense ranks of the compact form; needs no GPU)
from test_ranks_cpu import TIES, dense_colranks

DIM = (600, 160)
PROBS = (0, 0.25, 0.5, 1)
K_DENSE = 8
INT_MAX = ac.INT_MAX


# ---------------------------------------------------------------------------
# a host operand: the CSC arrays, as uploaded or as downloaded
# ---------------------------------------------------------------------------
class Mat:
    def __init__(self, nrow, type, col_ptr, row_idx, val):
        self.nrow, self.type = int(nrow), type
        self.col_ptr = np.ascontiguousarray(col_ptr, dtype=np.int64)
        self.row_idx = np.ascontiguousarray(row_idx, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=sc.NP_DTYPE[type])
        self.ncol, self.nnz = self.col_ptr.size - 1, self.row_idx.size

    def svt(self):
        return SVT_SparseArray.from_csc((self.nrow, self.ncol), self.type, self.col_ptr, self.row_idx, self.val)

    @functools.cached_property
    def dense(self):
        """(dense values, mask of the stored entries), nrow x ncol in Fortran order"""
        d = np.zeros((self.nrow, self.ncol), dtype=self.val.dtype, order="F")
        s = np.zeros((self.nrow, self.ncol), dtype=bool, order="F")
        col = np.repeat(np.arange(self.ncol), np.diff(self.col_ptr))
        d[self.row_idx, col] = self.val
        s[self.row_idx, col] = True
        return d, s

    @functools.cached_property
    def as_float(self):
        """the dense values as doubles, NaN for the NA of an integer or logical operand"""
        d = self.dense[0]
        f = d.astype(np.float64)
        if self.type != "double":
            f[d == NA_integer] = np.nan
        return f


def mat_from_dense(dense, stored, type):
    c, r = np.nonzero(np.asarray(stored).T)
    cp = np.zeros(stored.shape[1] + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=stored.shape[1]), out=cp[1:])
    return Mat(stored.shape[0], type, cp, r, np.asarray(dense)[r, c])


def mat_from_svt(x):
    cp, ri, val = x.to_csc()
    return Mat(x.dim[0], x.type, cp, ri, val)


def check_invariants(m: Mat, nrow, ncol, type, what):
    """what every downloaded intermediate must be, whatever made it"""
    assert (m.nrow, m.ncol, m.type) == (nrow, ncol, type), f"{what}: {m.nrow} x {m.ncol} {m.type}, want {nrow} x {ncol} {type}"
    check_structure(m, what)


def check_structure(m: Mat, what):
    """the part of the invariants that needs no expectation: without it the arrays are no operand at all"""
    type = m.type
    cp = m.col_ptr
    assert cp[0] == 0 and np.all(np.diff(cp) >= 0), f"{what}: col_ptr does not start at 0 or decreases"
    assert cp[-1] == m.nnz == m.row_idx.size == m.val.size, f"{what}: col_ptr[ncol], nnz and the array lengths differ"
    assert m.val.dtype == sc.NP_DTYPE[type], f"{what}: dtype {m.val.dtype}"
    if m.nnz:
        assert m.row_idx.min() >= 0 and m.row_idx.max() < m.nrow, f"{what}: a row outside [0, nrow)"
        starts = np.zeros(m.nnz, bool)
        starts[cp[:-1][np.diff(cp) > 0]] = True
        assert np.all((np.diff(m.row_idx) > 0) | starts[1:]), f"{what}: rows do not ascend inside a column"


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _mask(seed, empty_mod, full_col=None, dim=DIM, density=0.1):
    m = np.random.default_rng(seed).random(dim) < density
    m &= (np.arange(dim[1]) % empty_mod[0] != empty_mod[1])[None, :]
    if full_col is not None:
        m[:, full_col] = True
    return m


def _with_values(mask, type, values):
    """the entries of ``mask`` stored, ``values(k)`` -> the values of the k stored entries in column-major order"""
    base = mat_from_dense(np.zeros(mask.shape), mask, "double")
    return Mat(mask.shape[0], type, base.col_ptr, base.row_idx, values(base.nnz))


def _specials_mix(n, seed):
    """tracer-like doubles with about 10 % of them drawn from SPECIALS_F64"""
    rng = np.random.default_rng(seed)
    v = np.arange(1, n + 1, dtype=np.float64) * rng.choice([-0.5, 0.25, 1.0], size=n)
    at = rng.random(n) < 0.1
    v[at] = sc.SPECIALS_F64[rng.integers(0, len(sc.SPECIALS_F64), size=int(at.sum()))]
    return v


def _int_mix(n, seed):
    """small and mid-sized integers of both signs, NA_integer, and values at and near INT_MAX"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-40000, 40001, size=n).astype(np.int32)
    v[v == 0] = 7
    at = rng.random(n) < 0.08
    v[at] = rng.choice(np.array([NA_integer, INT_MAX, INT_MAX - 1, -INT_MAX, 65536, 46341, 32767, 32768], dtype=np.int32),
                       size=int(at.sum()))
    return v


def _logical_mix(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([1, 1, 1, 0, NA_integer], dtype=np.int32), size=n)


_INPUTS = {
    # 600 x 160, density about 0.1: more than 2 subset tiles, more than 4 Arith tiles; column 80 full, every 7th empty
    "x": lambda: mat_from_svt(sc.operand("wide")[0]),
    # another pattern (every 5th column empty, column 17 full), values that are no tracer of x's
    "m": lambda: _with_values(_mask(41, (5, 2), 17, density=0.13), "double", lambda n: np.arange(1, n + 1) * 0.5 + 0.25),
    "xs": lambda: _with_values(_mask(42, (7, 3), 80), "double", lambda n: _specials_mix(n, 43)),
    "i": lambda: _with_values(_mask(44, (7, 5), 80), "integer", lambda n: _int_mix(n, 45)),
    "lg": lambda: _with_values(_mask(46, (9, 4), 11), "logical", lambda n: _logical_mix(n, 47)),
    # the 3-d operands of arith_cases, 9 x 5 x 4 read as 9 x 20 leaves; and one that is 9 x 4 x 5
    "a3": lambda: mat_from_svt(ac.operand("d3d")),
    "b3": lambda: _with_values(np.random.default_rng(48).random((9, 20)) < 0.4, "double", lambda n: -np.arange(1.0, n + 1)),
}


@functools.lru_cache(maxsize=None)
def operand(name):
    m = _INPUTS[name]()
    for a in (m.col_ptr, m.row_idx, m.val):
        a.setflags(write=False)
    return m


def _incr(n, keep, seed):
    return np.flatnonzero(np.random.default_rng(seed).random(n) < keep).astype(np.int32)


def _perm_rep(n, length, seed):
    """a permutation of 0 .. n-1 repeated up to ``length`` entries"""
    p = np.random.default_rng(seed).permutation(n)
    return np.resize(p, length).astype(np.int32)


def _cols_with_repeats(seed, ncol=DIM[1], length=400, must=(80, 80, 3, 3, 3)):
    return np.concatenate([np.asarray(must), _perm_rep(ncol, length - len(must), seed)]).astype(np.int32)


# what chain 4 adds to its subset: an operand of the subset's extents (420 rows kept by seed 61: see the CPU twin)
ROWS4 = _incr(DIM[0], 0.7, 61)
COLS4 = _cols_with_repeats(62, length=200)

# ---------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------
ORDER = [(f, na_rm) for f in ("colmedians", "colquantiles", "colmads") for na_rm in (False, True)]
RANKS = [("colranks", t) for t in TIES]
STATS = [("colstats", op) for op in ("sum", "mean", "var1", "min", "max", "countNAs")]
FULL = STATS + [("rowsums",)] + ORDER + RANKS + [("crossprod",)]
NOT_FINITE = STATS + [("rowsums",)] + ORDER + RANKS                      # (the exact product is stated for finite values)


def crossprod_Y(nrow):
    """the dense operand of crossprod(z, Y): nrow x 8 small integers"""
    return np.random.default_rng(nrow + 5).integers(-3, 4, size=(nrow, K_DENSE)).astype(np.float64)


def check_consumer(cons, m: Mat, got, what):
    """``got``: what the consumer returned for the operand whose actual arrays are ``m`` (numpy, the device level's
    layout); asserts its rule"""
    kind = cons[0]
    what = f"{what}: {cons}"
    if kind == "colstats":
        op, inner = cons[1], (cons[2] if len(cons) > 2 else 1)
        cells = ex.column_cells(m.col_ptr, m.val, m.nrow, inner=inner)
        assert np.asarray(got).size == cells.ncell, what
        stc.check_stat(op, got, cells, None, None, is_int=m.type != "double", what=what)
    elif kind == "rowsums":
        assert np.asarray(got).size == m.nrow, what
        stc.check_stat("sum", got, ex.row_cells(m.col_ptr, m.row_idx, m.val, m.nrow), None, None, what=what)
    elif kind == "colmedians":
        assert_equal(got, dense_colmedians(m.as_float, cons[1]), tol=0, strict_na=True, what=what)
    elif kind == "colquantiles":
        got = np.asarray(got)
        assert got.shape == (len(PROBS), m.ncol), what
        assert_equal(got.T, dense_colquantiles(m.as_float, PROBS, cons[1]), tol=0, strict_na=True, what=what)
    elif kind == "colmads":
        assert_equal(got, dense_colmads(m.as_float, None, 1.4826, cons[1]), tol=0, strict_na=True, what=what)
    elif kind == "colranks":
        rank_nz, zero_rank = got
        dtype = np.float64 if cons[1] == "average" else np.int32
        assert rank_nz.dtype == dtype and zero_rank.dtype == dtype and rank_nz.size == m.nnz and zero_rank.size == m.ncol, what
        assert_equal(expand_ranks(m.nrow, m.col_ptr, m.row_idx, rank_nz, zero_rank), dense_colranks(m.as_float, cons[1]), tol=0, strict_na=True, what=what)
    elif kind == "crossprod":
        p = ep.exact_sparse_dense(m.col_ptr, m.row_idx, m.val, crossprod_Y(m.nrow))
        ep.check_product(np.asarray(got).T, p, what).require()
    else:
        raise KeyError(kind)


def host_consumer(cons, m: Mat):
    """the consumer's answer by plain numpy in double precision where that is a few lines (sum, mean, var1, rowsums,
    crossprod: held to the same bounds by the CPU twin), else by the dense rule itself"""
    kind = cons[0]
    f = m.as_float
    with np.errstate(all="ignore"):
        if kind == "colstats":
            op, inner = cons[1], (cons[2] if len(cons) > 2 else 1)
            g = f.reshape(m.nrow * inner, m.ncol // inner, order="F")
            cells = ex.column_cells(m.col_ptr, m.val, m.nrow, inner=inner)
            if op in ("sum", "mean"):
                return g.sum(axis=0) if op == "sum" else (g.mean(axis=0) if g.shape[0] else np.full(g.shape[1], np.nan))
            if op == "var1":
                return g.var(axis=0, ddof=1) if g.shape[0] > 1 else np.full(g.shape[1], np.nan)
            if op in ("min", "max"):
                return ex.exact_minmax(cells, op == "min", as_int=m.type != "double")
            return ex.exact_count_nas(cells)
        if kind == "rowsums":
            return f.sum(axis=1)
        if kind == "colmedians":
            return dense_colmedians(f, cons[1])
        if kind == "colquantiles":
            return dense_colquantiles(f, PROBS, cons[1]).T
        if kind == "colmads":
            return dense_colmads(f, None, 1.4826, cons[1])
        if kind == "colranks":
            r = dense_colranks(f, cons[1])
            # the compact form of the dense ranks: a rank per stored value, and per column the rank of an implicit
            # zero (NA where the column has none)
            col = np.repeat(np.arange(m.ncol), np.diff(m.col_ptr))
            zero = np.empty(m.ncol, dtype=r.dtype)
            na = dense_colranks(np.full((1, 1), np.nan), cons[1])[0, 0]
            for j in range(m.ncol):
                z = np.flatnonzero(~m.dense[1][:, j])
                zero[j] = r[z[0], j] if z.size else na
            return r[m.row_idx, col], zero
        if kind == "crossprod":
            return (np.where(m.dense[1], f, 0.0).T @ crossprod_Y(m.nrow)).T
    raise KeyError(kind)


# ---------------------------------------------------------------------------
# producers: the dense rule of a step on the actual arrays of its sources
# ---------------------------------------------------------------------------
ULPS_OPS = {"log1p": "log1p", "expm1": "expm1", "^": "^"}


class Want:
    """the expectation of one step: extents and type, and check(got Mat); .mat() is the rule's own result"""

    def __init__(self, nrow, ncol, type, expected=None, dense=None, stored=None, ulps_of=None):
        self.nrow, self.ncol, self.type, self.expected, self.ulps_of = nrow, ncol, type, expected, ulps_of
        self.dense, self.stored = (expected.dense, expected.stored) if expected is not None else (dense, stored)
        self.overflow = expected.overflow if expected is not None else False

    def check(self, got: Mat, what, max_ulps=0):
        check_invariants(got, self.nrow, self.ncol, self.type, what)
        gd, gs = got.dense
        if self.expected is not None:
            return ac.compare(gd, gs, self.expected, what, max_ulps)
        assert np.array_equal(gs, self.stored), f"{what}: the stored entries differ"
        assert np.array_equal(sc.bits(gd), sc.bits(self.dense)), f"{what}: values differ as bits"
        return 0

    def mat(self):
        return mat_from_dense(self.dense, self.stored, self.type)


def ulps_histogram(got: Mat, want: Want):
    """{distance in ulps: how many stored values} of a step compared in ulps, NaN results left out"""
    e = want.expected
    at = e.stored & got.dense[1]
    g, w = got.dense[0][at], e.dense[at]
    ok = ~np.isnan(w) & ~np.isnan(g)
    d, n = np.unique(np.asarray(ac.ulp_distance(g[ok], w[ok]), dtype=np.float64), return_counts=True)
    return {int(k): int(v) for k, v in zip(d, n)}


def _aperm_dense(a, dim, perm):
    """a: nrow x leaves in Fortran order of the array of extents ``dim``; 1-based ``perm``"""
    new = np.transpose(a.reshape(dim, order="F"), [p - 1 for p in perm])
    return np.asfortranarray(new.reshape((new.shape[0], -1), order="F"))


def rule(step, mats) -> Want:
    """``step``: (result, kind, source, *arguments); ``mats``: name -> Mat of everything made so far"""
    _, kind, src, *args = step
    x = mats[src]
    if kind == "scalar":
        op, s, st = args
        e = ac.expect_scalar(op, x.svt(), s, st)
        return Want(x.nrow, x.ncol, ac.out_type("scalar", op, x.type, st), e, ulps_of=ULPS_OPS.get(op))
    if kind == "merge":
        op, other = args
        y = mats[other]
        return Want(x.nrow, x.ncol, ac.out_type("merge", op, x.type, y.type), ac.expect_merge(op, x.svt(), y.svt()))
    if kind == "neg":
        return Want(x.nrow, x.ncol, x.type, ac.expect_neg(x.svt()))
    if kind == "math":
        return Want(x.nrow, x.ncol, "double", ac.expect_math(args[0], x.svt()), ulps_of=ULPS_OPS.get(args[0]))
    d, s = x.dense
    if kind == "subset":
        rows, cols = args[0], args[1]
        r = np.arange(x.nrow) if rows is None else np.asarray(rows, dtype=np.int64)
        c = np.arange(x.ncol) if cols is None else np.asarray(cols, dtype=np.int64)
        return Want(r.size, c.size, x.type, dense=np.asfortranarray(d[np.ix_(r, c)]), stored=np.asfortranarray(s[np.ix_(r, c)]))
    if kind == "t":
        return Want(x.ncol, x.nrow, x.type, dense=np.asfortranarray(d.T), stored=np.asfortranarray(s.T))
    if kind == "aperm":
        dim, perm = args
        dd, ss = _aperm_dense(d, dim, perm), _aperm_dense(s, dim, perm)
        return Want(dd.shape[0], dd.shape[1], x.type, dense=dd, stored=ss)
    raise KeyError(kind)


def subset_route(step, mats):
    """the route counts svt_dev_subset adds for a subset step (include/svt_hip.h): the column gather when cols is given;
    for rows the filter when they ascend strictly, else the composition t, gather, t"""
    rows, cols = step[3], step[4]
    want = {"column_gather": int(cols is not None), "row_filter": 0, "general_rows": 0}
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64)
        if np.all(np.diff(r) > 0):
            want["row_filter"] = 1
        else:
            want["general_rows"] = 1
            want["column_gather"] += 1
    return want


# ---------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------
class Chain:
    """``refused``: (operand, word of the message) -- Arith on that operand is an error, not a result"""

    def __init__(self, inputs, steps, consumers, claims=(), refused=()):
        self.inputs, self.steps, self.consumers, self.claims, self.refused = inputs, steps, consumers, claims, refused


_ROWS2 = _incr(DIM[0], 0.6, 51)
_COLS2 = _cols_with_repeats(52)
_ROWS2_GENERAL = _perm_rep(DIM[0], 700, 53)

CHAINS = {
    # z = log1p(x * s) - m: what the commit that added Arith names ("normalise, log, centre, product")
    "normalise_log_centre_consume": Chain(
        ("x", "m"),
        [("xs", "scalar", "x", "*", 0.001, "double"), ("l", "math", "xs", "log1p"), ("z", "merge", "l", "-", "m"),
         ("zt", "t", "z")],
        [("z", c) for c in FULL]),
    "subset_then_everything": Chain(
        ("x",),
        [("w", "subset", "x", _ROWS2, _COLS2), ("w2", "subset", "x", _ROWS2_GENERAL, None),
         ("wn", "neg", "w"), ("w0", "merge", "w", "+", "wn"),
         ("ww", "subset", "w", _incr(_ROWS2.size, 0.5, 54), _perm_rep(_COLS2.size, 90, 55)),
         ("wt", "t", "w"), ("wts", "subset", "wt", _perm_rep(_COLS2.size, 150, 56), _incr(_ROWS2.size, 0.3, 57)),
         ("w2t", "t", "w2")],
        [("w", c) for c in FULL] + [("w2", c) for c in FULL] + [("w0", c) for c in STATS + RANKS],
        claims=("w0 is empty",)),
    "empty_intermediates": Chain(
        ("x", "xs"),
        [("e_nnz0", "merge", "x", "-", "x"), ("e_nrow0", "subset", "x", np.zeros(0, np.int32), None),
         ("e_ncol0", "subset", "x", None, np.zeros(0, np.int32)), ("e_nan", "scalar", "xs", "*", 0.0, "double"),
         ("t_nnz0", "t", "e_nnz0"), ("t_nrow0", "t", "e_nrow0"), ("t_ncol0", "t", "e_ncol0"),
         ("again", "merge", "e_nnz0", "+", "e_nan"), ("none_of_none", "subset", "e_nnz0", _ROWS2, _COLS2)],
        [("e_nnz0", c) for c in FULL] + [("e_nrow0", c) for c in FULL] + [("e_ncol0", c) for c in FULL] +
        [("e_nan", c) for c in NOT_FINITE],
        claims=("e_nnz0 is empty", "e_nrow0 has no rows", "e_ncol0 has no columns", "e_nan holds only NaN")),
    "stored_zeros_and_specials": Chain(
        ("xs",),
        [("s", "subset", "xs", ROWS4, COLS4), ("y", "subset", "xs", _perm_rep(DIM[0], ROWS4.size, 63), _perm_rep(DIM[1], COLS4.size, 64)),
         ("plus", "merge", "s", "+", "y"), ("times", "merge", "s", "*", "y")],
        [("s", c) for c in RANKS + ORDER + [("colstats", "countNAs"), ("colstats", "min"), ("colstats", "max")]] +
        [("plus", c) for c in [("colstats", "countNAs"), ("colranks", "min")]] +
        [("times", c) for c in [("colstats", "countNAs"), ("colmedians", True)]],
        claims=("s holds every special", "plus drops zeros", "times drops zeros")),
    "type_changes": Chain(
        ("i", "m", "lg"),
        [("i65536", "scalar", "i", "*", 65536, "integer"), ("half", "scalar", "i", "/", 2, "integer"),
         ("i_plus_d", "merge", "i", "+", "m"), ("lgs", "subset", "lg", _ROWS2, _COLS2)],
        [("i65536", c) for c in [("colstats", "sum"), ("colstats", "min"), ("colstats", "max"), ("colstats", "countNAs"),
                                 ("colranks", "max"), ("colranks", "average"), ("colmedians", False), ("colmedians", True)]] +
        [("half", c) for c in [("colstats", "sum"), ("colmedians", True)]] +
        [("i_plus_d", c) for c in [("colstats", "sum"), ("colstats", "countNAs"), ("colmedians", True)]] +
        [("lgs", c) for c in [("colstats", "countNAs"), ("colranks", "dense")]],
        claims=("i65536 overflows", "lgs stays logical"), refused=(("lgs", "logical"),)),
    "t_and_aperm_results_as_inputs": Chain(
        ("x", "m", "a3", "b3"),
        [("xt", "t", "x"), ("mt", "t", "m"), ("xt_mt", "merge", "xt", "*", "mt"), ("xm", "merge", "x", "*", "m"),
         ("xm_t", "t", "xm"),
         ("a132", "aperm", "a3", (9, 5, 4), (1, 3, 2)), ("sum3", "merge", "a132", "+", "b3")],
        [("xt_mt", c) for c in [("colstats", "sum"), ("rowsums",), ("colmedians", False)]] +
        [("sum3", c) for c in [("colstats", "sum", 4), ("colstats", "mean", 4), ("colstats", "max", 4), ("colstats", "sum", 20)]],
        claims=("xt_mt equals xm_t",)),
}
NAMES = list(CHAINS)


def check_claim(claim, mats, wants):
    """what a chain says about its intermediates, on the arrays ``mats`` (actual on the GPU, the rules' own in the twin)"""
    if claim.endswith("is empty"):
        m = mats[claim.split()[0]]
        assert m.nnz == 0 and m.nrow > 0 and m.ncol > 0 and not m.col_ptr.any(), claim
    elif claim == "e_nrow0 has no rows":
        assert mats["e_nrow0"].nrow == 0 and mats["e_nrow0"].ncol == DIM[1] and mats["e_nrow0"].nnz == 0, claim
    elif claim == "e_ncol0 has no columns":
        assert mats["e_ncol0"].ncol == 0 and mats["e_ncol0"].nrow == DIM[0] and mats["e_ncol0"].nnz == 0, claim
    elif claim == "e_nan holds only NaN":
        v = mats["e_nan"].val
        assert 0 < v.size < mats["xs"].nnz and np.isnan(v).all(), claim
    elif claim == "s holds every special":
        have = set(sc.bits(mats["s"].val).tolist())
        assert set(sc.bits(sc.SPECIALS_F64).tolist()) <= have, claim     # NA_real_, two other NaNs, +-Inf, -0.0, 0.0
    elif claim in ("plus drops zeros", "times drops zeros"):
        name = claim.split()[0]
        s, y = mats["s"].dense[1], mats["y"].dense[1]
        assert 0 < int(wants[name].stored.sum()) < int((s | y).sum()), claim
        assert mats[name].nnz == 0 or not (mats[name].val == 0).any(), claim
    elif claim == "i65536 overflows":
        assert wants["i65536"].overflow and (mats["i65536"].val == NA_integer).sum() > (mats["i"].val == NA_integer).sum(), claim
        assert ((mats["i65536"].val != NA_integer) & (mats["i65536"].val != 0)).any(), claim
    elif claim == "lgs stays logical":
        assert mats["lgs"].type == "logical" and (mats["lgs"].val == NA_integer).any() and (mats["lgs"].val == 0).any(), claim
    elif claim == "xt_mt equals xm_t":
        a, b = mats["xt_mt"], mats["xm_t"]
        assert a.nnz > 500 and np.array_equal(a.col_ptr, b.col_ptr) and np.array_equal(a.row_idx, b.row_idx), claim
        assert np.array_equal(sc.bits(a.val), sc.bits(b.val)), claim
    else:
        raise KeyError(claim)
