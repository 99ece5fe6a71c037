"""Operands, subscripts and values for x[i, j, ...] <- value by an N-index (Session.subassign, DeviceCSC.subassign;
.subassign_SVT_by_Nindex, R/SparseArray-subassignment.R:114-170, C_subassign_SVT_with_short_Rvector,
src/SparseArray_subassignment.c:1005-1230), shared by tests/test_zzz_subassign_cpu.py (a per-leaf statement of the rule,
Session.subassign over a recording dispatcher) and tests/test_hip_subassign.py (the device routes).

The expectation is numpy's on the dense array after widening to the result's type (the wider of logical < integer <
double; NA_integer_ becomes NA_real_): ``dense[np.ix_(i0, j0, ...)] = value``, the vector recycled over the row
subscript (position p gets value[p % len(value)], the same in every selected leaf; positions apply in order, so the last
occurrence of a row wins -- written here as a loop over p, which does not lean on what numpy does with repeats).  Two
things are compared, both at tolerance 0: the values AS BITS (subset_cases.bits), and the mask of STORED entries --
``value != 0`` in the selected leaves (a NaN or NA is stored, -0.0 and 0 are not, and a stored zero of x there goes even
on a row outside i), x's own mask in every other leaf.  A cell that is not stored reads +0.

The shapes are the smallest that reach each branch of the device kernels: T = 2048 merged places per tile of the merge
(kernels_arith.hip), P = 4096 entries of the placed operand per tile of the placement's fill (kernels_subassign.hip).
"""
from __future__ import annotations

import functools

import numpy as np

from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from subset_cases import NP_DTYPE, SPECIALS_F64, bits, build

T = 2048
P = 4096
TYPE_ORDER = ("logical", "integer", "double")
NAN_PAYLOAD = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]


def wider(t1, t2):
    return max(t1, t2, key=TYPE_ORDER.index)


def widen(a, from_type, to_type):
    """values of ``from_type`` in the dtype of ``to_type``: the same bits, or int32 -> double with NA_integer_ -> NA_real_"""
    a = np.asarray(a, dtype=NP_DTYPE[from_type])
    if NP_DTYPE[to_type] == NP_DTYPE[from_type]:
        return a.copy()
    out = a.astype(np.float64)
    out[a == NA_integer] = NA_real
    return out


def nleaves_of(dim):
    return int(np.prod(dim[1:], dtype=np.int64)) if len(dim) > 1 else 1


def make(dim, type, mask, palette="tracer"):
    """an N-d object with exactly the entries of ``mask`` (nrow x leaves, the outermost dimension slowest) stored"""
    x2 = build((dim[0], nleaves_of(dim)), type, mask, palette)
    return SVT_SparseArray(tuple(dim), type, x2.leaves)


def dense_and_stored(x):
    """(dense values, mask of the stored entries) of an N-d object, both of x.dim"""
    flat = np.zeros((x.dim[0], len(x.leaves)), dtype=x.np_dtype, order="F")
    stored = np.zeros((x.dim[0], len(x.leaves)), dtype=bool, order="F")
    for c, lf in enumerate(x.leaves):
        if lf is None:
            continue
        flat[lf[0], c] = 1 if lf[1] is None else lf[1]
        stored[lf[0], c] = True
    return np.reshape(flat, x.dim, order="F"), np.reshape(stored, x.dim, order="F")


def index0(dim, index):
    """the 0-based subscripts, the whole axis written out"""
    return [np.arange(d, dtype=np.int64) if s is None else np.asarray(s, dtype=np.int64).reshape(-1) - 1
            for s, d in zip(index, dim)]


def leaf_list(dim, index):
    """the 0-based numbers of the selected leaves in the order of the leaves of a value with the selection's dims (the
    outermost dimension slowest), or None when every subscript of dims 2..N is missing"""
    if all(s is None for s in index[1:]):
        return None
    sub = index0(dim, index)[1:]
    lens = [len(s) for s in sub]
    out = np.zeros(int(np.prod(lens, dtype=np.int64)), dtype=np.int64)
    stride, rep = 1, 1
    for s, d, n in zip(sub, dim[1:], lens):
        # position q of the list has coordinate (q // rep) % n along this dimension
        q = np.arange(out.size)
        out += stride * s[(q // rep) % n] if n else 0
        stride *= d
        rep *= n
    return out.astype(np.int32)


def _mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def _vec(type, n, seed, zeros=0.0):
    """n values of ``type``, none of them zero unless ``zeros`` > 0"""
    rng = np.random.default_rng(seed)
    if type == "double":
        v = rng.integers(1, 50, n).astype(np.float64) / 4 * rng.choice([-1.0, 1.0], n)
    elif type == "integer":
        v = (rng.integers(1, 50, n) * rng.choice([-1, 1], n)).astype(np.int32)
    else:
        v = np.ones(n, dtype=np.int32)
    if zeros:
        v[rng.random(n) < zeros] = 0
    return v


def _host_subset(x, index):
    """x[i, j, ...] on the host, stored entries kept as they are (the value of the put-back cases)"""
    dense, stored = dense_and_stored(x)
    sel = np.ix_(*index0(x.dim, index))
    d, s = dense[sel], stored[sel]
    dim = d.shape
    d2, s2 = np.reshape(d, (dim[0], -1), order="F"), np.reshape(s, (dim[0], -1), order="F")
    leaves = []
    for c in range(d2.shape[1]):
        offs = np.flatnonzero(s2[:, c]).astype(np.int32)
        leaves.append(None if offs.size == 0 else (offs, np.ascontiguousarray(d2[offs, c])))
    return SVT_SparseArray(dim, x.type, leaves)


def _times(v, k):
    """v * k on the host for a tracer operand (no NA, no overflow at these sizes)"""
    return SVT_SparseArray(v.dim, v.type, [None if lf is None else (lf[0], (lf[1] * k).astype(v.np_dtype)) for lf in v.leaves])


# ---------------------------------------------------------------------------
# the cases: name -> () -> (x, index (1-based, None = the whole axis), value, value type)
# value: a 1-D numpy array (the vector form) or an SVT_SparseArray (the SVT form)
# ---------------------------------------------------------------------------
def _merged_length(total):
    """nnz(x) + nnz(Y) == total: 1047 entries of Y in one column of 1200 rows, over about 730 entries of x, next to an
    untouched column of 172"""
    def f():
        nx = total - 1047 - 172
        mask = np.zeros((1200, 2), dtype=bool)
        mask[:nx, 1] = True
        mask[::7, 0] = True
        x = make((1200, 2), "double", mask)
        v = np.zeros(1200)
        v[100:1147] = _vec("double", 1047, 40)
        return x, [None, [2]], v, "double"
    return f


def _pair_split():
    # one column: x stores rows 0 .. 1100, Y rows 1 .. 1100: the merged sequence is x0, x1 y1, x2 y2, ... -- x1024 is
    # place 2047, the last of the first tile, and the y entry it is paired with the first of the second
    mask = np.zeros((1200, 1), dtype=bool)
    mask[:1101, 0] = True
    x = make((1200, 1), "double", mask)
    v = np.zeros(1200)
    v[1:1101] = _vec("double", 1100, 41)
    return x, [None, [1]], v, "double"


def _column_of_5000():
    mask = _mask((5000, 3), 0.01, 42)
    mask[:, 1] = np.arange(5000) % 2 == 0                               # 2500 entries of x in the covered column
    x = make((5000, 3), "double", mask)
    return x, [None, [2]], _vec("double", 5000, 43, zeros=0.48), "double"       # about 2600 of Y: three tiles


def _empty_columns():
    mask = np.zeros((40, 304), dtype=bool)
    mask[:, 1] = mask[:, 302] = True
    x = make((40, 304), "double", mask)
    return x, [list(range(3, 38)), [1, 2, 150, 151, 303, 304]], _vec("double", 35, 44, zeros=0.3), "double"


def _filter():
    x = make((600, 160), "double", _mask((600, 160), 0.1, 45) | (np.arange(160) == 80)[None, :])
    rows = (np.flatnonzero(_mask(600, 0.5, 46)) + 1).tolist()
    cols = (np.flatnonzero(_mask(160, 0.5, 47)) + 1).tolist()
    return x, [rows, cols], np.array([0.0]), "double"


def _x_empty():
    x = make((70, 9), "double", np.zeros((70, 9), dtype=bool))
    return x, [[5, 9, 60], [2, 9]], np.array([1.5, -2.0, 3.25]), "double"


def _wholly_covered():
    x = make((90, 11), "double", _mask((90, 11), 0.4, 48), "specials")
    return x, [None, None], _vec("double", 90, 49, zeros=0.5), "double"


def _nothing_covered(which):
    def f():
        x = make((37, 23), "integer", _mask((37, 23), 0.2, 50), "specials")
        return x, ([[], None] if which == "i" else [None, []]), np.array([2.5]), "double"
    return f


def _replicated():
    x = make((50, 400), "double", _mask((50, 400), 0.05, 51))
    rows = list(range(11, 41))
    return x, [rows, None], _vec("double", 30, 52), "double"            # Y: 400 leaves of 30 entries, three tiles of P


def _rows_reversed():
    x = make((37, 23), "double", _mask((37, 23), 0.3, 53))
    return x, [list(range(37, 0, -1)), [3, 4, 20]], _vec("double", 37, 54, zeros=0.2), "double"


def _rows_repeated():
    x = make((37, 23), "double", _mask((37, 23), 0.3, 55))
    rows = [3, 3, 3, 1, 37, 1, 20, 20, 3, 12]                           # row 3: 1., 2., 3. and then 0. -- the zero wins
    return x, [rows, [1, 5, 23]], np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.0, 8.0, 0.0, 10.0]), "double"


def _leaves_repeated():
    x = make((29, 31), "integer", _mask((29, 31), 0.25, 56))
    return x, [[2, 5, 9, 28], [31, 1, 1, 1, 7, 31, 7]], np.array([4, 0, -6, 8], dtype=np.int32), "integer"


def _nvals(n):
    def f():
        x = make((37, 23), "double", _mask((37, 23), 0.3, 57))
        rows = [36, 2, 4, 30, 9, 11]
        return x, [rows, [2, 3, 22]], _vec("double", n, 58 + n), "double"
    return f


def _special_values():
    x = make((37, 23), "double", _mask((37, 23), 0.4, 60), "specials")
    rows = list(range(2, 34))
    v = np.tile(np.array([0.0, -0.0, NA_real, NAN_PAYLOAD, np.inf, 1.5, SPECIALS_F64[2], -7.0]), 4)
    return x, [rows, [1, 2, 10, 23]], v, "double"


def _special_integers():
    x = make((29, 31), "integer", _mask((29, 31), 0.4, 61), "specials")
    return x, [[1, 4, 5, 29], [2, 30]], np.array([0, NA_integer, 2 ** 31 - 1, -1], dtype=np.int32), "integer"


def _stored_zeros():
    # the specials palette stores 0.0 and -0.0: in the selected leaves they go, rows 1 .. 10 assigned or not; elsewhere they stay
    x = make((37, 23), "double", np.ones((37, 23), dtype=bool), "specials")
    return x, [list(range(1, 11)), [2, 3, 4, 5, 6, 7, 8, 9]], np.array([9.0]), "double"


def _type_pair_vector(tx, tv):
    def f():
        x = make((19, 17), tx, _mask((19, 17), 0.4, 62), "specials")
        v = {"double": np.array([0.0, 2.5, NA_real]), "integer": np.array([0, NA_integer, 7], dtype=np.int32),
             "logical": np.array([1, 0, 1], dtype=np.int32)}[tv]     # (a Python caller has no logical NA to write)
        return x, [[1, 2, 3, 9, 10, 19], [1, 8, 17]], v, tv
    return f


def _type_pair_svt(tx, tv):
    def f():
        x = make((19, 17), tx, _mask((19, 17), 0.4, 63), "specials")
        v = make((6, 3), tv, _mask((6, 3), 0.6, 64), "specials")
        return x, [[1, 2, 3, 9, 10, 19], [17, 1, 8]], v, tv
    return f


def _three_d():
    x = make((13, 5, 4), "double", _mask((13, 20), 0.3, 65), "specials")
    return x, [[2, 3, 13], [5, 1], [4, 2, 2]], np.array([1.0, 0.0, NA_real]), "double"


def _four_d():
    x = make((7, 3, 4, 2), "integer", _mask((7, 24), 0.4, 66))
    return x, [None, [3], None, [2, 1]], np.array([5], dtype=np.int32), "integer"


def _three_d_svt():
    x = make((13, 5, 4), "double", _mask((13, 20), 0.3, 67))
    index = [[2, 3, 13], [5, 1], [4, 2]]
    v = make((3, 2, 2), "double", _mask((3, 4), 0.7, 68), "specials")
    return x, index, v, "double"


def _put_back(k):
    def f():
        x = make((600, 160), "double", _mask((600, 160), 0.1, 69) | (np.arange(160) == 80)[None, :])
        index = [(np.flatnonzero(_mask(600, 0.5, 70)) + 1).tolist(), list(range(40, 121))]
        v = _host_subset(x, index)
        return x, index, (v if k == 1 else _times(v, k)), "double"
    return f


def _svt_leaves_reversed():
    x = make((37, 23), "double", _mask((37, 23), 0.3, 71))
    index = [[1, 5, 6, 30, 37], list(range(23, 0, -1))]
    return x, index, make((5, 23), "double", _mask((5, 23), 0.5, 72)), "double"


def _svt_stored_zeros():
    x = make((37, 23), "double", _mask((37, 23), 0.5, 73), "specials")
    return x, [list(range(4, 24)), [2, 9, 1]], make((20, 3), "double", np.ones((20, 3), dtype=bool), "specials"), "double"


def _svt_whole_axes():
    x = make((37, 23), "integer", _mask((37, 23), 0.3, 74))
    return x, [None, None], make((37, 23), "integer", _mask((37, 23), 0.2, 75), "specials"), "integer"


_CASES = {
    "merged_length_T_minus_1": _merged_length(T - 1),
    "merged_length_T": _merged_length(T),
    "merged_length_T_plus_1": _merged_length(T + 1),
    "pair_split_across_a_tile_edge": _pair_split,
    "covered_column_of_5000_rows": _column_of_5000,
    "300_empty_columns_around_two_full_ones": _empty_columns,
    "filter_value_zero": _filter,
    "x_without_nonzeros": _x_empty,
    "x_wholly_covered": _wholly_covered,
    "nothing_covered_empty_i": _nothing_covered("i"),
    "nothing_covered_empty_j": _nothing_covered("j"),
    "patch_leaf_over_400_leaves": _replicated,
    "rows_reversed": _rows_reversed,
    "rows_repeated_last_wins": _rows_repeated,
    "leaves_repeated": _leaves_repeated,
    "nvals_1": _nvals(1),
    "nvals_3": _nvals(3),
    "nvals_len_i": _nvals(6),
    "values_zero_minus_zero_NA_NaN": _special_values,
    "values_integer_zero_NA": _special_integers,
    "stored_zeros_of_x_inside_and_outside": _stored_zeros,
    "three_d": _three_d,
    "four_d": _four_d,
    "svt_three_d": _three_d_svt,
    "svt_put_back_of_subset": _put_back(1),
    "svt_put_back_of_subset_times_2": _put_back(2),
    "svt_leaves_reversed": _svt_leaves_reversed,
    "svt_v_with_stored_zeros": _svt_stored_zeros,
    "svt_whole_axes": _svt_whole_axes,
}
for _tx in TYPE_ORDER:
    for _tv in TYPE_ORDER:
        _CASES[f"types_{_tx}_vector_{_tv}"] = _type_pair_vector(_tx, _tv)
        _CASES[f"types_{_tx}_svt_{_tv}"] = _type_pair_svt(_tx, _tv)
NAMES = list(_CASES)
SVT_NAMES = [n for n in NAMES if n.startswith("svt_") or "_svt_" in n]


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, index, value, value type, result type, expected dense (read-only), expected stored mask (read-only))"""
    x, index, value, v_type = _CASES[name]()
    new_type = wider(x.type, v_type)
    dense, stored = dense_and_stored(x)
    want = np.asfortranarray(np.reshape(widen(dense, x.type, new_type), x.dim, order="F"))
    sub = index0(x.dim, index)
    selected = np.zeros(x.dim, dtype=bool)
    if all(len(s) for s in sub):
        selected[np.ix_(np.arange(x.dim[0]), *sub[1:])] = True          # the selected leaves, every row of them
        if isinstance(value, SVT_SparseArray):
            assert value.dim == tuple(len(s) for s in sub)
            want[np.ix_(*sub)] = widen(dense_and_stored(value)[0], v_type, new_type)
        else:
            v = widen(value, v_type, new_type)
            assert 1 <= v.size <= len(sub[0]) and len(sub[0]) % v.size == 0, "the short form"
            for p, r in enumerate(sub[0]):                              # in order: the last occurrence of a row wins
                want[np.ix_([r], *sub[1:])] = v[p % v.size]
    want_stored = np.where(selected, want != 0, stored)                 # (a NaN != 0; -0.0 == 0)
    want[~want_stored] = 0
    want.setflags(write=False)
    want_stored.setflags(write=False)
    return x, index, value, v_type, new_type, want, want_stored


def check_invariants(res, dim, type_):
    assert isinstance(res, SVT_SparseArray)
    assert res.dim == tuple(dim) and res.type == type_ and not res.na_background
    assert len(res.leaves) == nleaves_of(dim)
    for lf in res.leaves:
        if lf is None:
            continue
        offs = np.asarray(lf[0])
        assert offs.size > 0 and offs.dtype == np.int32
        assert offs[0] >= 0 and offs[-1] < dim[0] and np.all(np.diff(offs) > 0)
        assert lf[1] is None or (len(lf[1]) == offs.size and np.asarray(lf[1]).dtype == NP_DTYPE[type_])


def check(res, name, what=""):
    x, _, _, _, new_type, want, want_stored = case(name)
    what = f"{what}{name}"
    check_invariants(res, x.dim, new_type)
    got, got_stored = dense_and_stored(res)
    assert np.array_equal(got_stored, want_stored), f"{what}: the stored entries differ"
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), f"{what}: values differ as bits"


def restate(x, index, value, v_type):
    """The rule leaf by leaf, written for the tests: a leaf all of whose coordinates along dims 2..N are in the
    subscripts is rebuilt from its dense form -- the assignments in the order of the row subscript, then an entry
    exactly where the final value is not zero; every other leaf is x's, widened."""
    new_type = wider(x.type, v_type)
    sub = index0(x.dim, index)
    lens = [len(s) for s in sub]
    empty = any(n == 0 for n in lens)
    is_svt = isinstance(value, SVT_SparseArray)
    if not empty and not is_svt:
        v = widen(value, v_type, new_type)
    leaves = []
    for q, lf in enumerate(x.leaves):
        coords, rest = [], q
        for d in x.dim[1:]:
            coords.append(rest % d)
            rest //= d
        where = [np.flatnonzero(s == c) for s, c in zip(sub[1:], coords)]
        if empty or any(w.size == 0 for w in where):
            leaves.append(None if lf is None else
                          (lf[0], widen(np.ones(len(lf[0]), x.np_dtype) if lf[1] is None else lf[1], x.type, new_type)))
            continue
        col = np.zeros(x.dim[0], dtype=NP_DTYPE[new_type])
        if lf is not None:
            col[lf[0]] = widen(np.ones(len(lf[0]), x.np_dtype) if lf[1] is None else lf[1], x.type, new_type)
        if is_svt:
            # (no repeats in the SVT form: one leaf of v lands here)
            vq, stride = 0, 1
            for w, n in zip(where, lens[1:]):
                vq += stride * int(w[-1])
                stride *= n
            src = np.zeros(lens[0], dtype=NP_DTYPE[new_type])
            vl = value.leaves[vq]
            if vl is not None:
                src[vl[0]] = widen(np.ones(len(vl[0]), value.np_dtype) if vl[1] is None else vl[1], v_type, new_type)
            for p, r in enumerate(sub[0]):
                col[r] = src[p]
        else:
            for p, r in enumerate(sub[0]):
                col[r] = v[p % v.size]
        keep = (col != 0) | (col != col)
        offs = np.flatnonzero(keep).astype(np.int32)
        leaves.append(None if offs.size == 0 else (offs, np.ascontiguousarray(col[offs])))
    return SVT_SparseArray(x.dim, new_type, leaves, dimnames=x.dimnames)
