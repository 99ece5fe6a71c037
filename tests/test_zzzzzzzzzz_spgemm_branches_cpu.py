"""The cases of tests/spgemm_branch_cases.py without a GPU: ``expect_csc`` proved equal to ``spgemm_cases.expect``
(on every device case of spgemm_cases for the three panel heights, and on every new case that exists as a dense
operand), every case proved to have the property it is named for -- asserted from its shape against the selection
rules quoted in the module docstring of spgemm_branch_cases -- and ``expect`` itself held to the exact product within
Higham's ``gamma(n) M``."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import exact_products as ep
import spgemm_branch_cases as bc
import spgemm_cases as gc

bits = ac.sc.bits


@pytest.fixture(scope="module")
def panel():
    from sparsearray_amd.device import spgemm_panel
    P = spgemm_panel(10 ** 6)
    assert P in gc.PANELS
    return P


def _assert_same_as_expect(A, B, what):
    want = gc.expect(A, B)
    (cp, ri, vv), cls, not_finite = bc.expect_csc(A.shape, A.csc, B.shape, B.csc)
    wcp, wri, wv = want.csc
    assert cp.dtype == np.int64 and np.array_equal(cp, wcp), f"{what}: col_ptr"
    assert ri.dtype == np.int32 and np.array_equal(ri, wri), f"{what}: row_idx"
    assert vv.dtype == np.float64 and np.array_equal(bits(vv), bits(wv)), f"{what}: values as bits"
    assert np.array_equal(cls, want.csc_cls), f"{what}: classes"
    assert not_finite == want.not_finite, f"{what}: not_finite"
    return want


# ---------------------------------------------------------------------------
# A. expect_csc is expect()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", gc.PANELS)
def test_expect_csc_is_expect_on_every_device_case(P):
    cases = gc.device_cases(P)
    assert list(cases) == gc.DEVICE_NAMES
    for name in gc.DEVICE_NAMES:
        _assert_same_as_expect(cases[name].A, cases[name].B, f"{name}, P = {P}")


@pytest.mark.parametrize("name", bc.SMALL)
def test_expect_csc_is_expect_on_every_small_case(panel, name):
    c = bc.case(panel, name)
    want = _assert_same_as_expect(c.A, c.B, name)
    assert np.array_equal(bits(c.want.csc[2]), bits(want.csc[2])) and c.want.csc[1].size > 0


def test_expect_csc_on_a_literal_case_and_the_vectors_are_reused():
    A = gc.Op.of(3, 2, [0, 2, 1, 2], [0, 0, 1, 1], [2.0, 3.0, 5.0, -3.0])
    B = gc.Op.of(2, 3, [0, 1, 1, 0], [0, 0, 1, 2], [1.0, 1.0, 0.0, -1.0])
    (cp, ri, vv), cls, not_finite = bc.expect_csc(A.shape, A.csc, B.shape, B.csc)
    # column 0: 2, 5, 3 - 3 (dropped); column 1: 5 * 0 and -3 * 0 (reached, zero); column 2 starts from +0.0 again
    assert cp.tolist() == [0, 2, 2, 4] and ri.tolist() == [0, 1, 0, 2] and vv.tolist() == [2.0, 5.0, -2.0, -3.0]
    assert cls.tolist() == [ac.EXACT] * 4 and not not_finite


def test_names_only_at_import():
    assert bc.case.cache_info().currsize <= len(bc.NAMES) and len(set(bc.NAMES)) == len(bc.NAMES)
    assert set(bc.TALL) <= set(bc.NAMES) and set(bc.SMALL) | set(bc.TALL) == set(bc.NAMES)


# ---------------------------------------------------------------------------
# B.1 metadata batches
# ---------------------------------------------------------------------------
def _batches(n):
    """the pairs per metadata batch of a column of n entries"""
    return [min(64, n - c0) for c0 in range(0, n, 64)]


def test_b_column_family_covers_the_batch_loop():
    assert _batches(63) == [63] and _batches(64) == [64] and _batches(65) == [64, 1]
    last = {n: _batches(n)[-1] for n in bc.B_COLUMN_N}
    assert {last[n] % 4 for n in bc.B_COLUMN_N if n > 64} == {0, 1, 2, 3}       # lanes past np must hold len == 0
    assert last[128] == 64 and len(_batches(128)) == 2                          # np of 64 in a second batch
    assert len(_batches(129)) == 3 and len(_batches(200)) == 4


@pytest.mark.parametrize("name", [n for n in bc.NAMES if n.startswith("b_column_")])
def test_b_column_cases_are_what_their_names_say(panel, name):
    P, c = panel, bc.case(panel, name)
    n = int(name.split("_")[2])
    assert c.A.shape == (P + 9, n) and c.B.shape == (n, 3) and c.A.type == "double"
    assert c.A.stored[P - 1].all() and c.A.stored[P].all()                      # every leaf on either side of the edge
    assert 0.02 < c.A.nnz / c.A.stored.size < 0.04
    assert max(max(bc.runs(c.A, j, P)) for j in range(n)) < 128
    nb = c.B.stored.sum(axis=0)
    assert nb.tolist() == [n, 0, len({0, 63, 64, n - 1} & set(range(n)))]
    assert np.flatnonzero(c.B.stored[:, 2]).tolist() == sorted({0, 63, 64, n - 1} & set(range(n)))
    for k in (0, 2):                                                            # every pair meets in two cells across the edge
        rows, vals = c.want.column(k)
        assert {P - 1, P} <= set(rows.tolist())
    assert c.want.column(1)[0].size == 0
    assert c.B.type == ("integer" if "integer" in name else "double")
    if "NA_integer" in name:
        at = int(name.rsplit("_", 1)[1])
        assert at >= 64 and c.B.dense[at, 0] == bc.NA_integer and (c.B.dense == bc.NA_integer).sum() == 1
        assert c.want.not_finite
        rows, vals = c.want.column(0)
        hit = np.isin(rows, bc.leaf(c.A, at)[1])
        assert hit.sum() == bc.leaf(c.A, at)[1].size                            # the cells of that leaf: all kept, all NaN
        assert np.isnan(vals[hit]).all() and np.isfinite(vals[~hit]).all()
        assert np.array_equal(c.want.csc_cls[:rows.size] == ac.ANY_NAN, hit)
        assert np.isfinite(c.want.column(2)[1]).all() or at in (63, 64, n - 1)
    else:
        assert not c.want.not_finite and np.isfinite(c.want.csc[2]).all()


# ---------------------------------------------------------------------------
# B.2 the order across batch and group edges
# ---------------------------------------------------------------------------
def test_the_order_case_tells_orders_apart_across_batches_and_groups(panel):
    P, c = panel, bc.case(panel, "order_across_batches")
    assert c.A.shape == (P + 5, 200) and c.B.shape == (200, 1) and c.B.stored.all() and (c.B.dense == 1.0).all()
    assert len(_batches(200)) == 4
    for r, js, pattern in bc.ORDER_ROWS(P):
        assert np.flatnonzero(c.A.stored[r]).tolist() == list(js) and c.A.dense[r, list(js)].tolist() == list(pattern)
        got = c.want.cell(r, 0)
        assert got is None if pattern == bc.ORDER_ZERO else got == 1.0, (r, got)
    assert c.want.csc[1].tolist() == [6, 8, 10, 12, 14] and not c.want.not_finite
    # B's column is full: the position of a pair in the column is its j
    batch, group = (lambda j: j // 64), (lambda j: j // 4)
    assert len({batch(j) for j in (10, 70, 130)}) == 3                          # three batches
    assert group(2) == group(3) != group(4) and batch(63) != batch(64) and group(62) == group(63)
    assert group(4) == group(5) == group(6) and group(64) == group(65) == group(66) and batch(64) == 1
    # the same products in other orders: (a) the first two exchanged -- nothing to see; (b) a group visited backwards
    assert (1.0 + 1e16) + -1e16 == 0.0 and (-1e16 + 1e16) + 1.0 == 1.0
    assert (1.0 + -1e16) + 1e16 == 0.0 != 1.0                                  # ORDER_ONE backwards: rows 12 and 14 vanish
    # a dropped batch: row 6 loses its last term (1e16 - 1e16 = 0, not stored), row 5 keeps 1e16 + 1
    assert 1e16 + -1e16 == 0.0 and 1e16 + 1.0 != 0.0


# ---------------------------------------------------------------------------
# B.3 run lengths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.RUN_N)
def test_run_cases_hold_runs_of_exactly_n(panel, n):
    P, c = panel, bc.case(panel, f"run_{n}")
    assert c.A.shape == (2 * P + 3, 3) and c.B.shape == (3, 2) and c.B.stored.all()
    assert bc.runs(c.A, 0, P) == [n] and bc.leaf(c.A, 0)[1][-1] == P - 1       # ends at the edge
    assert bc.runs(c.A, 1, P) == [n] and bc.leaf(c.A, 1)[1][0] == P            # starts at it
    assert bc.runs(c.A, 2, P) == [n // 2, n - n // 2] and max(bc.runs(c.A, 2, P)) < n
    assert np.all(np.diff(bc.leaf(c.A, 2)[1]) == 1)
    products = c.A.stored.astype(int) @ c.B.stored.astype(int)
    assert products.max() == 2 and products[P - 1, 0] == 2 and products[P, 1] == 2
    assert (63 in (n, n // 2, n - n // 2)) or n >= 64


def test_run_family_covers_the_lane_count_edges():
    assert set(bc.RUN_N) == {63, 64, 65, 128, 129}
    trips = {n: len(range(64, n, 64)) for n in bc.RUN_N}                        # trips of for (x = 64; x < plen; x += 64)
    assert trips == {63: 0, 64: 0, 65: 1, 128: 1, 129: 2}


# ---------------------------------------------------------------------------
# B.4 split forms and the scan's second trip
# ---------------------------------------------------------------------------
def split_rule(ncol, nnz):
    """rowpanel_split() of kernels_rowstats.hip"""
    if ncol <= 0 or nnz // ncol < bc.SPLIT_AT:
        return 1
    best, best_t = 1, 1e30
    for sp in (1, 2, 4):
        nwg = (ncol * sp + 15) // 16
        t = ((nwg + 511) // 512) / sp
        if t < best_t - 1e-9:
            best, best_t = sp, t
    return best


def _lds_form(P, nrow):
    return ((nrow + P - 1) // P + 1) * 16 * 4 <= 64 * 1024


def test_the_split_rule_at_its_edges():
    big = 10 ** 9
    assert split_rule(1, big) == 4 and split_rule(2048, 2048 * 2048) == 4
    assert split_rule(2049, 2049 * 2048) == 2 and split_rule(4096, big * 10) == 2
    assert split_rule(2049, 2049 * 2048 - 1) == 1 and split_rule(6, 6 * 2048 - 1) == 1


def test_split_cases_are_what_their_names_say(panel):
    P = panel
    c = bc.case(P, "split4")
    lens = np.diff(c.A.csc[0])
    assert c.A.shape == (3 * P, 6) and c.A.nnz // 6 >= 2048 and 6 <= 2048 and lens.min() > bc.SCAN_TRIP
    assert split_rule(6, c.A.nnz) == 4 and _lds_form(P, 3 * P)
    assert 2 not in bc.referred(c.B) and 5 in bc.referred(c.B)

    c = bc.case(P, "split4_ragged")
    lens = np.diff(c.A.csc[0])
    assert c.A.shape == (3 * P, 7) and c.A.nnz // 7 >= 2048 and split_rule(7, c.A.nnz) == 4
    assert lens[1] == 0 and lens[2] == 3 and bc.leaf(c.A, 2)[1].tolist() == [P - 1, P, 3 * P - 1]
    segments = lambda n: [n * (sg + 1) // 4 - n * sg // 4 for sg in range(4)]   # noqa: E731  (entries per segment)
    assert segments(3) == [0, 1, 1, 1] and segments(1) == [0, 0, 0, 1]          # leaf 6: three of four segments empty
    assert lens[6] == 1 and bc.leaf(c.A, 6)[1].tolist() == [P]
    assert bc.leaf(c.A, 3)[1].min() >= 2 * P and lens[3] > 1024 and bc.leaf(c.A, 4)[1].max() < P and lens[4] > 1024
    assert set(range(7)) == set(bc.referred(c.B).tolist())                      # the empty leaf is referred to as well
    assert {P - 1, P, 3 * P - 1} <= set(c.want.column(2)[0].tolist()) and P in c.want.column(3)[0].tolist()

    c = bc.case(P, "split2")
    lens = np.diff(c.A.csc[0])
    ncol = bc.SPLIT2_NCOL
    assert c.A.shape == (2 * P + 3, ncol) and c.A.nnz // ncol >= 2048 and 2048 < ncol <= 4096
    assert split_rule(ncol, c.A.nnz) == 2 and _lds_form(P, 2 * P + 3) and lens.min() > 1024
    per_column = c.B.stored.sum(axis=0)
    assert c.B.shape == (ncol, 3) and per_column.min() >= 65 and per_column.max() <= 128   # two metadata batches
    assert {0, ncol - 1} <= set(bc.referred(c.B).tolist()) and ncol - 2 not in bc.referred(c.B)

    c = bc.case(P, "long_leaf_unsplit")
    lens = np.diff(c.A.csc[0])
    assert c.A.shape == (3 * P, 8) and c.A.nnz // 8 < 2048 and split_rule(8, c.A.nnz) == 1
    assert lens[bc.LONG_LEAF] > bc.SCAN_TRIP and np.delete(lens, bc.LONG_LEAF).max() < 30 and lens.min() >= 2
    assert bc.LONG_LEAF in bc.referred(c.B) and not {2, 5, 6} & set(bc.referred(c.B).tolist())


@pytest.mark.parametrize("form", bc.FLAG_FORMS)
def test_flag_variants_raise_the_flag_and_give_values_by_class(panel, form):
    c = bc.case(panel, form)
    places = bc.flag_places(c)
    positions = {p for what, j, p in places if what.startswith("long leaf")}
    n_long = int(np.diff(c.A.csc[0])[places[0][1]])
    assert {0, n_long - 1, n_long // 2 - 1, n_long // 2} <= positions
    if form != "split2" or n_long > bc.SCAN_TRIP:       # (a leaf of split2 is 0.55 (2 P + 3) long: below 4096 at P = 2048)
        assert {bc.SCAN_TRIP - 1, bc.SCAN_TRIP} <= positions
    assert [what for what, _, _ in places[-2:]] == ["the last leaf of A, its last position", "a leaf nobody refers to"]
    assert places[-2][1] == c.A.shape[1] - 1 and places[-1][1] not in bc.referred(c.B)
    for type in ("double", "integer"):
        A0 = bc.sparse(c.A) if type == "double" else bc.as_integer(c.A, 3900)
        base = bc.ExpectedCSC(A0, c.B)
        assert not base.not_finite
        for what, j, pos in places:
            for tag, v in bc.SPECIALS[type]:
                A, at = bc.with_special(A0, j, pos, v)
                want = bc.ExpectedCSC(A, c.B)
                assert want.not_finite, (form, what, tag)
                assert np.array_equal(want.csc[0], base.csc[0]) and np.array_equal(want.csc[1], base.csc[1])
                changed = bits(want.csc[2]) != bits(base.csc[2])
                if j not in bc.referred(c.B):
                    assert not changed.any()
                    continue
                row = A.csc[1][at]
                assert changed.any() and np.all(want.csc[1][changed] == row)    # the cells of that row, nothing else
                assert np.array_equal(changed, ~np.isfinite(want.csc[2]))
                if tag == "Inf":
                    assert np.isinf(want.csc[2][changed]).all() and np.all(want.csc_cls == ac.EXACT)
                else:
                    assert np.isnan(want.csc[2][changed]).all() and np.array_equal(want.csc_cls == ac.ANY_NAN, changed)


# ---------------------------------------------------------------------------
# B.5 very tall A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TALL)
def test_tall_cases_are_what_their_names_say(panel, name):
    P, c = panel, bc.case(panel, name)
    A, B = c.A, c.B
    assert isinstance(A, bc.SparseOp) and isinstance(B, bc.SparseOp)            # CSC only: no nrow x ncol array anywhere
    nrow, ninner = A.shape
    npan = (nrow + P - 1) // P
    lens = np.diff(A.csc[0])
    if name == "tall_last_lds":
        assert nrow == 1023 * P and npan == 1023 and (npan + 1) * 64 <= 65536 and _lds_form(P, nrow)
    else:
        assert nrow == 1023 * P + 1 and npan == 1024 and (npan + 1) * 64 > 65536 and not _lds_form(P, nrow)
        assert (nrow - 1) % P == 0                                              # the single row of the last panel
    wide = (A.nnz // ninner >= bc.WIDE_AT and ninner > 1) or ninner == 1        # the workgroup-per-leaf form
    assert (ninner, wide) == {"tall_last_lds": (5, False), "tall_narrow": (5, False), "tall_wide": (2, True),
                              "tall_wide_empty_leaf": (3, True), "tall_one_leaf": (1, True)}[name]
    assert wide or (ninner + 3) // 4 != ninner                                  # the kernel tells the forms apart by its grid
    want_lens = {"tall_last_lds": 40, "tall_narrow": 40, "tall_wide": 1500, "tall_wide_empty_leaf": 2300, "tall_one_leaf": 300}[name]
    full = np.flatnonzero(lens > 0)
    assert np.all(np.abs(lens[full] - want_lens) <= 5)
    assert (lens == 0).sum() == (1 if name in ("tall_last_lds", "tall_narrow", "tall_wide_empty_leaf") else 0)
    if name == "tall_wide":
        assert A.nnz // ninner >= 1024
    for j in (full[0], full[-1]):
        rows = bc.leaf(A, j)[1]
        assert set(bc.tall_marks(P, nrow)) <= set(rows.tolist())
        assert np.unique(rows >> (P.bit_length() - 1)).size <= 5                # long stretches of empty panels
    assert np.unique(A.csc[1] >> (P.bit_length() - 1)).size <= 5
    # B: K = 3, column 0 full, column 1 empty, column 2 refers to the last leaf (and to the empty one where there is one)
    nb = np.diff(B.csc[0])
    assert B.shape == (ninner, 3) and nb[0] == ninner and nb[1] == 0 and nb[2] >= 1
    assert ninner - 1 in B.csc[1][B.csc[0][2]:].tolist()
    if (lens == 0).any():
        assert int(np.flatnonzero(lens == 0)[0]) in bc.referred(B)
    for k in (0, 2):
        assert set(bc.tall_marks(P, nrow)) <= set(c.want.column(k)[0].tolist())
    assert c.want.column(1)[0].size == 0 and not c.want.not_finite
    # the flag variants: a special at the first and at the last value of A, both types
    places = bc.tall_flag_places(c)
    assert [bc.with_special(A, j, pos, 1.0)[1] for _, j, pos in places] == [0, A.nnz - 1]
    for type in ("double", "integer"):
        A0 = A if type == "double" else bc.as_integer(A, 3901)
        for what, j, pos in places:
            for tag, v in bc.SPECIALS[type]:
                want = bc.ExpectedCSC(bc.with_special(A0, j, pos, v)[0], B)
                assert want.not_finite and not np.isfinite(want.csc[2]).all(), (name, what, tag)


@pytest.mark.parametrize("name", bc.TALL)
def test_workspace_of_the_tall_shapes_holds_the_layout_of_the_header(panel, name):
    from sparsearray_amd._hip import load_library
    from sparsearray_amd.svt import REALSXP
    lib = load_library()

    class Csc(ctypes.Structure):
        _fields_ = [("Rtype", ctypes.c_int32), ("owned", ctypes.c_int32), ("nrow", ctypes.c_int64), ("ncol", ctypes.c_int64),
                    ("nnz", ctypes.c_int64), ("col_ptr", ctypes.c_void_p), ("row_idx", ctypes.c_void_p), ("val", ctypes.c_void_p),
                    ("na_background", ctypes.c_int32)]

    c = bc.case(panel, name)
    nrow, ninner = c.A.shape
    need = lib.svt_dev_spgemm_ws_bytes(ctypes.byref(Csc(REALSXP, 0, nrow, ninner, c.A.nnz, None, None, None, 0)), 3)
    npan = (nrow + panel - 1) // panel
    least = bc.ws_least(panel, nrow, ninner, 3)
    assert least == 256 + -(-(npan + 1) * ninner * 4 // 256) * 256 + -(-(3 * npan + 1) * 8 // 256) * 256
    assert need >= least, (need, least)


# ---------------------------------------------------------------------------
# B.6 integers near 2^31
# ---------------------------------------------------------------------------
def _descending(A, B):
    """the same products added in DESCENDING order of j"""
    Ad, Bd = ac.as_double(A.dense), ac.as_double(B.dense)
    acc = np.zeros((A.shape[0], B.shape[1]))
    for k in range(B.shape[1]):
        for j in np.flatnonzero(B.stored[:, k])[::-1]:
            rows = np.flatnonzero(A.stored[:, j])
            acc[rows, k] += Ad[rows, j] * Bd[j, k]
    return acc


@pytest.mark.parametrize("ta,tb", bc.LARGE_TYPES)
def test_large_integer_cases_tell_the_rule_from_its_neighbours(panel, ta, tb):
    P, c = panel, bc.case(panel, f"large_integers_{ta}_x_{tb}")
    assert (c.A.type, c.B.type) == (ta, tb)
    for op in (c.A, c.B):
        assert set(np.unique(op.dense[op.stored]).astype(np.int64).tolist()) <= set(bc.LARGE)
    assert (c.B.dense[:, 0] == bc.INT_MAX).all() and c.B.stored[:, 0].all()
    assert {int(abs(v)) for v in c.A.dense[c.A.stored]} == {abs(v) for v in bc.LARGE}
    met = c.A.stored.astype(int) @ c.B.stored.astype(int)
    assert (met >= 3).sum() > 100 and met[P - 1].min() >= 3 and met[P].min() >= 3
    want = gc.expect(c.A, c.B)
    assert not want.not_finite and np.abs(want.dense).max() > 2.0 ** 53
    # the order shows: at least one cell differs from the same products added in descending j
    other = _descending(c.A, c.B)
    assert (bits(other) != bits(want.dense)).any()
    # a product formed in int32 before widening is another number; a sum kept in int64 rounds elsewhere (or wraps)
    a, b = c.A.dense.astype(np.int64), c.B.dense.astype(np.int64)
    exact = a.astype(object) @ b.astype(object)
    assert max(abs(int(v)) for v in exact.ravel()) >= 2 ** 63
    as_double = np.array([[float(v) for v in row] for row in exact])
    assert (as_double != want.dense).any()                                      # the sums round on the way: not the exact sum rounded once
    wrapped = (a[:, :, None] * b[None, :, :]).astype(np.int32).astype(np.float64).sum(axis=1)
    assert (wrapped != want.dense).any()


# ---------------------------------------------------------------------------
# C. the yardstick for the expectation itself
# ---------------------------------------------------------------------------
def _sub_block(A, B, k):
    """column k of B and the leaves of A it refers to: the same cells of result column k"""
    js = np.flatnonzero(B.stored[:, k])
    return gc.Op(A.dense[:, js], A.stored[:, js]), gc.Op(B.dense[js][:, [k]], B.stored[js][:, [k]])


@pytest.mark.parametrize("name", bc.FINITE_SMALL)
def test_expect_is_within_gamma_n_M_of_the_exact_product(panel, name):
    """|expect - E| <= gamma(n) M per cell with n >= 1, exactly 0 where n == 0 (exact_products.py; no slack factor)"""
    c = bc.case(panel, name)
    A, B = c.A, c.B
    if name == "split2":                        # the exact form of the whole is large: one column of B, and its leaves of A
        A, B = _sub_block(c.A, c.B, 2)
        assert np.array_equal(bits(gc.expect(A, B).dense[:, 0]), bits(gc.expect(c.A, c.B).dense[:, 2]))
    want = gc.expect(A, B)
    assert not want.not_finite
    p = ep.exact_matmul_sparse(A.shape[0], A.csc, B.csc)
    v = ep.check_product(want.dense, p, name)
    assert v.ncompared == int((p.n > 0).sum()) > 0
    v.require()
