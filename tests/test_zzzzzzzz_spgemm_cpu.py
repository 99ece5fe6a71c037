"""The sparse x sparse products with a sparse result, without a GPU: the case builder of tests/spgemm_cases.py proved
against plain numpy, and the checks of Session.matmul_sparse / crossprod_sparse / tcrossprod_sparse against a
dispatcher that records its calls."""
import numpy as np
import pytest

import spgemm_cases as gc
from sparsearray_amd import SVT_SparseArray
from sparsearray_amd.api import Session, SparseArrayError, SparseArrayUnsupported


@pytest.fixture(scope="module")
def panel():
    from sparsearray_amd.device import spgemm_panel
    return spgemm_panel(10 ** 6)


# ---------------------------------------------------------------------------
# the case builder's own proofs
# ---------------------------------------------------------------------------
def test_the_library_answers_one_of_the_panel_heights_the_cases_are_built_for(panel):
    from sparsearray_amd.device import spgemm_panel
    assert panel in gc.PANELS
    assert {spgemm_panel(n) for n in (0, 1, panel - 1, panel + 1, 10 ** 9)} <= set(gc.PANELS)


@pytest.mark.parametrize("name", gc.INTEGER_VALUED)
def test_expect_is_the_matrix_product_on_integer_valued_operands(panel, name):
    c = gc.device_cases(panel)[name]
    want = c.want
    exact = c.A.dense.astype(np.int64) @ c.B.dense.astype(np.int64)
    assert np.abs(exact).max() < 2 ** 53 and np.array_equal(want.dense, exact.astype(np.float64))
    assert np.array_equal(want.stored, exact != 0) and not want.not_finite
    assert want.stored.any() and not want.stored.all()


def test_expect_on_a_literal_case():
    A = gc.Op.of(3, 2, [0, 2, 1, 2], [0, 0, 1, 1], [2.0, 3.0, 5.0, -3.0])
    B = gc.Op.of(2, 2, [0, 1, 1], [0, 0, 1], [1.0, 1.0, 0.0])
    want = gc.expect(A, B)
    assert np.array_equal(want.dense, [[2.0, 0.0], [5.0, 0.0], [0.0, 0.0]])           # row 2, column 0: 3 - 3
    assert np.array_equal(want.stored, [[True, False], [True, False], [False, False]])  # column 1: reached, 5 * 0 and -3 * 0
    cp, ri, vv = want.csc
    assert cp.tolist() == [0, 2, 2] and ri.tolist() == [0, 1] and vv.tolist() == [2.0, 5.0]


def test_the_order_case_tells_the_orders_apart(panel):
    c = gc.device_cases(panel)["order_matters"]
    d = c.want.dense
    assert d[5, 0] == 0.0 and d[6, 0] == 1.0 and not c.want.stored[5, 0] and c.want.stored[6, 0]
    # the same products of row 5 added in the other order give the other answer
    assert (1e16 + -1e16) + 1.0 == 1.0 and (1e16 + 1.0) + -1e16 == 0.0
    # descending j would store row 5 and keep row 6 at (1.0 - 1e16) + 1e16 == 0.0: the case tells that order apart too
    assert (-1e16 + 1.0) + 1e16 == 0.0 and (1.0 + -1e16) + 1e16 == 0.0


@pytest.mark.parametrize("P", gc.PANELS)
def test_boundary_cases_have_entries_on_both_sides_of_a_panel_edge(P):
    cases = gc.device_cases(P)
    for name in gc.BOUNDARY:
        assert gc.straddles(cases[name], P), name
    c = cases["nrow_2P+3"]
    assert c.edges == (P, 2 * P) and c.A.shape[0] == 2 * P + 3 and c.want.stored[2 * P + 2].any()
    for name, nrow in (("nrow_P-1", P - 1), ("nrow_P", P)):
        assert cases[name].A.shape[0] == nrow and cases[name].want.stored[nrow - 1].any() and cases[name].want.stored[0].any()
    # a run that ends exactly at the edge, one that starts there, one that crosses it
    A = cases["runs_at_a_panel_edge"].A
    assert [np.flatnonzero(A.stored[:, j])[[0, -1]].tolist() for j in range(3)] == [[P - 5, P - 1], [P, P + 4], [P - 2, P + 2]]


def test_cases_are_what_their_names_say(panel):
    cases = gc.device_cases(panel)
    c = cases["one_column_receives_everything"]
    assert c.B.shape[1] == 1 and c.B.stored.all() and c.want.stored.sum() > panel
    c = cases["100000_empty_columns"]
    assert c.B.shape[1] == 100_003 and (c.B.stored.any(axis=0)).sum() == 5 and c.want.stored.any()
    c = cases["empty_leaves_referred_to"]
    empty = np.flatnonzero(~c.A.stored.any(axis=0))
    assert empty.tolist() == [2, 4] and c.B.stored[empty].any(axis=1).all()
    assert not c.want.stored[:, 0].any() and c.want.stored[:, 1].any()                # column 0 refers to empty leaves only
    for name in ("empty_A", "empty_B", "empty_both", "K_0", "n_0", "nrow_0"):
        assert not cases[name].want.stored.any() and not cases[name].want.not_finite
    assert cases["K_0"].want.dense.shape[1] == 0 and cases["n_0"].A.shape[1] == 0 and cases["nrow_0"].want.dense.shape[0] == 0
    c = cases["every_cell_cancels"]
    assert c.want.csc[0].tolist() == [0, 0] and c.A.nnz == 600
    c = cases["stored_zeros"]
    assert (c.A.dense[c.A.stored] == 0).any() and (c.B.dense[c.B.stored] == 0).any()
    assert not c.want.stored[:, 1].any() and c.want.stored[:, 0].sum() == 3            # rows 2, 3 and P of column 0
    c = cases["minus_zero_and_subnormal"]
    kept = c.want.dense[c.want.stored]
    assert not c.want.stored[:, 0].any() and (np.abs(kept) < 2.2250738585072014e-308).sum() == 2 and not (kept == 0).any()
    for name, c in cases.items():
        special = any(name.startswith(p) for p in ("NA_", "NaN_", "plus_Inf", "minus_Inf", "Inf_in_B"))
        assert c.want.not_finite == special, name
        if name.endswith("in_a_leaf_nobody_refers_to"):
            assert np.isfinite(c.want.dense).all() and c.want.stored.any(), name       # the special takes part in no pair
        if name.endswith("read_by_a_pair"):
            assert not np.isfinite(c.want.dense[c.want.stored]).all(), name
    assert np.isfinite(cases["Inf_in_B_against_an_empty_leaf"].want.dense).all()
    assert sum(n.startswith("random_") for n in cases) == gc.RANDOM_SHAPES
    assert {cases[f"random_{s:02d}"].A.type for s in range(gc.RANDOM_SHAPES)} == {"double", "integer"}


def test_random_values_do_not_cancel_by_accident(panel):
    """every reached cell of the random family is stored: a dropped cell there would be a cancellation nobody planned"""
    cases = gc.device_cases(panel)
    for s in range(gc.RANDOM_SHAPES):
        c = cases[f"random_{s:02d}"]
        A, B = c.A.stored.astype(np.int64), c.B.stored.astype(np.int64)
        assert np.array_equal(c.want.stored, (A @ B) > 0), s


# ---------------------------------------------------------------------------
# Session.matmul_sparse / crossprod_sparse / tcrossprod_sparse: the checks in their order, then one call
# ---------------------------------------------------------------------------
class Recorder:
    def __init__(self, answer=None):
        self.calls, self.answer = [], answer

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        return self.answer(*args) if callable(self.answer) else self.answer


def _typed(type_, dim, dimnames=None, na_background=False):
    x = SVT_SparseArray(dim, "double", [None] * int(np.prod(dim[1:])), dimnames=dimnames, na_background=na_background)
    x.type = type_
    return x


def _answer(x, y, tr_x, tr_y):
    return _typed("double", (x.dim[1 if tr_x else 0], y.dim[0 if tr_y else 1])), False


def test_the_three_methods_make_one_call_with_their_flags():
    x, y, z, w = _typed("double", (41, 29)), _typed("integer", (29, 17)), _typed("double", (41, 13)), _typed("integer", (23, 29))
    for method, args, want in (("matmul_sparse", (x, y), (x, y, False, False)), ("crossprod_sparse", (x, z), (x, z, True, False)),
                               ("crossprod_sparse", (x,), (x, x, True, False)), ("tcrossprod_sparse", (x, w), (x, w, False, True)),
                               ("tcrossprod_sparse", (x,), (x, x, False, True))):
        rec = Recorder(_answer)
        out = getattr(Session(rec), method)(*args)
        assert rec.calls == [("C_matmul_SVT_SVT_sparse",) + want], method
        assert out.type == "double" and out.dimnames is None
        assert out.dim == {"matmul_sparse": (41, want[1].dim[1]), "crossprod_sparse": (29, want[1].dim[1]),
                           "tcrossprod_sparse": (41, want[1].dim[0])}[method]
        # integer and double operands went over with their own types
        assert [a.type for a in rec.calls[0][1:3]] == [a.type for a in want[:2]]


def test_a_logical_operand_is_coerced_to_the_common_type():
    x, l = _typed("double", (41, 29)), SVT_SparseArray((29, 17), "logical", [None] * 17)
    rec = Recorder(_answer)
    Session(rec).matmul_sparse(x, l)
    assert [a.type for a in rec.calls[0][1:3]] == ["double", "double"]
    with pytest.raises(SparseArrayError, match='must be of type\\(\\) "double" or "integer"'):
        Session(rec).matmul_sparse(SVT_SparseArray((41, 29), "logical", [None] * 29), l)


def test_dimnames_of_the_three_methods():
    rn, cn = gc.names("r", 41), gc.names("c", 29)
    x = _typed("double", (41, 29), [rn, cn])
    y = _typed("double", (29, 17), [gc.names("yr", 29), gc.names("yc", 17)])
    z = _typed("double", (41, 13), [None, gc.names("zc", 13)])
    w = _typed("double", (23, 29), [gc.names("wr", 23), None])
    plain = _typed("double", (29, 17))
    s = Session(Recorder(_answer))
    assert s.matmul_sparse(x, y).dimnames == [rn, y.dimnames[1]]
    assert s.matmul_sparse(x, plain).dimnames == [rn, None]
    assert s.matmul_sparse(_typed("double", (41, 29), [None, cn]), plain).dimnames is None       # the NULL simplification
    assert s.crossprod_sparse(x, z).dimnames == [cn, z.dimnames[1]]
    assert s.crossprod_sparse(x).dimnames == [cn, cn]
    assert s.crossprod_sparse(z, _typed("double", (41, 5))).dimnames == [z.dimnames[1], None]
    assert s.tcrossprod_sparse(x, w).dimnames == [rn, w.dimnames[0]]
    assert s.tcrossprod_sparse(x).dimnames == [rn, rn]
    assert s.tcrossprod_sparse(z, z).dimnames is None


def test_every_refusal_comes_before_any_call():
    rec = Recorder(_answer)
    s = Session(rec)
    x, y = _typed("double", (41, 29)), _typed("double", (29, 17))
    na = _typed("double", (29, 17), na_background=True)
    for method, what in (("matmul_sparse", "%\\*%"), ("crossprod_sparse", "crossprod"), ("tcrossprod_sparse", "tcrossprod")):
        with pytest.raises(SparseArrayError, match=f"unable to find an inherited method for function '{what}'"):
            getattr(s, method)(x, na)
        with pytest.raises(SparseArrayError, match="unable to find an inherited method"):
            getattr(s, method)(na, y)
        with pytest.raises(SparseArrayError, match="input objects must have 2 dimensions"):
            getattr(s, method)(x, _typed("double", (29, 17, 1)))
        with pytest.raises(SparseArrayError, match="input objects must have 2 dimensions"):
            getattr(s, method)(_typed("double", (41,)), y)
        with pytest.raises(SparseArrayError, match="needs two SVT_SparseArray objects"):
            getattr(s, method)(x, np.ones((29, 17)))
        with pytest.raises(SparseArrayError, match="needs two SVT_SparseArray objects"):
            getattr(s, method)(np.ones((41, 29)), y)
    with pytest.raises(SparseArrayError, match="non-conformable arguments"):
        s.matmul_sparse(x, _typed("double", (28, 17)))
    with pytest.raises(SparseArrayError, match="non-conformable arguments"):
        s.crossprod_sparse(x, _typed("double", (40, 13)))
    with pytest.raises(SparseArrayError, match="non-conformable arguments"):
        s.tcrossprod_sparse(x, _typed("double", (23, 28)))
    for bad in ("character", "raw", "complex", "logical"):
        with pytest.raises(SparseArrayError, match='input objects must be of type\\(\\) "double" or "integer"'):
            s.matmul_sparse(_typed(bad, (41, 29)), _typed(bad, (29, 17)))
    for bad in ("character", "raw", "complex"):
        with pytest.raises(SparseArrayError, match='input objects must be of type\\(\\) "double" or "integer"'):
            s.crossprod_sparse(_typed(bad, (41, 29)))
    assert rec.calls == []


def test_not_finite_raises_unsupported_and_names_the_function():
    x, y = _typed("double", (41, 29)), _typed("double", (29, 17))
    for method, args in (("matmul_sparse", (x, y)), ("crossprod_sparse", (x,)), ("tcrossprod_sparse", (x,))):
        rec = Recorder(lambda a, b, tr_x, tr_y: (_answer(a, b, tr_x, tr_y)[0], True))
        with pytest.raises(SparseArrayUnsupported) as e:
            getattr(Session(rec), method)(*args)
        msg = str(e.value)
        assert msg.startswith(f"{method}()") and "non-finite or NA values" in msg and "matmul()" in msg and "crossprod()" in msg
        assert len(rec.calls) == 1


def test_a_session_on_the_oracle_says_not_offered(oracle):
    x = gc.host_operand("x").svt()
    for call in (lambda s: s.matmul_sparse(x, gc.host_operand("y").svt()), lambda s: s.crossprod_sparse(x),
                 lambda s: s.tcrossprod_sparse(x)):
        with pytest.raises(SparseArrayUnsupported, match="C_matmul_SVT_SVT_sparse is not offered by this session's library"):
            call(oracle)


def test_workspace_query_needs_no_gpu_and_grows_with_the_items(panel):
    """svt_dev_spgemm_ws_bytes: head + table of run bounds + one int64 per (column, panel) item + the scan's scratch"""
    import ctypes
    from sparsearray_amd._hip import load_library
    from sparsearray_amd.svt import REALSXP
    lib = load_library()

    class Csc(ctypes.Structure):
        _fields_ = [("Rtype", ctypes.c_int32), ("owned", ctypes.c_int32), ("nrow", ctypes.c_int64), ("ncol", ctypes.c_int64),
                    ("nnz", ctypes.c_int64), ("col_ptr", ctypes.c_void_p), ("row_idx", ctypes.c_void_p), ("val", ctypes.c_void_p),
                    ("na_background", ctypes.c_int32)]

    def need(nrow, n, K):
        return lib.svt_dev_spgemm_ws_bytes(ctypes.byref(Csc(REALSXP, 0, nrow, n, 0, None, None, None, 0)), K)

    npan = 3                                                            # 2 P + 3 rows
    least = 256 + 10 * (npan + 1) * 4 + (7 * npan + 1) * 8
    assert need(2 * panel + 3, 10, 7) >= least and need(2 * panel + 3, 10, 7) % 256 == 0
    assert need(2 * panel + 3, 10, 100_000) >= need(2 * panel + 3, 10, 7) + (100_000 - 7) * npan * 8
    assert need(64 * panel, 1000, 7) >= need(2 * panel + 3, 1000, 7) + 1000 * (64 - npan) * 4
    assert need(0, 0, 0) >= 256 + 8
