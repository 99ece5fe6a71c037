"""x[i, j] by an N-index without a GPU: the host statement of the rule in oracle/rules.py (Session.subset on the
oracle session, whose dispatcher has it as its subsetting entry) against numpy on the dense matrix,
``dense[np.ix_(i, j)]``, at tolerance 0 (values and the mask of stored entries, as bits; tests/subset_cases.py), and the
argument checks, which run before dispatch and are the same for every session.

An operand with three dimensions: the host statement raises SparseArrayError ("2D objects only"); the library path
answers "not supported here", SparseArrayUnsupported (tests/test_hip_subset.py)."""
import numpy as np
import pytest

import subset_cases as sc
from sparsearray_amd import NA_integer, SparseArrayError, SVT_SparseArray
from sparsearray_amd.api import Session


@pytest.mark.parametrize("name", sc.NAMES)
def test_host_statement_against_the_dense_rule(oracle, name):
    _, op, i, j = sc.BY_NAME[name]
    x, _, _ = sc.operand(op)
    sc.check(oracle.subset(x, i, j), name)


def test_case_list_covers_what_it_names():
    ops = {c[1] for c in sc.CASES}
    assert ops == set(sc._OPERANDS)
    x, dense, stored = sc.operand("double_specials")
    b = sc.bits(dense[stored])
    for v in sc.bits(sc.SPECIALS_F64):                   # NA_real_, the NaNs, +-Inf, -0.0 and a stored 0.0 are all stored
        assert (b == v).any()
    assert sc.operand("all_zero")[0].svt_is_null and sc.operand("na_double")[0].na_background
    assert any(lf is not None and lf[1] is None for lf in sc.operand("logical")[0].leaves)
    assert (sc.bits(sc.operand("integer_specials")[1]) == sc.bits(np.array([NA_integer]))[0]).any()


def test_a_subscript_accepts_any_integer_valued_array_like(oracle):
    x, _, _ = sc.operand("double")
    want = oracle.subset(x, [3, 1, 3], [2, 2])
    for i, j in (((3, 1, 3), (2, 2)), (np.array([3.0, 1.0, 3.0]), np.array([2, 2], dtype=np.int64)),
                 (np.array([3, 1, 3], dtype=np.int32), [2.0, 2.0])):
        sc.same_object(oracle.subset(x, i, j), want)
    sc.same_object(oracle.subset(x), oracle.subset(x, None, None))
    sc.check(oracle.subset(x), "neither")


def test_dimnames_follow_the_subscripts(oracle):
    x0, _, _ = sc.operand("double")
    x = SVT_SparseArray(x0.dim, x0.type, x0.leaves, dimnames=[[f"r{k}" for k in range(37)], None])
    res = oracle.subset(x, [37, 1, 1], [5])
    assert res.dimnames == [["r36", "r0", "r0"], None]


@pytest.mark.parametrize("args,match", [
    (([1.5], None), "integer-valued"),
    ((None, ["a"]), "integer vectors"),
    ((None, "12"), "integer vectors"),
    (([True, False], None), "integer vectors"),
    (([[1, 2], [3, 4]], None), "integer vectors"),
    (([1, float("nan")], None), "NAs"),
    ((None, np.array([1, NA_integer], dtype=np.int32)), "NAs"),
    (([0], None), "out of bounds"),
    (([38], None), "out of bounds"),
    ((None, [24]), "out of bounds"),
    ((None, [-1]), "out of bounds"),
    (([1], [1], [1]), "number of subscripts"),
])
def test_argument_errors(oracle, args, match):
    x, _, _ = sc.operand("double")
    with pytest.raises(SparseArrayError, match=match):
        oracle.subset(x, *args)


def test_argument_checks_run_before_dispatch():
    """the same errors from a session whose dispatcher claims the library entry: it is never reached"""
    class Claims:
        def has_entry(self, name):
            return True

        def __call__(self, name, *args):
            raise AssertionError(f"{name} was dispatched")

    x, _, _ = sc.operand("double")
    s = Session(Claims())
    for args in (([1.5], None), ([0], None), (None, [24]), ([1, float("nan")], None), ([1], [1], [1]), (None, "12")):
        with pytest.raises(SparseArrayError):
            s.subset(x, *args)


def test_three_dimensions(oracle):
    x = SVT_SparseArray.from_dense(np.arange(24, dtype=np.float64).reshape(2, 3, 4))
    with pytest.raises(SparseArrayError, match="2D objects"):
        oracle.subset(x, [1], [1], [1])
    with pytest.raises(SparseArrayError, match="number of subscripts"):
        oracle.subset(x, [1], [1])
