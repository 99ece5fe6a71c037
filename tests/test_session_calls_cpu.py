"""Which ``.Call`` entry points ``Session`` issues, and that it computes nothing itself, without a GPU.

Session runs over a recording dispatcher around the CPU oracle's (tests/session_calls_cases.py), told to deny
C_rowStatsFull_SVT, to claim and refuse it, or to claim and answer it.  Every result is compared with what the Session of
commit 6957427 returned for the same call (tests/golden/session_calls.json, written by tests/golden/make_session_calls.py
on that commit): values with NaN equal to NaN, dtype and memory order.

ROW_ROUTES is the route table of DESIGN.md, "Row statistics in one call", written down from that commit.  S, C, F, T:
C_rowStats_SVT, C_colStats_SVT, C_rowStatsFull_SVT, C_transpose_2D_SVT (C_aperm_SVT for more than two dimensions);
NO: SparseArrayError, "unable to find an inherited method", before any call."""
import json
import os

import pytest

import session_calls_cases as sc
import sparsearray_amd.api as api
from sparsearray_amd.api import Session

S, C, F, T, A, NO = "C_rowStats_SVT", "C_colStats_SVT", sc.FULL, "C_transpose_2D_SVT", "C_aperm_SVT", None
#   the library has C_rowStatsFull_SVT:   no   no   yes, answers   yes, refuses       (dims = 0: whichever)
#                               dims:    > 0   0    > 0            > 0
_BASE = {"plain": ([S], [C], [S], [S]), "NaArray": ([S], [C], [S], [S])}
_OLD = {"plain": ([T, C], [C], [F], [F, T, C]), "NaArray": (NO, [C], NO, NO)}
ROW_ROUTES = {   # na.rm = FALSE, no center
    "rowAnyNAs": _BASE, "rowCountNAs": _BASE, "rowMins": _BASE, "rowMaxs": _BASE, "rowSums": _BASE,
    "rowAnys": _OLD, "rowAlls": _OLD, "rowProds": _OLD,
    "rowRanges": {"plain": ([S, S], [C, C], [F], [F, S, S]), "NaArray": ([S, S], [C, C], [F], [F, S, S])},
    "rowMeans": {"plain": ([S], [C], [F], [F, S]), "NaArray": (NO, [C], NO, NO)},
    "rowVars": {"plain": ([S, S], [C, C], [F], [F, S, S]), "NaArray": (NO, [C], NO, NO)},
    "rowSds": {"plain": ([S, S], [C, C], [F], [F, S, S]), "NaArray": (NO, [C], NO, NO)},
}
# na.rm = TRUE: the composition counts the NAs first (one more call in front of it); a given center saves the row sums
ROW_ROUTES_NA_RM = {
    "rowMeans": {"plain": ([S, S], [C, C], [F], [F, S, S]), "NaArray": (NO, [C], NO, NO)},
    "rowVars": {"plain": ([S, S, S], [C, C, C], [F], [F, S, S, S]), "NaArray": (NO, [C], NO, NO)},
    "rowSds": {"plain": ([S, S, S], [C, C, C], [F], [F, S, S, S]), "NaArray": (NO, [C], NO, NO)},
}
ROW_ROUTES_CENTER = {"no": [S], "refuse": [F, S]}


def expected_route(method, key, kw, full):
    if "center" in kw:
        return ROW_ROUTES_CENTER[full]
    table = ROW_ROUTES_NA_RM if kw.get("na_rm") else ROW_ROUTES
    row = table[method]["NaArray" if key.endswith("NA") else "plain"]
    route = row[1] if kw["dims"] == 0 else row[("no", None, "answer", "refuse").index(full)]
    return route if key != "X3" or route is NO else [A if name == T else name for name in route]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "session_calls.json")) as f:
        return json.load(f)["results"]


@pytest.fixture(scope="module")
def ops():
    return sc.operands()


def test_operands_are_what_the_cases_need(ops):
    x = ops["X"]
    assert x.dim == (5, 4) and x.leaves[2] is None and 0.0 in x.leaves[1][1] and api.is_NA_real(x.leaves[0][1]).any()
    assert not any(lf is not None and 4 in lf[0] for lf in x.leaves)                # the empty row
    assert ops["XI"].type == "integer" and (ops["XI"].leaves[0][1] == api.NA_integer).any()
    assert ops["X3"].dim == (2, 3, 2) and ops["XNA"].na_background and ops["XINA"].na_background


def test_order_statistics_and_subset_issue_one_call(oracle, ops, golden):
    for cid, m, key, args, kw in sc.order_cases():
        res, calls = sc.run(oracle, ops, m, key, args, kw)
        want = sc.ZERO_EXTENT_CALLS[(m, key)] if key.startswith("Z") else [sc.entry_of(m)]
        assert calls == want, (cid, calls)
        sc.assert_same(res, golden[cid], cid)


def test_row_statistics_take_the_routes_of_the_table(oracle, ops, golden):
    cases = sc.row_cases()
    assert {m for _, m, *_ in cases} == set(ROW_ROUTES) == set(sc.ROW_METHODS)
    for cid, m, key, kw, full in cases:
        res, calls = sc.run(oracle, ops, m, key, (), kw, full)
        want = expected_route(m, key, kw, full)
        if want is NO:
            assert calls == [] and isinstance(res, api.SparseArrayError) and "inherited method" in str(res), cid
        else:
            assert calls == want, (cid, calls, want)
        sc.assert_same(res, golden[cid], cid)


def test_session_holds_no_host_statement_of_a_rule():
    assert not [n for n in dir(Session) if n.startswith("_leaf_")]
    with open(api.__file__) as f:
        src = f.read()
    assert "oracle" not in src.lower()
    assert src.count("has_entry") == 1                   # Session._has, the one query of the dispatcher
