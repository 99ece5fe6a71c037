"""Compare / Logic without a GPU: the R-level checks of Session.compare / logic / logical_not and their messages
(R/SparseArray-Compare-methods.R, R/SparseArray-Logic-methods.R), the ``__host__`` side of the two element rules
(sparsearray_amd/csrc/svt_arith_rules.h, through tests/compare_rules_main.cpp) against the expectations of
tests/compare_cases.py, and the case builder's proofs of its placements under the new rules."""
import os
import subprocess

import numpy as np
import pytest

import arith_cases as ac
import compare_cases as cc
from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.api import COMPARE_OPCODES, LOGIC_OPCODES, Session
from test_arith_cpu import TABLE_F64, NoCall, _hex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
NA = int(NA_integer)


# ---------------------------------------------------------------------------
# the host side of the two rules
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/compare_rules_main.cpp, built with the host compiler like tests/arith_rules_main.cpp"""
    exe = tmp_path_factory.mktemp("compare_rules") / "compare_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", str(exe),
                    os.path.join(ROOT, "tests", "compare_rules_main.cpp"), "-lm"], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return [int(s) for s in out.stdout.split("\n")[:-1]]
    return ask


def test_opcodes_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    for name, code in (("EQ", 1), ("NE", 2), ("LE", 3), ("GE", 4), ("LT", 5), ("GT", 6)):
        assert f"SVT_COMPARE_{name} = {code}" in text
    assert "SVT_LOGIC_AND = 1" in text and "SVT_LOGIC_OR = 2" in text
    assert COMPARE_OPCODES == {"==": 1, "!=": 2, "<=": 3, ">=": 4, "<": 5, ">": 6} and LOGIC_OPCODES == {"&": 1, "|": 2}


def test_host_compare_rule_agrees_with_the_case_module(rules):
    """every pair of the specials table of tests/test_arith_cpu.py (NA, NaNs, +-Inf, +-0, ordinary values) under the six
    operators"""
    x, y = [a.reshape(-1) for a in np.meshgrid(TABLE_F64, TABLE_F64, indexing="ij")]
    # integers through as.double(): the one rule in double against the comparison done on integers
    vals = np.array([NA, 0, 1, -1, 7, -7, INT_MAX, -INT_MAX, INT_MAX - 1], dtype=np.int64)
    a, b = [v.reshape(-1) for v in np.meshgrid(vals, vals, indexing="ij")]
    for op in COMPARE_OPCODES:
        got = rules([f"C {COMPARE_OPCODES[op]} {p} {q}" for p, q in zip(_hex(x), _hex(y))])
        assert got == cc.compare_values(op, x, y).tolist(), op
        got = rules([f"J {COMPARE_OPCODES[op]} {p} {q}" for p, q in zip(a, b)])
        want = np.where((a == NA) | (b == NA), NA, cc.COMPARE_OPS[op](a, b).astype(np.int64))
        assert got == want.tolist(), op
        assert got == cc.compare_values(op, a.astype(np.int32), b.astype(np.int32)).tolist(), op


def test_host_logic_rule_is_the_three_valued_table(rules):
    vals = [1, 0, NA]
    got = rules([f"L {code} {x} {y}" for code in (1, 2) for x in vals for y in vals])
    #                x:  TRUE         FALSE      NA         (y: TRUE, FALSE, NA)
    assert got[:9] == [1, 0, NA,   0, 0, 0,   NA, 0, NA]                     # &
    assert got[9:] == [1, 1, 1,    1, 0, NA,  1, NA, NA]                     # |
    x, y = [np.array(v, dtype=np.int32).reshape(-1) for v in np.meshgrid(vals, vals, indexing="ij")]
    assert got[:9] == cc.logic_values("&", x, y).tolist() and got[9:] == cc.logic_values("|", x, y).tolist()


def test_literal_pins(rules):
    na, inf = _hex(NA_real)[0], _hex(np.inf)[0]
    h = lambda v: _hex(v)[0]                                                         # noqa: E731
    gt, lt = COMPARE_OPCODES[">"], COMPARE_OPCODES["<"]
    assert rules([f"C {gt} {na} {h(0.0)}", f"C {lt} {h(-0.0)} {h(0.0)}", f"C {gt} {inf} {h(1e308)}",
                  f"J {gt} {INT_MAX} {INT_MAX - 1}", f"L 1 {NA} 0", f"L 2 {NA} 1", f"J {gt} {NA} 0",
                  f"C {COMPARE_OPCODES['==']} {h(-0.0)} {h(0.0)}", f"C {COMPARE_OPCODES['!=']} {h(np.nan)} {h(np.nan)}"]) == \
        [NA, 0, 1, 1, 0, 1, NA, 1, NA]


# ---------------------------------------------------------------------------
# the Session's checks: raised before any call
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checks():
    return Session(NoCall())


def _when(op, when):
    return f"x {op} y: operation not supported on SparseArray object x when {when} (result wouldn't be sparse)"


COMPARE_CHECKS = [
    # (op, e1, e2, message)
    (">", "d1", [1.0, 2.0], "comparison operations are not supported between a SparseArray object and a vector of length != 1"),
    (">", "d1", [], "vector of length != 1"),
    (">", "d1", {"a": 1}, "comparison operations between SparseArray objects and list vectors are not supported"),
    ("<", "d1", 1j, "invalid comparison with complex values"),
    (">=", 2j, "d1", "invalid comparison with complex values"),
    (">", "d1", float("nan"), _when(">", "y is NA or NaN")),
    ("!=", "i1", NA, _when("!=", "y is NA or NaN")),
    ("==", NA_real, "d1", _when("==", "y is NA or NaN")),
    ("<=", "d1", True, _when("<=", "y is a logical or raw value")),
    ("<", "l1", False, _when("<", "y is a logical or raw value")),
    ("<", "d1", "a", _when("<", 'type(x) is "character" or y is a string')),
    ("==", "d1", 0, _when("==", "y is 0 or FALSE or the empty string")),
    ("==", "l1", False, _when("==", "y is 0 or FALSE or the empty string")),
    ("==", "d1", "", _when("==", "y is 0 or FALSE or the empty string")),
    ("!=", "d1", 2.0, _when("!=", "y is not 0, FALSE, or the empty string")),
    ("<=", "d1", 0.0, _when("<=", "y is >= 0")),
    ("<=", "i1", 3, _when("<=", "y is >= 0")),
    (">=", "d1", 0, _when(">=", "y is <= 0, or FALSE, or the empty string")),
    (">=", "d1", -1.5, _when(">=", "y is <= 0, or FALSE, or the empty string")),
    ("<", "d1", 1, _when("<", "y is > 0")),
    (">", "d1", -1, _when(">", "y is < 0")),
    ("<", -1, "d1", _when(">", "y is < 0")),                       # -1 < x is x > -1
    (">", 1, "d1", _when("<", "y is > 0")),                        # 1 > x is x < 1
    ("==", "d1", "a", "comparison operations are not implemented yet between SVT_SparseArray objects, or between an "
                      "SVT_SparseArray object and a single value, when one or the other is of type() \"character\""),
    ("==", "d1", "d2", '"==" is not supported between SparseArray objects (result wouldn\'t be sparse in general), but "!=" is'),
    ("<=", "i1", "d2", '"<=" is not supported between SparseArray objects (result wouldn\'t be sparse in general), but "<" is'),
    (">=", "l1", "l2", '">=" is not supported between SparseArray objects (result wouldn\'t be sparse in general), but ">" is'),
    ("!=", "d1", "d_ncol0", "non-conformable arrays"),
    (">", "d3d", "d1", "non-conformable arrays"),
    ("<>", "d1", "d2", 'invalid Compare operation "<>"'),
    ("+", "d1", 1.0, 'invalid Compare operation "+"'),
]


def _arg(a):
    return cc.operand(a) if isinstance(a, str) and (a in cc._OPERANDS or a in ac._OPERANDS) else a


def test_compare_checks_raise_the_reference_messages(checks):
    for op, e1, e2, msg in COMPARE_CHECKS:
        with pytest.raises(SparseArrayError) as e:
            checks.compare(op, _arg(e1), _arg(e2))
        assert msg in str(e.value), (op, e1, e2, str(e.value))
        assert not isinstance(e.value, SparseArrayUnsupported), (op, e1, e2)


def test_what_the_reference_takes_and_this_library_does_not(checks):
    d = cc.operand("d1")
    for op in ("==", "!="):
        with pytest.raises(SparseArrayUnsupported, match="complex"):
            checks.compare(op, d, 1 + 2j if op == "==" else 0j)
    with pytest.raises(SparseArrayUnsupported, match="dense array"):
        checks.compare("!=", d, np.zeros(d.dim))
    with pytest.raises(SparseArrayUnsupported, match="dense array"):
        checks.logic("&", cc.operand("l1"), np.zeros(d.dim, bool))
    with pytest.raises(SparseArrayError, match="needs an SVT_SparseArray operand"):
        checks.compare(">", 1, 2)


LOGIC_CHECKS = [
    ("&", "d1", "l1", "'Logic' operation \"&\" and \"|\" not supported on SparseArray object of type() \"double\""),
    ("|", "l1", "i1", "'Logic' operation \"&\" and \"|\" not supported on SparseArray object of type() \"integer\""),
    ("&", "i1", True, "'Logic' operation \"&\" and \"|\" not supported on SparseArray object of type() \"integer\""),
    ("&", "l1", 1, '"&" between a SparseArray object and a integer vector is not supported'),
    ("|", "l1", 0.0, '"|" between a SparseArray object and a numeric vector is not supported'),
    ("&", "l1", [True, False], '"&" between a SparseArray object and a vector of length != 1 is not supported'),
    ("&", "l1", None, _when("&", "y is NA")),
    ("|", None, "l1", _when("|", "y is NA")),
    ("|", "l1", True, _when("|", "y is TRUE")),
    ("|", True, "l1", _when("|", "y is TRUE")),
    ("&", "l1", "l_3d", "non-conformable arrays"),
    ("&&", "l1", "l2", 'invalid Logic operation "&&"'),
]


def test_logic_checks_raise_the_reference_messages(checks):
    from sparsearray_amd import SVT_SparseArray
    for op, e1, e2, msg in LOGIC_CHECKS:
        if isinstance(e2, str) and e2 == "l_3d":
            e2 = SVT_SparseArray((3, 2, 2), "logical", [None] * 4)
        with pytest.raises(SparseArrayError) as e:
            checks.logic(op, _arg(e1), _arg(e2))
        assert msg in str(e.value), (op, e1, str(e.value))
        assert not isinstance(e.value, SparseArrayUnsupported), (op, e1)


def test_logical_not_and_the_arith_group_stay_as_they_are(checks):
    with pytest.raises(SparseArrayError) as e:
        checks.logical_not(cc.operand("l1"))
    assert str(e.value) == ("logical negation (\"!\") is not supported on SparseArray objects (result wouldn't be sparse in "
                            "general)")
    with pytest.raises(SparseArrayError, match="invalid Arith operation"):
        checks.arith("&", cc.operand("d1"), cc.operand("d1"))
    with pytest.raises(SparseArrayError, match="invalid Arith operation"):
        checks.arith(">", cc.operand("d1"), 0)


def test_checked_calls_reach_the_entry_point_flipped_and_coerced():
    """what passes the checks arrives as one call: a scalar on the left flips the operator, the scalar goes out as a
    double value with the bigger of the two types; Logic with a scalar makes no call at all"""
    seen = []

    class Recorder(NoCall):
        def __call__(self, name, *args):
            seen.append((name,) + args[1:])
            return "ans"

    s = Session(Recorder())
    d, i, l1, l2 = cc.operand("d1"), cc.operand("i1"), cc.operand("l1"), cc.operand("l2")
    assert s.compare("<", 3, i) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 3.0, "integer", ">")
    assert s.compare(">=", -2.5, d) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", -2.5, "double", "<=")
    assert s.compare("==", 3, d) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 3.0, "double", "==")
    assert s.compare("!=", 0, i) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 0.0, "integer", "!=")
    assert s.compare(">", i, 2.5) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 2.5, "double", ">")
    assert s.compare(">", i, 0) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 0.0, "integer", ">")
    assert s.compare(">", l1, False) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 0.0, "logical", ">")
    assert s.compare("==", l1, True) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 1.0, "logical", "==")
    assert s.compare(">=", l1, 1) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", 1.0, "integer", ">=")
    assert s.compare(">", d, float("inf")) == "ans" and seen.pop() == ("C_Compare_SVT1_v2", float("inf"), "double", ">")
    assert s.compare("!=", d, i) == "ans" and seen.pop() == ("C_Compare_SVT1_SVT2", i, "!=")
    assert s.compare("<", l1, d) == "ans" and seen.pop() == ("C_Compare_SVT1_SVT2", d, "<")
    assert s.logic("|", l1, l2) == "ans" and seen.pop() == ("C_Logic_SVT1_SVT2", l2, "|")
    assert not seen
    nocall = Session(NoCall())
    assert nocall.logic("&", l1, True) is l1 and nocall.logic("&", True, l1) is l1
    assert nocall.logic("|", l1, False) is l1 and nocall.logic("|", np.bool_(False), l1) is l1
    emptied = nocall.logic("&", l1, False)
    assert emptied.dim == l1.dim and emptied.type == "logical" and emptied.svt_is_null and emptied.nzcount() == 0
    assert not l1.svt_is_null


def test_the_oracle_session_does_not_offer_them(oracle):
    d, l1 = cc.operand("d1"), cc.operand("l1")
    for call in (lambda: oracle.compare(">", d, 0), lambda: oracle.compare("!=", d, d), lambda: oracle.logic("&", l1, l1)):
        with pytest.raises(SparseArrayUnsupported, match="not offered"):
            call()
    with pytest.raises(SparseArrayError, match="non-conformable arrays"):      # the checks come first there too
        oracle.compare("!=", d, cc.operand("d_ncol0"))
    with pytest.raises(SparseArrayError, match="y is 0 or FALSE"):
        oracle.compare("==", d, 0)
    assert oracle.logic("&", l1, True) is l1                                   # no call: nothing to offer


# ---------------------------------------------------------------------------
# the case builder proves its own placements under the new rules
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    from sparsearray_amd.device import arith_tile
    return arith_tile()


def test_straddling_pairs_with_equal_values_are_false_under_ne(T):
    """the pairs sit across the tile boundaries (tests/test_arith_cpu.py proves the places); with equal values `!=` is
    FALSE there and the two positions leave the result, with other values they stay"""
    c = ac.device_cases(T)["straddling_pairs_cancel"]
    kx, vx, ky, vy = cc.device_operands(c, "double")
    assert np.array_equal(vx[np.searchsorted(kx, ky)], vy)
    cp, ri, v = cc.device_expect("compare", "!=", kx, vx, ky, vy, c.nrow, c.ncol)
    assert cp[-1] == kx.size - 2 and np.all(v == 1)
    assert not np.isin(ky, ri.astype(np.int64) + np.repeat(np.arange(c.ncol), np.diff(cp)) * c.nrow).any()
    c2 = ac.device_cases(T)["straddling_pairs_columns"]
    assert cc.device_expect("compare", "!=", *cc.device_operands(c2, "double"), c2.nrow, c2.ncol)[0][-1] == c2.kx.size
    # the same holds for the values rounded to integers, on either side
    for values in ("integer", "mixed"):
        assert cc.device_expect("compare", "!=", *cc.device_operands(c, values), c.nrow, c.ncol)[0][-1] == kx.size - 2


def test_first_tile_of_a_tile_cancels_is_all_false_under_ne(T):
    c = ac.device_cases(T)["a_tile_cancels"]
    kx, vx, ky, vy = cc.device_operands(c, "double")
    keys, _ = ac.merged_places(kx, ky)
    assert np.array_equal(keys[:T:2], keys[1:T:2]) and np.array_equal(vx[:T // 2], vy[:T // 2])   # T/2 equal pairs fill tile 0
    v = cc.compare_values("!=", vx, vy)
    assert not v[:T // 2].any() and np.all(v[T // 2:] == 1)
    cp, ri, val = cc.device_expect("compare", "!=", kx, vx, ky, vy, c.nrow, c.ncol)
    assert cp[-1] == 300 and ri.size == 300 and np.all(val == 1)
    # `<` keeps some of the later entries and none of the first tile's
    assert 0 < cc.device_expect("compare", "<", kx, vx, ky, vy, c.nrow, c.ncol)[0][-1] < 300


def test_logical_placements_hold_all_nine_combinations(T):
    c = ac.device_cases(T)["all_match"]
    kx, vx, ky, vy = cc.device_operands(c, "logical")
    assert {(int(a), int(b)) for a, b in zip(vx, vy)} == {(a, b) for a in (1, 0, NA) for b in (1, 0, NA)}
    for op in cc.LOGIC_OPS:
        cp, ri, v = cc.device_expect("logic", op, kx, vx, ky, vy, c.nrow, c.ncol)
        assert 0 < v.size < kx.size and set(v.tolist()) == {1, NA}


def test_expectation_examples():
    """the expectation itself on a few literal values"""
    x = np.array([NA_real, np.nan, -0.0, 0.0, 1.5, -np.inf, np.inf])
    assert cc.compare_values(">", x, np.float64(0)).tolist() == [NA, NA, 0, 0, 1, 0, 1]
    assert cc.compare_values("!=", x, np.int32(0)).tolist() == [NA, NA, 0, 0, 1, 1, 1]
    assert cc.compare_values("<", x, np.float64(0)).tolist() == [NA, NA, 0, 0, 0, 1, 0]
    xi = np.array([NA, 0, 3, -3, INT_MAX], dtype=np.int32)
    assert cc.compare_values(">", xi, np.float64(2.5)).tolist() == [NA, 0, 1, 0, 1]
    assert cc.compare_values("!=", xi, xi).tolist() == [NA, 0, 0, 0, 0]
    assert cc.compare_values("<", xi, np.array([1.0, np.nan, 3.5, -3.0, np.inf])).tolist() == [NA, NA, 1, 0, 1]
    t = np.array([1, 0, NA], dtype=np.int32)
    assert cc.logic_values("&", t, t[::-1]).tolist() == [NA, 0, NA] and cc.logic_values("|", t, t[::-1]).tolist() == [1, 0, 1]
