"""sweep(x, MARGIN, STATS, FUN) without a GPU: the case builder's own proofs (tests/sweep_cases.py), Session.sweep's check
order and messages against a recording dispatcher, the (with_rows, stride, len) derivation against np.unravel_index,
and the two host predicates of sparsearray_amd/csrc/svt_arith_rules.h through tests/sweep_rules_main.cpp."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import arith_cases as ac
import compare_cases as cc
import sweep_cases as sw
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd.api import ARITH_OPCODES, COMPARE_OPCODES, Session, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.device import arith_tile, sweep_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGLSXP, INTSXP, REALSXP = 10, 13, 14
ENTRY = "C_sweep_SVT"


# ---------------------------------------------------------------------------
# the builder's own proofs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    return arith_tile()


def test_index_of_on_literal_cells():
    k = sw.index_of((3, 2), 1)
    assert k.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert sw.index_of((3, 2), 2).tolist() == [[0, 1], [0, 1], [0, 1]]
    # (2, 3, 2): leaf q = j + 3 * l; margin 3 -> l, margin (2, 3) -> q, margin (1, 2) -> i + 2 * j
    assert sw.index_of((2, 3, 2), 3)[0].tolist() == [0, 0, 0, 1, 1, 1]
    assert sw.index_of((2, 3, 2), (2, 3))[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert sw.index_of((2, 3, 2), (1, 2)).tolist() == [[0, 2, 4, 0, 2, 4], [1, 3, 5, 1, 3, 5]]


def test_expectation_on_literal_values():
    """t(t(x) / s) and x * w by hand on a 2 x 2 operand: the stored zero and the product that becomes zero leave"""
    cp, ri = np.array([0, 2, 3]), np.array([0, 1, 1], np.int32)
    val = np.array([6.0, 0.0, -9.0])
    (ocp, ori, ov), cls, t, over = sw.expect_csc("/", 2, (cp, ri, val), (2, 2), 2, np.array([2.0, 3.0]), "double")
    assert (ocp.tolist(), ori.tolist(), ov.tolist(), t, over) == ([0, 1, 2], [0, 1], [3.0, -3.0], "double", False)
    (ocp, ori, ov), cls, t, over = sw.expect_csc("*", 2, (cp, ri, val.astype(np.int32)), (2, 2), 1, np.array([5, 0], np.int32),
                                                  "integer")
    assert (ocp.tolist(), ori.tolist(), ov.tolist(), t) == ([0, 1, 1], [0], [30], "integer")
    (ocp, ori, ov), cls, t, over = sw.expect_csc(">", 2, (cp, ri, val), (2, 2), 1, np.array([5.0, 0.0]), "double")
    assert (ocp.tolist(), ori.tolist(), ov.tolist(), t) == ([0, 1, 1], [0], [1], "logical")


def test_vectors_hold_distinct_values_that_keep_the_result_sparse():
    for op in sw.ARITH_OPS + sw.COMPARE_OPS:
        for st in ("integer", "double"):
            s = sw.stats_for(op, 300, st)
            assert s.dtype == (np.int32 if st == "integer" else np.float64)
            assert np.unique(s).size == (1 if op == "!=" else 300), (op, st)
            if op in cc.COMPARE_OPS:
                assert not cc.compare_values(op, np.zeros(300), s).any(), (op, st)
            else:
                assert np.all(s > 0) and np.all(np.isfinite(s.astype(np.float64)))


def test_placement_operand_has_the_shapes_the_kernel_can_get_wrong(T):
    lengths = np.array(sw.placement_lengths(T))
    cp = np.concatenate([[0], np.cumsum(lengths)])
    assert cp[-1] == 3 * T + 5 and lengths[0] == 0 and lengths[-1] == 0
    assert lengths.max() > T and lengths.max() <= sw.NROW
    # 300 empty leaves in a row, all at one entry position strictly inside a tile (more leaves than threads)
    empty_runs = np.flatnonzero(lengths[1:-1] == 0) + 1
    assert empty_runs.size == 300 and np.all(np.diff(empty_runs) == 1) and cp[empty_runs[0]] % T != 0
    # the boundaries: T and 3T strictly inside leaves of 2-3 entries, 2T inside the long leaf
    for b, small in ((T, True), (2 * T, False), (3 * T, True)):
        q = int(np.searchsorted(cp, b, side="right")) - 1
        assert cp[q] < b < cp[q + 1], b
        assert (2 <= lengths[q] <= 3) if small else lengths[q] > T, (b, lengths[q])
    for type in ("double", "integer"):
        nrow, (cp2, ri, val) = sw.device_operands(T)[f"placement_{type}"]
        assert np.array_equal(cp2, cp) and ri.size == cp[-1]
        col = np.repeat(np.arange(lengths.size), lengths)
        assert np.all((np.diff(ri) > 0) | (np.diff(col) > 0)) and ri.min() >= 0 and ri.max() < nrow
        if type == "double":
            assert ac.is_NA_real(val).any() and (np.isnan(val) & ~ac.is_NA_real(val)).any()
            assert (val == np.inf).any() and (val == -np.inf).any() and (val == 0).any()
        else:
            assert (val == NA_integer).any() and (val == 0).any()
    ops = sw.device_operands(T)
    assert ops["nnz_0_double"][1][2].size == 0 and ops["nnz_T_double"][1][2].size == T and ops["ncol_1_integer"][1][0].size == 2


def test_session_cases_expect_something():
    """every shared case keeps some entries and, where a zero divisor or product can arise, drops some"""
    for name in sw.SESSION_NAMES:
        x, s = sw.session_stats(name)
        _, _, margin, op, st = sw.SESSION_BY_NAME[name]
        want = sw.expect_session(op, x, s, st, margin)
        assert want.dense.shape == (x.dim[0], len(x.leaves)), name
        if x.nzcount() > 0 and op in ("*", "/"):
            assert want.stored.any(), name
    x, s = sw.session_stats("int_overflow")
    assert sw.expect_session("*", x, s, "integer", 2).overflow


# ---------------------------------------------------------------------------
# the index form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("margin", sw.MARGINS_4D + ((1, 2, 3), (1, 2, 3, 4)))
def test_index_form_against_unravel_index(margin):
    """k = (with_rows ? r : 0) + (with_rows ? nrow : 1) * ((q // stride) % len) for every cell of a (5, 4, 3, 2) array"""
    dim = sw.DIM_4D
    with_rows, stride, length = sweep_form(dim, margin)
    nrow, nl = dim[0], int(np.prod(dim[1:]))
    r, q = np.meshgrid(np.arange(nrow), np.arange(nl), indexing="ij")
    k = (r if with_rows else 0) + (nrow if with_rows else 1) * ((q // stride) % length)
    assert np.array_equal(k, sw.index_of(dim, margin))
    assert (nrow if with_rows else 1) * length == sw.stats_length(dim, margin)
    assert nl % (stride * length) == 0


def test_index_form_refuses_other_margins():
    for margin in ((1, 3), (2, 1), (2, 2), (2, 4), (), (0,), (5,), (1.5,), True):
        with pytest.raises(SparseArrayError, match="margin"):
            sweep_form(sw.DIM_4D, margin)
    assert sweep_form((7, 3), 2) == (0, 1, 3) and sweep_form((7, 3), 1) == (1, 1, 1) and sweep_form((7,), 1) == (1, 1, 1)


# ---------------------------------------------------------------------------
# Session.sweep: the checks in their order, then one call
# ---------------------------------------------------------------------------
class Recorder:
    def __init__(self, answer=None):
        self.calls, self.answer = [], answer

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        return self.answer


def _logical():
    return cc.operand("l1")


D = (41, 29)
CHECKS = [
    # (x, MARGIN, STATS, FUN, message) -- the STATS of the type and MARGIN checks have a wrong length too: those checks come first
    ("d1", 2, [1.0], "&", 'invalid Arith or Compare operation "&"'),
    ("logical", 2, [1.0], "*", 'arithmetic operation not supported on SparseArray object of type() "logical"'),
    ("d1", 2, [True], "*", "arithmetic operations between SparseArray objects and logical vectors are not supported"),
    ("d1", 2, ["a"], "/", "arithmetic operations between SparseArray objects and character vectors are not supported"),
    ("d1", 2, [1j], "/", "arithmetic operations between SparseArray objects and complex vectors are not supported"),
    ("d1", 2, [1.0], "+", '"+" is not supported between a SparseArray object and a numeric vector (result wouldn\'t be sparse '
                          'in general)'),
    ("i1", 1, [1], "-", '"-" is not supported between a SparseArray object and a integer vector (result wouldn\'t be sparse'),
    ("d1", 2, [1j], "<", "invalid comparison with complex values"),
    ("d1", 2, ["a"] * D[1], "==", 'type() "character"'),
    ("d1", (1, 3), [1.0], "*", "'MARGIN' does not match dim(x)"),
    ("d3d", (1, 3), [1.0], "*", "strictly increasing run of consecutive dimensions; c(1, 3) is not supported"),
    ("d1", (2, 1), [1.0], "*", "c(2, 1) is not supported"),
    ("d1", 0, [1.0], "*", "'MARGIN' does not match dim(x)"),
    ("d1", 1.5, [1.0], "*", "'MARGIN' must be a vector of dimension numbers"),
    ("d1", 2, np.ones(D[0]), "/", f"length(STATS) is {D[0]} but prod(dim(x)[MARGIN]) is {D[1]}"),
    ("d1", 1, np.ones(D[1]), "/", f"length(STATS) is {D[1]} but prod(dim(x)[MARGIN]) is {D[0]}"),
    ("d1", (1, 2), np.ones(D[1]), "/", f"prod(dim(x)[MARGIN]) is {D[0] * D[1]}"),
]


def _operand(name):
    return _logical() if name == "logical" else cc.operand(name)


@pytest.mark.parametrize("k", range(len(CHECKS)))
def test_checks_come_before_any_call(k):
    xn, margin, stats, op, msg = CHECKS[k]
    rec = Recorder()
    with pytest.raises(SparseArrayError) as e:
        Session(rec).sweep(_operand(xn), margin, stats, op)
    assert msg in str(e.value), str(e.value)
    assert rec.calls == []


def _with(n, at, value, base=2.0, dtype=np.float64):
    s = (np.arange(n) + base).astype(dtype)
    for k in at:
        s[k] = value
    return s


ELEMENT_CHECKS = [
    # (x, MARGIN, FUN, STATS with two offenders, message: the first offender, 1-based, by the scalar method's wording)
    ("d1", 2, "*", _with(29, (7, 3), np.nan), "'x * y' and 'y * x': operations not supported on SparseArray object x when STATS[4] "
                                              "is NA or NaN (result wouldn't be sparse)"),
    ("d1", 2, "*", _with(29, (5, 9), np.inf), "when STATS[6] is Inf or -Inf"),
    ("i1", 1, "/", _with(41, (40, 2), NA_integer, dtype=np.int32), "x / y: operation not supported on SparseArray object x when "
                                                                   "STATS[3] is NA or NaN"),
    ("d1", 2, "^", _with(29, (1, 28), -1.0), "x ^ y: operation not supported on SparseArray object x when STATS[2] is non-positive"),
    ("d1", 2, "^", _with(29, (4, 6), 0.0), "when STATS[5] is non-positive"),
    ("d1", 1, "/", _with(41, (10, 11), 0.0), "x / y: operation not supported on SparseArray object x when STATS[11] == 0"),
    ("i1", 2, "%%", _with(29, (0, 1), 0, dtype=np.int32), "x %% y: operation not supported on SparseArray object x when STATS[1] == 0"),
    ("i1", 2, "%/%", _with(29, (28,), 0.0), "x %/% y: operation not supported on SparseArray object x when STATS[29] == 0"),
    ("d1", 2, "*", _with(29, (8,), np.nan) + _with(29, (2,), np.inf, 0.0), "when STATS[3] is Inf or -Inf"),
    ("d1", 2, ">", _with(29, (3, 4), np.nan), "x > y: operation not supported on SparseArray object x when STATS[4] is NA or NaN"),
    ("d1", 2, ">", _with(29, (6, 7), -1.0), "when STATS[7] is < 0"),
    ("d1", 2, "==", _with(29, (2, 5), 0.0), "when STATS[3] is 0 or FALSE or the empty string"),
    ("d1", 2, "!=", _with(29, (0,), 0.0), "when STATS[2] is not 0, FALSE, or the empty string"),
    ("d1", 1, "<=", _with(41, (), 0.0, base=-40.0), "when STATS[41] is >= 0"),
    ("d1", 1, ">=", _with(41, (9,), 0.0), "when STATS[10] is <= 0, or FALSE, or the empty string"),
    ("d1", 1, "<", _with(41, (9,), 0.5, base=-50.0), "when STATS[10] is > 0"),
    ("l1", 2, "<", np.zeros(29, bool), "when STATS[1] is a logical or raw value"),
]


@pytest.mark.parametrize("k", range(len(ELEMENT_CHECKS)))
def test_elements_are_checked_on_the_host_and_the_first_offender_is_named(k):
    xn, margin, op, stats, msg = ELEMENT_CHECKS[k]
    rec = Recorder()
    with pytest.raises(SparseArrayError) as e:
        Session(rec).sweep(cc.operand(xn), margin, stats, op)
    assert msg in str(e.value) and "(result wouldn't be sparse)" in str(e.value), str(e.value)
    assert rec.calls == []


def test_refusals_that_are_not_about_the_vector():
    rec = Recorder()
    s, d = Session(rec), cc.operand("d1")
    with pytest.raises(SparseArrayError, match="needs an SVT_SparseArray object as 'x'"):
        s.sweep(np.ones(29), 2, d, "*")                               # STATS on the left
    na = SVT_SparseArray(d.dim, d.type, d.leaves, na_background=True)
    with pytest.raises(SparseArrayError, match=r"sweep\(\) is not supported on NaArray objects"):
        s.sweep(na, 2, np.ones(29), "*")
    assert rec.calls == []


def test_checked_calls_reach_the_entry_point_with_the_coerced_vector():
    """one call; the vector's type follows .Arith_SVT1_v2 (double next to a double x and for / and ^) and
    .Compare_SVT1_v2 (the bigger of the two types); an N-d STATS goes over column-major; the answer comes back as it is"""
    d, i, d3 = cc.operand("d1"), cc.operand("i1"), cc.operand("d3d")
    marker = object()
    cases = [(d, 2, np.arange(1, 30), "*", "double", np.float64), (i, 2, np.arange(1, 30), "*", "integer", np.int32),
             (i, 2, np.arange(1, 30), "/", "double", np.float64), (i, 1, np.arange(1, 42), "^", "double", np.float64),
             (i, 1, np.arange(1.0, 42.0), "%%", "double", np.float64), (i, 2, np.arange(1, 30), ">", "integer", np.int32),
             (d, 2, np.arange(1, 30), ">", "double", np.float64), (cc.operand("l1"), 2, np.ones(29, bool), "==", "logical", np.int32),
             (cc.operand("l1"), 2, np.arange(1, 30), ">=", "integer", np.int32)]
    for x, margin, stats, op, stype, dtype in cases:
        rec = Recorder((marker, False))
        assert Session(rec).sweep(x, margin, stats, op) is marker
        (name, gx, gs, gt, gm, gop), = rec.calls
        assert name == ENTRY and gx is x and gt == stype and gm == (margin,) and gop == op
        assert gs.dtype == dtype and np.array_equal(gs, np.asarray(stats).astype(dtype))
    rec = Recorder((marker, False))
    stats = np.arange(1.0, 21.0).reshape(5, 4)
    Session(rec).sweep(d3, (2, 3), stats, "*")
    assert rec.calls[0][4] == (2, 3) and np.array_equal(rec.calls[0][2], stats.reshape(-1, order="F"))


def test_overflow_flag_becomes_the_reference_warning():
    marker = object()
    with pytest.warns(UserWarning, match="NAs produced by integer overflow"):
        assert Session(Recorder((marker, True))).sweep(cc.operand("i1"), 2, np.arange(1, 30), "*") is marker
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Session(Recorder((marker, True))).sweep(cc.operand("i1"), 2, np.arange(1, 30), ">")      # Compare has no such flag


def test_a_dispatcher_without_the_entry_point_says_so(oracle):
    class Lacking:
        def has_entry(self, name):
            return False

        def __call__(self, name, *args):
            raise AssertionError(f"{name} was called")

    with pytest.raises(SparseArrayUnsupported, match=f"{ENTRY} is not offered"):
        Session(Lacking()).sweep(cc.operand("d1"), 2, np.ones(29), "*")
    with pytest.raises(SparseArrayUnsupported, match=f"{ENTRY} is not offered"):
        oracle.sweep(cc.operand("d1"), 2, np.ones(29), ">")


def test_arith_and_compare_still_refuse_a_longer_vector():
    s, d = Session(Recorder()), cc.operand("d1")
    with pytest.raises(SparseArrayError, match="a vector of length != 1"):
        s.arith("*", d, np.ones(29))
    with pytest.raises(SparseArrayError, match="a vector of length != 1"):
        s.compare(">", d, np.ones(29))


# ---------------------------------------------------------------------------
# queries that need no GPU
# ---------------------------------------------------------------------------
def test_workspace_query_is_the_maps():
    from sparsearray_amd._hip import load_library
    lib = load_library()
    for ncol, nnz in ((0, 0), (1, 5000), (100_000, 7), (3, 2 ** 33)):
        assert lib.svt_dev_sweep_ws_bytes(ncol, nnz) == lib.svt_dev_arith_map_ws_bytes(ncol, nnz)


# ---------------------------------------------------------------------------
# the two predicates on the host
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/sweep_rules_main.cpp, built with the host compiler as arith_rules_main.cpp is"""
    exe = tmp_path_factory.mktemp("sweep_rules") / "sweep_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", str(exe),
                    os.path.join(ROOT, "tests", "sweep_rules_main.cpp"), "-lm"], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return [int(a) for a in out.stdout.split("\n")[:-1]]
    return ask


def _hex(v):
    return format(int(np.float64(v).view(np.uint64)), "x")


DEN = 4.9406564584124654e-324
# element -> (is NA / NaN, finite, sign: -1 / 0 / 1)
DOUBLES = [(NA_real, True, False, 0), (float("nan"), True, False, 0), (np.float64(np.uint64(0xFFF80000DEADBEEF).view(np.float64)), True, False, 0),
           (np.inf, False, False, 1), (-np.inf, False, False, -1), (0.0, False, True, 0), (-0.0, False, True, 0),
           (DEN, False, True, 1), (-DEN, False, True, -1), (1e-310, False, True, 1), (1.0, False, True, 1), (-1.0, False, True, -1),
           (2.5, False, True, 1), (-2147483648.0, False, True, -1), (1.7976931348623157e308, False, True, 1)]
INTS = [(NA_integer, True, 0), (0, False, 0), (1, False, 1), (-1, False, -1), (2 ** 31 - 1, False, 1), (-2 ** 31 + 1, False, -1), (7, False, 1)]
LOGICALS = [(NA_integer, True, 0), (0, False, 0), (1, False, 1)]


def _arith_table(op, na, finite, sign):
    """the issue's table"""
    if na:
        return False
    if op == "*":
        return finite
    if op in ("/", "%%", "%/%"):
        return sign != 0
    if op == "^":
        return sign > 0
    return False                                                      # + and -: refused for every vector


def _compare_table(op, na, sign):
    """not NA / NaN, and 0 op s is FALSE"""
    return not na and not {"==": sign == 0, "!=": sign != 0, "<=": sign >= 0, ">=": sign <= 0, "<": sign > 0, ">": sign < 0}[op]


def test_arith_predicate_is_the_table(rules):
    for op, code in ARITH_OPCODES.items():
        got = rules([f"A {code} {REALSXP} {_hex(v)}" for v, *_ in DOUBLES])
        assert got == [int(_arith_table(op, na, fin, sg)) for _, na, fin, sg in DOUBLES], op
        got = rules([f"A {code} {INTSXP} {v}" for v, *_ in INTS])
        assert got == [int(_arith_table(op, na, True, sg)) for _, na, sg in INTS], op
    assert rules([f"A 0 {REALSXP} {_hex(1.0)}", f"A 8 {REALSXP} {_hex(1.0)}"]) == [0, 0]       # unknown opcodes keep nothing


def test_compare_predicate_is_the_table(rules):
    for op, code in COMPARE_OPCODES.items():
        got = rules([f"C {code} {REALSXP} {_hex(v)}" for v, *_ in DOUBLES])
        assert got == [int(_compare_table(op, na, sg)) for _, na, _, sg in DOUBLES], op
        for Rtype, table in ((INTSXP, INTS), (LGLSXP, LOGICALS)):
            got = rules([f"C {code} {Rtype} {v}" for v, *_ in table])
            assert got == [int(_compare_table(op, na, sg)) for _, na, sg in table], (op, Rtype)


def test_int_min_is_na_for_an_integer_element_and_a_number_for_a_double_one(rules):
    mult, gt = ARITH_OPCODES["*"], COMPARE_OPCODES[">"]
    assert rules([f"A {mult} {INTSXP} {NA_integer}", f"A {mult} {REALSXP} {_hex(-2147483648.0)}",
                  f"C {gt} {LGLSXP} {NA_integer}", f"C {gt} {REALSXP} {_hex(2147483648.0)}"]) == [0, 1, 0, 1]
