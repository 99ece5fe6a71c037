"""Arith / unary minus / Math without a GPU: the R-level checks of Session.arith / unary_minus / math and their
messages (R/SparseArray-Arith-methods.R, R/SparseArray-Math-methods.R), the queries that need no device, the
``__host__`` side of the element rules (sparsearray_amd/csrc/svt_arith_rules.h, through tests/arith_rules_main.cpp)
against the expectations of tests/arith_cases.py, and the case builder's proofs of its own placements."""
import os
import subprocess

import numpy as np
import pytest

import arith_cases as ac
import subset_cases as sc
from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.api import ARITH_OPCODES, MATH_OPCODES, Session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGLSXP, INTSXP, REALSXP = 10, 13, 14


# ---------------------------------------------------------------------------
# the Session's checks: raised before any call
# ---------------------------------------------------------------------------
class NoCall:
    """a dispatcher that offers every entry point and must never be reached"""

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        raise AssertionError(f"{name} was called")


@pytest.fixture(scope="module")
def checks():
    return Session(NoCall())


def _logical():
    return sc.operand("logical")[0]


CHECKS = [
    # (op, e1, e2, message)
    ("+", "d1", "d_ncol0", "non-conformable arrays"),
    ("*", "d3d", "d1", "non-conformable arrays"),
    ("/", "d1", "d2", '"/" is not supported between SparseArray objects (result wouldn\'t be sparse in general)'),
    ("^", "i1", "i2", '"^" is not supported between SparseArray objects'),
    ("%%", "d1", "d2", '"%%" is not supported between SparseArray objects'),
    ("+", "d1", 2.0, '"+" is not supported between a SparseArray object and a numeric vector (result wouldn\'t be sparse '
                     'in general)'),
    ("-", "i1", 2, '"-" is not supported between a SparseArray object and a integer vector'),
    ("/", 2.0, "d1", '"/" is not supported between a numeric vector on the left and an SVT_SparseArray object on the right '
                     '(result wouldn\'t be sparse in general)'),
    ("^", 2, "d1", '"^" is not supported between a integer vector on the left'),
    ("*", "d1", float("nan"), "'x * y' and 'y * x': operations not supported on SparseArray object x when y is NA or NaN "
                              "(result wouldn't be sparse)"),
    ("*", NA_real, "d1", "when y is NA or NaN"),
    ("/", "i1", int(NA_integer), "x / y: operation not supported on SparseArray object x when y is NA or NaN"),
    ("*", "d1", float("inf"), "'x * y' and 'y * x': operations not supported on SparseArray object x when y is Inf or -Inf"),
    ("*", "d1", float("-inf"), "when y is Inf or -Inf"),
    ("^", "d1", 0.0, "x ^ y: operation not supported on SparseArray object x when y is non-positive"),
    ("^", "d1", -2, "when y is non-positive"),
    ("/", "d1", 0, "x / y: operation not supported on SparseArray object x when y == 0"),
    ("%%", "i1", 0.0, "x %% y: operation not supported on SparseArray object x when y == 0"),
    ("%/%", "i1", 0, "x %/% y: operation not supported on SparseArray object x when y == 0"),
    ("*", "d1", [1.0, 2.0], "arithmetic operations are not supported between a SparseArray object and a vector of "
                            "length != 1"),
    ("*", "d1", True, "arithmetic operations between SparseArray objects and logical vectors are not supported"),
    ("*", "d1", "a", "arithmetic operations between SparseArray objects and character vectors are not supported"),
    ("*", "d1", 1j, "arithmetic operations between SparseArray objects and complex vectors are not supported"),
    ("+", "logical", "d1", 'arithmetic operation not supported on SparseArray object of type() "logical"'),
    ("*", "d1", "logical", 'arithmetic operation not supported on SparseArray object of type() "logical"'),
    ("*", "logical", 2.0, 'arithmetic operation not supported on SparseArray object of type() "logical"'),
]


def _arg(a):
    if isinstance(a, str) and a == "logical":
        return _logical()
    return ac.operand(a) if isinstance(a, str) and a in ac._OPERANDS else a


@pytest.mark.parametrize("k", range(len(CHECKS)))
def test_arith_checks_raise_the_reference_messages(checks, k):
    op, e1, e2, msg = CHECKS[k]
    if e1 == "logical" and e2 == "d1":
        e2 = sc.build(_logical().dim, "double", np.zeros(_logical().dim, bool))
    if e2 == "logical":
        e1 = sc.build(_logical().dim, "double", np.zeros(_logical().dim, bool))
    with pytest.raises(SparseArrayError) as e:
        checks.arith(op, _arg(e1), _arg(e2))
    assert msg in str(e.value), str(e.value)
    assert not isinstance(e.value, SparseArrayUnsupported)


def test_unary_minus_and_math_checks(checks):
    d, i, lgl = ac.operand("d1"), ac.operand("i1"), _logical()
    with pytest.raises(SparseArrayError, match='arithmetic operation not supported on SparseArray object of type\\(\\) "logical"'):
        checks.unary_minus(lgl)
    for op in ("log", "exp", "cos", "cumsum", "gamma", "log2"):
        with pytest.raises(SparseArrayError) as e:
            checks.math(op, d)
        assert str(e.value) == f"{op}() is not supported on SparseArray objects (result wouldn't be sparse in general)"
    for op in ("sqrt", "log1p", "sin", "round", "signif"):
        for x in (i, lgl):
            with pytest.raises(SparseArrayError) as e:
                checks.math(op, x)
            assert str(e.value) == (f"the {op}() method for SVT_SparseArray objects only supports input of type \"double\" "
                                    "at the moment")
    for digits in ([1, 2], "2", True):
        with pytest.raises(SparseArrayError, match="'digits' must be a single number"):
            checks.math("round", d, digits)
    with pytest.raises(SparseArrayError, match="invalid Arith operation"):
        checks.arith("&", d, d)


def test_checked_calls_reach_the_entry_point_with_the_coerced_scalar():
    """what passes the checks arrives as one call: the scalar's type follows .Arith_SVT1_v2 (double next to a double x
    and for / and ^), a scalar on the left of * goes to the right"""
    seen = []

    class Recorder(NoCall):
        def __call__(self, name, *args):
            seen.append((name,) + args[1:])
            return ("ans", False) if name.startswith("C_Arith") else "ans"

    s, d, i = Session(Recorder()), ac.operand("d1"), ac.operand("i1")
    assert s.arith("*", 3, i) == "ans" and seen.pop() == ("C_Arith_SVT1_v2", 3.0, "integer", "*")
    assert s.arith("*", d, 3) == "ans" and seen.pop() == ("C_Arith_SVT1_v2", 3.0, "double", "*")
    assert s.arith("/", i, 3) == "ans" and seen.pop() == ("C_Arith_SVT1_v2", 3.0, "double", "/")
    assert s.arith("%%", i, -3) == "ans" and seen.pop() == ("C_Arith_SVT1_v2", -3.0, "integer", "%%")
    assert s.arith("^", d, float("inf")) == "ans" and seen.pop() == ("C_Arith_SVT1_v2", float("inf"), "double", "^")
    assert s.arith("-", d, i) == "ans" and seen.pop() == ("C_Arith_SVT1_SVT2", i, "-")
    assert s.unary_minus(i) == "ans" and seen.pop() == ("C_unary_minus_SVT",)
    assert s.math("expm1", d) == "ans" and seen.pop() == ("C_Math_SVT", "expm1", 0.0)
    assert s.math("round", d) == "ans" and seen.pop() == ("C_Math_SVT", "round", 0.0)
    assert s.math("signif", d, 3) == "ans" and seen.pop() == ("C_Math_SVT", "signif", 3.0)


def test_overflow_flag_becomes_the_reference_warning():
    class Overflowing(NoCall):
        def __call__(self, name, *args):
            return "ans", True

    with pytest.warns(UserWarning, match="^NAs produced by integer overflow$"):
        assert Session(Overflowing()).arith("*", ac.operand("i1"), 3) == "ans"


def test_the_oracle_session_does_not_offer_them(oracle):
    d = ac.operand("d1")
    for call in (lambda: oracle.arith("+", d, d), lambda: oracle.arith("*", d, 2.0), lambda: oracle.unary_minus(d),
                 lambda: oracle.math("sqrt", d)):
        with pytest.raises(SparseArrayUnsupported, match="not offered"):
            call()
    with pytest.raises(SparseArrayError, match="non-conformable arrays"):      # the checks come first there too
        oracle.arith("+", d, ac.operand("d_ncol0"))


# ---------------------------------------------------------------------------
# queries that need no GPU
# ---------------------------------------------------------------------------
def test_tile_and_workspace_queries_need_no_gpu():
    from sparsearray_amd._hip import load_library
    from sparsearray_amd.device import arith_tile
    lib = load_library()
    T = arith_tile()
    assert T == lib.svt_dev_arith_tile() and T >= 256 and T & (T - 1) == 0
    for f, args in ((lib.svt_dev_arith_map_ws_bytes, lambda ncol, n: (ncol, n)),
                    (lib.svt_dev_arith_merge_ws_bytes, lambda ncol, n: (ncol, n // 2, n - n // 2))):
        sizes = [f(*args(ncol, n)) for ncol in (0, 1, 1000) for n in (0, 1, T, T + 1, 100 * T)]
        assert all(s >= 256 and s % 256 == 0 for s in sizes)
        assert f(*args(10, 0)) <= f(*args(10, T)) <= f(*args(10, T + 1)) <= f(*args(10, 1000 * T))
        assert f(*args(0, T)) < f(*args(100_000, T))
        assert f(*args(1000, 100 * T)) < 1000 * 8 + 100 * 64 + 8192          # a few words per tile and per column
    assert lib.svt_dev_arith_merge_ws_bytes(5, T, T) == lib.svt_dev_arith_merge_ws_bytes(5, 2 * T, 0)
    assert lib.svt_dev_arith_merge_ws_bytes(-1, -1, -1) == lib.svt_dev_arith_merge_ws_bytes(0, 0, 0)


def test_result_types():
    from sparsearray_amd._hip import load_library
    from sparsearray_amd.device import ARITH_MATH, ARITH_MERGE, ARITH_NEG, ARITH_SCALAR
    rt = load_library().svt_dev_arith_out_Rtype
    code = {"integer": INTSXP, "double": REALSXP}
    for xt in code:
        for yt in code:
            for op in ac.MERGE_OPS:
                assert rt(ARITH_MERGE, ARITH_OPCODES[op], code[xt], code[yt]) == code[ac.out_type("merge", op, xt, yt)]
            for op in ac.SCALAR_OPS:
                assert rt(ARITH_SCALAR, ARITH_OPCODES[op], code[xt], code[yt]) == code[ac.out_type("scalar", op, xt, yt)]
        assert rt(ARITH_NEG, 0, code[xt], 0) == code[xt]
    for op in ac.MATH_OPS:
        assert rt(ARITH_MATH, MATH_OPCODES[op], REALSXP, 0) == REALSXP and rt(ARITH_MATH, MATH_OPCODES[op], INTSXP, 0) == 0
    for kind, op, xt, yt in ((ARITH_MERGE, ARITH_OPCODES["/"], REALSXP, REALSXP), (ARITH_SCALAR, ARITH_OPCODES["+"], REALSXP, REALSXP),
                             (ARITH_MERGE, 1, LGLSXP, REALSXP), (ARITH_SCALAR, 3, INTSXP, LGLSXP), (ARITH_NEG, 0, LGLSXP, 0),
                             (ARITH_MATH, MATH_OPCODES["sin"], REALSXP, 0), (ARITH_MATH, 0, REALSXP, 0), (7, 1, REALSXP, REALSXP)):
        assert rt(kind, op, xt, yt) == 0


# ---------------------------------------------------------------------------
# the host side of the rule functions
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/arith_rules_main.cpp, built with the host compiler, contraction off like the library"""
    exe = tmp_path_factory.mktemp("arith_rules") / "arith_rules"
    cxx = os.environ.get("CXX", "c++")
    # (-fno-builtin: NA_real_ is a signalling NaN, and the compiler's inline floor() would hand it back unquieted
    # where the C library's and the hardware's quiet it)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", str(exe),
                    os.path.join(ROOT, "tests", "arith_rules_main.cpp"), "-lm"], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:-1]
    return ask


def _hex(a):
    return [f"{int(b):016x}" for b in np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64)]


def _from_hex(lines):
    return np.array([int(s, 16) for s in lines], dtype=np.uint64).view(np.float64)


# the specials table of the double rules: every pair of these meets under every operator
TABLE_F64 = np.concatenate([sc.SPECIALS_F64, np.array([1.0, -1.0, 2.0, -3.0, 0.5, -2.5, 7.0, 1e300, -1e-300, 3.0, -7.5])])
DIVISORS = np.array([3.0, -3.0, 2.5, -0.5, np.inf, -np.inf, 1e-320, 7.0])


@pytest.mark.parametrize("op", ["+", "-", "*", "/", "%%", "%/%", "^"])
def test_host_double_rules_agree_with_the_case_module(rules, op):
    ys = TABLE_F64 if op in ac.MERGE_OPS else DIVISORS
    x, y = [a.reshape(-1) for a in np.meshgrid(TABLE_F64, ys, indexing="ij")]
    got = _from_hex(rules([f"D {ARITH_OPCODES[op]} {a} {b}" for a, b in zip(_hex(x), _hex(y))]))
    want, cls = ac._double_arith(op, x, y)
    from sparsearray_amd.svt import is_NA_real
    # every element "stored": the comparison of the case module, glibc's pow within 1 ulp of the correctly rounded value
    ac.compare(got, np.ones(x.size, bool), _expected_all(want, cls, is_NA_real(x)), f"host {op}", max_ulps=1)


def _expected_all(want, cls, from_na):
    e = ac.Expected("double", want, cls, np.ones(want.shape, bool), from_na=from_na)
    e.stored = np.ones(want.shape, bool)             # zeros too: the rule's value is compared everywhere
    return e


@pytest.mark.parametrize("op", ac.MATH_OPS)
def test_host_math_rules_agree_with_the_case_module(rules, op):
    x = np.concatenate([TABLE_F64, np.array(ac.ULPS_INPUTS.get(op, []), dtype=np.float64)])
    got = _from_hex(rules([f"M {MATH_OPCODES[op]} {a}" for a in _hex(x)]))
    want, cls = ac._math(op, x)
    from sparsearray_amd.svt import is_NA_real
    ac.compare(got, np.ones(x.size, bool), _expected_all(want, cls, is_NA_real(x)), f"host {op}", max_ulps=1)


def test_host_log1p_is_the_nearest_double(rules):
    """svt_rule_log1p against the correctly rounded value at 0 ulps: the arguments of the first chain of
    tests/chain_cases.py (x * 0.001: where the device library's log1p was one ulp off for 49 of 8747), and 20 000 seeded
    ones -- magnitudes from 2^-54 to 1e308, arguments down to -1 + 2^-53, table boundaries k / 128 and 2^k - 1"""
    import chain_cases as cc
    rng = np.random.default_rng(91)
    x = np.concatenate([cc.operand("x").val * 0.001, np.array(ac.ULPS_INPUTS["log1p"]),
                        np.exp(rng.uniform(np.log(2.0 ** -54), np.log(1e308), 6000)),
                        -np.exp(rng.uniform(np.log(2.0 ** -54), 0.0, 4000)), rng.uniform(-1.0, 1.0, 4000),
                        -1.0 + np.exp(rng.uniform(np.log(2.0 ** -53), 0.0, 3000)),
                        rng.integers(-32, 2000, 2000) / 128 + rng.normal(size=2000) * 1e-12, 2.0 ** rng.integers(-54, 1023, 1000) - 1.0])
    got = _from_hex(rules([f"M {MATH_OPCODES['log1p']} {a}" for a in _hex(x)]))
    want, cls = ac._math("log1p", x)
    from sparsearray_amd.svt import is_NA_real
    ac.compare(got, np.ones(x.size, bool), _expected_all(want, cls, is_NA_real(x)), "host log1p", max_ulps=0)


def test_host_int_rules_agree_with_the_case_module(rules):
    """NA propagation, %% with the divisor's sign, %/% flooring, a zero divisor, and the overflow edges: INT_MAX + 1 and
    -INT_MAX - 1 (= INT_MIN, which is NA_integer_) overflow, INT_MAX and -INT_MAX do not"""
    vals = np.array([NA_integer, 0, 1, -1, 7, -7, 3, -3, 2, 46341, -46341, 65536, ac.INT_MAX, -ac.INT_MAX, ac.INT_MAX - 1],
                    dtype=np.int32)
    x, y = [a.reshape(-1) for a in np.meshgrid(vals, vals, indexing="ij")]
    for op in ("+", "-", "*", "%%", "%/%"):
        out = [ln.split() for ln in rules([f"I {ARITH_OPCODES[op]} {a} {b}" for a, b in zip(x, y)])]
        got, flags = np.array([int(o[0]) for o in out], dtype=np.int64), np.array([int(o[1]) for o in out], dtype=bool)
        for k in range(x.size):
            want, over = ac._int_arith(op, x[k:k + 1], y[k:k + 1])
            assert (got[k], flags[k]) == (int(want[0]), over), f"{x[k]} {op} {y[k]}: {got[k]}, {flags[k]}"
    edge = rules([f"I {ARITH_OPCODES['+']} {ac.INT_MAX} 1", f"I {ARITH_OPCODES['-']} {-ac.INT_MAX} 1",
                  f"I {ARITH_OPCODES['+']} {ac.INT_MAX} 0", f"I {ARITH_OPCODES['-']} {-ac.INT_MAX} 0",
                  f"I {ARITH_OPCODES['%%']} -7 3", f"I {ARITH_OPCODES['%%']} 7 -3", f"I {ARITH_OPCODES['%/%']} -7 3",
                  f"I {ARITH_OPCODES['%/%']} 7 -3", f"I {ARITH_OPCODES['%%']} 7 0"])
    assert edge == [f"{ac.INT_MIN} 1", f"{ac.INT_MIN} 1", f"{ac.INT_MAX} 0", f"{-ac.INT_MAX} 0", "2 0", "-2 0", "-3 0", "-3 0",
                    f"{ac.INT_MIN} 0"]


def test_specials_of_mod_and_idiv_by_r_examples(rules):
    """a few values R prints, stated literally (not through the case module's formulas)"""
    inf, nan = np.inf, np.nan
    rows = [("%%", -1.0, inf, inf), ("%%", 1.0, inf, 1.0), ("%%", 1.0, -inf, -inf), ("%%", -1.0, -inf, -1.0),
            ("%%", inf, 3.0, nan), ("%%", -inf, -3.0, nan), ("%%", 5.5, -3.0, -0.5), ("%%", -5.5, 3.0, 0.5),
            ("%/%", -1.0, inf, -1.0), ("%/%", 1.0, -inf, -1.0), ("%/%", 1.0, inf, 0.0), ("%/%", -inf, inf, nan),
            ("%/%", inf, -inf, nan), ("%/%", 5.5, -3.0, -2.0), ("%/%", -5.5, 3.0, -2.0), ("%/%", inf, 3.0, inf),
            ("^", 1.0, inf, 1.0), ("^", -2.0, inf, nan), ("^", -0.5, inf, nan), ("^", -inf, 2.5, nan), ("^", -inf, 3.0, -inf),
            ("^", 0.5, inf, 0.0), ("^", 2.0, inf, inf), ("^", NA_real, 2.0, nan)]
    got = _from_hex(rules([f"D {ARITH_OPCODES[op]} {_hex(x)[0]} {_hex(y)[0]}" for op, x, y, _ in rows]))
    for (op, x, y, want), g in zip(rows, got):
        assert (np.isnan(g) and np.isnan(want)) or g == want, f"{x} {op} {y}: {g}, R gives {want}"


# ---------------------------------------------------------------------------
# the case builder proves its own placements
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    from sparsearray_amd.device import arith_tile
    return arith_tile()


def test_straddling_cases_have_their_pairs_on_the_tile_boundaries(T):
    for name in ("straddling_pairs_one_column", "straddling_pairs_columns", "straddling_pairs_cancel"):
        c = ac.device_cases(T)[name]
        keys, side = ac.merged_places(c.kx, c.ky)
        assert c.pairs_at == (T - 1, 2 * T - 1)
        for p in c.pairs_at:                              # x's entry closes a tile, y's entry of the same position opens the next
            assert keys[p] == keys[p + 1] and (side[p], side[p + 1]) == (0, 1) and (p + 1) % T == 0
        assert np.count_nonzero(keys[1:] == keys[:-1]) == 2
    c = ac.device_cases(T)["straddling_pairs_cancel"]
    assert c.want[0][-1] == c.kx.size - 2                 # both pairs cancelled, every other entry kept
    keys, side = ac.merged_places(*[ac.device_cases(T)["all_match_shifted"].__dict__[k] for k in ("kx", "ky")])
    pairs = np.flatnonzero(keys[1:] == keys[:-1])
    assert np.all(pairs % 2 == 1) and np.any(pairs % 8 == 7) and (T - 1) in pairs


def test_tile_exact_cases_have_the_lengths_they_claim(T):
    cases = ac.device_cases(T)
    for name, length in (("merged_length_-1_from_T", T - 1), ("merged_length_+0_from_T", T), ("merged_length_+1_from_T", T + 1),
                         ("merged_length_2T", 2 * T)):
        c = cases[name]
        keys, side = ac.merged_places(c.kx, c.ky)
        assert c.merged_length == keys.size == length
        assert 0 < np.count_nonzero(keys[1:] == keys[:-1]) < c.ky.size          # some pairs, not only pairs
    c = cases["a_tile_cancels"]
    keys, _ = ac.merged_places(c.kx, c.ky)
    assert np.array_equal(keys[:T:2], keys[1:T:2]) and np.array_equal(c.vx[:T // 2], c.vy[:T // 2])
    assert c.want[0][-1] == 300 and np.array_equal(c.want[2], -c.vx[T // 2:])
    c = cases["one_column_holds_everything"]
    assert c.ncol == 1 and c.nrow > 3 * T and c.merged_length > 2 * T
    c = cases["100000_empty_columns"]
    assert c.ncol > 100_000 and c.merged_length == 10 and np.count_nonzero(np.diff(c.want[0])) <= 5
    for c in cases.values():
        assert max(c.kx.size, c.ky.size) <= 3 * T + 100
        for cp, ri, _ in (c.x, c.y, c.want):
            assert cp[0] == 0 and np.all(np.diff(cp) >= 0) and cp[-1] == ri.size
            for j in np.flatnonzero(np.diff(cp) > 1)[:50]:
                assert np.all(np.diff(ri[cp[j]:cp[j + 1]]) > 0)


def test_expectation_examples():
    """the expectation itself on a few literal values: it is written from R's definitions, and this pins them"""
    x = np.array([ac.INT_MAX, -ac.INT_MAX, 7, -7, NA_integer, 0], dtype=np.int32)
    v, over = ac._int_arith("+", x, np.int32(1))
    assert v.tolist() == [ac.INT_MIN, 1 - ac.INT_MAX, 8, -6, ac.INT_MIN, 1] and over
    v, over = ac._int_arith("-", x, np.int32(1))
    assert v.tolist() == [ac.INT_MAX - 1, ac.INT_MIN, 6, -8, ac.INT_MIN, -1] and over
    assert ac._int_arith("%%", x, np.int32(-3))[0].tolist() == [-2, -1, -2, -1, ac.INT_MIN, 0]
    assert ac._int_arith("%/%", x, np.int32(-3))[0].tolist() == [-715827883, 715827882, -3, 2, ac.INT_MIN, 0]
    assert ac.r_log1p(-1.0) == -np.inf and np.isnan(ac.r_log1p(-1.5)) and ac.r_log1p(4.9406564584124654e-324) == 4.9406564584124654e-324
    assert ac.r_expm1(-np.inf) == -1.0 and ac.r_expm1(710.0) == np.inf and ac.r_expm1(1e-300) == 1e-300
    assert ac.r_pow(1e154, 2) == 1e308 and ac.r_pow(1e300, 2.5) == np.inf and ac.r_pow(-8.0, 3.0) == -512.0
    assert ac.r_pow(2.0, 0.5) == 1.4142135623730951 and ac.r_pow(4.9406564584124654e-324, 2) == 0.0
    assert ac.ulp_distance(np.array([1.0, -0.0, np.inf]), np.array([1.0000000000000002, 0.0, 1.7976931348623157e308])).tolist() == [1, 0, 1]
