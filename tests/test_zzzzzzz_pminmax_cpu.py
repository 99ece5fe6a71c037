"""pmin() / pmax() and is.na() / is.nan() / is.infinite() without a GPU: the three host rules of
sparsearray_amd/csrc/svt_arith_rules.h through tests/pminmax_rules_main.cpp against numpy's statement of the formulas, the
step-by-step emulation of the reference's .pminmax2 against the closed formula, the case builder's own proofs
(tests/pminmax_cases.py), and the checks of Session.pmin / pmax / is_na / sweep(..., "pmin") against a recording
dispatcher."""
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import pminmax_cases as pc
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd.api import (ISFUN_OPCODES, PMINMAX_NA_RM, PMINMAX_OPCODES, Session, SparseArrayError,
                                 SparseArrayUnsupported)
from sparsearray_amd.device import arith_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGLSXP, INTSXP, REALSXP = 10, 13, 14


# ---------------------------------------------------------------------------
# the rule program
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_lines(tmp_path_factory):
    """the output of tests/pminmax_rules_main.cpp, built with the host compiler under its address and undefined-behaviour
    sanitizers (a stand-alone program: the sanitizers' runtime is linked in)"""
    exe = tmp_path_factory.mktemp("pminmax_rules") / "pminmax_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pminmax_rules_main.cpp"), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    assert out.stderr == ""
    return out.stdout.split("\n")[:-1]


def _hex(v):
    v = np.asarray(v)
    return format(int(pc.bits(v.reshape(1))[0]) & (2 ** 64 - 1 if v.dtype == np.float64 else 2 ** 32 - 1),
                  "016x" if v.dtype == np.float64 else "08x")


def test_the_three_rules_are_the_formulas_on_bits(rule_lines):
    want = []
    for tx, ty in (("double", "double"), ("integer", "integer"), ("integer", "double"), ("double", "integer")):
        X, Y, t = pc.TABLE[tx], pc.TABLE[ty], pc.out_type(tx, ty)
        xw, yw = np.repeat(pc.widen(X, t), Y.size), np.tile(pc.widen(Y, t), X.size)
        for op in pc.OPS:
            for na_rm in (0, 1):
                v = pc.formula(op, bool(na_rm), xw, yw)
                want += [f"P {tx[0]} {ty[0]} {PMINMAX_OPCODES[op]} {na_rm} {k // Y.size} {k % Y.size} {_hex(v[k])}" for k in range(v.size)]
    for fn in pc.ISFUNS:
        for t in ("double", "integer"):
            want += [f"F {t[0]} {ISFUN_OPCODES[fn]} {i} {r}" for i, r in enumerate(pc.isfun_values(fn, pc.TABLE[t]))]
    for op in pc.OPS:
        for na_rm in (0, PMINMAX_NA_RM):
            for t in ("double", "integer"):
                want += [f"K {t[0]} {PMINMAX_OPCODES[op] | na_rm} {i} {int(pc.keeps_sparse(op, s, t))}" for i, s in enumerate(pc.TABLE[t])]
    assert len(rule_lines) == len(want) == 4 * (81 + 25 + 45 + 45) + 3 * 14 + 4 * 14
    assert rule_lines == want


def test_formula_by_hand():
    """the formula itself on literal values: ties take x (seen on the zeros' signs), an NA wins without na_rm and loses
    with it, two NaNs give x's without na_rm and x's with it, the payload survives"""
    x = np.array([0.0, -0.0, 3.0, NA_real, 2.0, pc.NAN_PAYLOAD, NA_real])
    y = np.array([-0.0, 0.0, 1.0, 1.0, float("nan"), NA_real, pc.NAN_PAYLOAD])
    hexes = lambda v: [_hex(e) for e in v]                            # noqa: E731
    assert hexes(pc.formula("pmin", False, x, y)) == hexes(np.array([0.0, -0.0, 1.0, NA_real, float("nan"), pc.NAN_PAYLOAD, NA_real]))
    assert hexes(pc.formula("pmin", True, x, y)) == hexes(np.array([0.0, -0.0, 1.0, 1.0, 2.0, pc.NAN_PAYLOAD, NA_real]))
    assert hexes(pc.formula("pmax", False, x, y)) == hexes(np.array([0.0, -0.0, 3.0, NA_real, float("nan"), pc.NAN_PAYLOAD, NA_real]))
    i = np.array([5, NA_integer, -7, NA_integer], np.int32)
    j = np.array([NA_integer, 2, -7, NA_integer], np.int32)
    assert pc.formula("pmax", False, i, j).tolist() == [NA_integer, NA_integer, -7, NA_integer]
    assert pc.formula("pmax", True, i, j).tolist() == [5, 2, -7, NA_integer]


# ---------------------------------------------------------------------------
# the rule is the reference's: .pminmax2 step by step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ty", pc.TYPES)
@pytest.mark.parametrize("tx", pc.TYPES)
def test_the_five_steps_of_the_reference_give_the_formula(tx, ty):
    X, Y, t = pc.TABLE[tx], pc.TABLE[ty], pc.out_type(tx, ty)
    x, y = np.repeat(X, Y.size), np.tile(Y, X.size)
    for op in pc.OPS:
        for na_rm in (False, True):
            got = pc.steps(op, na_rm, x, y, t)
            want = pc.formula(op, na_rm, pc.widen(x, t), pc.widen(y, t))
            assert got.dtype == want.dtype == pc.np_dtype(t)
            assert np.array_equal(pc.bits(got), pc.bits(want)), (tx, ty, op, na_rm)


# ---------------------------------------------------------------------------
# the builder's own proofs
# ---------------------------------------------------------------------------
def test_expectations_on_literal_2x2_cases():
    """by hand.  x = [[6, 0s], [., -9]] (0s: a stored zero), y = [[2, -1], [NA, .]] as linear keys over (2, 2)"""
    kx, vx = np.array([0, 2, 3]), np.array([6.0, 0.0, -9.0])
    ky, vy = np.array([0, 1, 2]), np.array([2.0, NA_real, -1.0])
    (cp, ri, v), t = pc.expect_merge("pmin", False, 2, 2, kx, vx, "double", ky, vy, "double")
    # cells: (0,0) min(6, 2) = 2; (1,0) x implicit 0, y NA -> NA; (0,1) stored zero against -1 -> -1; (1,1) -9 against 0 -> -9
    assert (cp.tolist(), ri.tolist(), t) == ([0, 2, 4], [0, 1, 0, 1], "double")
    assert [_hex(e) for e in v] == [_hex(e) for e in np.array([2.0, NA_real, -1.0, -9.0])]
    (cp, ri, v), t = pc.expect_merge("pmax", True, 2, 2, kx, vx, "double", ky, vy, "double")
    # (0,0) 6; (1,0) NA removed: x's implicit 0 -> not stored; (0,1) max(0s, -1) = 0 -> the result becomes zero, not stored; (1,1) 0
    assert (cp.tolist(), ri.tolist(), v.tolist()) == ([0, 1, 1], [0], [6.0])
    # an integer x against a double y: the result is double, NA_integer_ arrives as NA_real_
    (cp, ri, v), t = pc.expect_merge("pmin", False, 2, 2, kx, np.array([6, NA_integer, -9], np.int32), "integer", ky, vy, "double")
    assert t == "double" and ri.tolist() == [0, 1, 0, 1] and _hex(v[2]) == _hex(NA_real) and v[3] == -9.0
    # the scalar map: cap at 5, and at 0 (what is above disappears); with na_rm an NA entry becomes the scalar
    csc = (np.array([0, 2, 4]), np.array([0, 1, 0, 1], np.int32), np.array([6.0, -3.0, NA_real, 0.0]))
    (cp, ri, v), t = pc.expect_map("pmin", False, csc, "double", 5.0, "double")
    assert (cp.tolist(), ri.tolist()) == ([0, 2, 3], [0, 1, 0]) and v[:2].tolist() == [5.0, -3.0] and _hex(v[2]) == _hex(NA_real)
    (cp, ri, v), t = pc.expect_map("pmin", True, csc, "double", 0, "integer")
    assert (cp.tolist(), ri.tolist(), v.tolist(), t) == ([0, 1, 1], [1], [-3.0], "double")
    (cp, ri, v), t = pc.expect_map("pmin", True, csc, "double", 5.0, "double")
    assert (cp.tolist(), v.tolist()) == ([0, 2, 3], [5.0, -3.0, 5.0])
    # a cap per column
    (cp, ri, v), t = pc.expect_sweep("pmin", False, csc, "double", (2, 2), 2, np.array([1.0, 0.0]), "double")
    assert (cp.tolist(), ri.tolist()) == ([0, 2, 3], [0, 1, 0]) and v[:2].tolist() == [1.0, -3.0]
    # is.na and friends
    assert [a.tolist() for a in pc.expect_isfun("is.na", csc)] == [[0, 0, 1], [0], [1]]
    assert pc.expect_isfun("is.nan", csc)[1].size == 0
    inf = (csc[0], csc[1], np.array([np.inf, pc.NAN_PAYLOAD, -np.inf, 1.0]))
    assert [a.tolist() for a in pc.expect_isfun("is.infinite", inf)] == [[0, 1, 2], [0, 0], [1, 1]]
    assert [a.tolist() for a in pc.expect_isfun("is.nan", inf)] == [[0, 1, 1], [1], [1]]


def test_table_pair_holds_every_combination_and_both_lonely_sides():
    for tx in pc.TYPES:
        for ty in pc.TYPES:
            nrow, ncol, kx, vx, ky, vy = pc.table_pair(tx, ty)
            X, Y = pc.TABLE[tx], pc.TABLE[ty]
            assert np.all(np.diff(kx) > 0) and np.all(np.diff(ky) > 0) and max(kx[-1], ky[-1]) < nrow * ncol
            both, ix, iy = np.intersect1d(kx, ky, return_indices=True)
            combos = {(_hex(a), _hex(b)) for a, b in zip(vx[ix], vy[iy])}
            assert combos == {(_hex(a), _hex(b)) for a in X for b in Y}
            assert np.setdiff1d(kx, ky).size == X.size and np.setdiff1d(ky, kx).size == Y.size


def test_placement_pair_has_the_shapes_the_merge_can_get_wrong():
    T = arith_tile()
    nrow, ncol, kx, ky, long_leaf = pc.placement_keys(T)
    keys, side = pc.ac.merged_places(kx, ky)
    assert keys.size == 3 * T + 5
    leaf = keys // nrow
    counts = np.bincount(leaf, minlength=ncol)
    assert counts[0] == 0 and counts[-1] == 0                           # an empty first and last leaf
    # T strictly inside a short leaf
    q = leaf[T]
    assert leaf[T - 1] == q and counts[q] == 3 and (leaf == q).nonzero()[0][0] < T
    # 300 empty leaves in a row at a place strictly inside a tile
    empty = np.flatnonzero(counts[1:-1] == 0) + 1
    assert empty.size == 300 and np.all(np.diff(empty) == 1) and int((leaf < empty[0]).sum()) % T != 0
    # 2T inside a leaf longer than a tile
    assert leaf[2 * T - 1] == leaf[2 * T] == long_leaf and counts[long_leaf] > T
    # 3T inside a pair: the same cell on both sides, x's entry the last place of a tile, y's the first of the next
    assert keys[3 * T - 1] == keys[3 * T] and side[3 * T - 1] == 0 and side[3 * T] == 1
    assert np.intersect1d(kx, ky).size == 1
    for tx, ty in (("double", "double"), ("integer", "integer"), ("integer", "double"), ("logical", "logical")):
        _, _, _, vx, _, vy = pc.placement_pair(T, tx, ty)
        assert pc.isna(vx).any() and pc.isna(vy).any() and (vx == 0).any()
        (cp, ri, v), t = pc.expect_merge("pmin", False, nrow, ncol, kx, vx, tx, ky, vy, ty)
        assert 0 < ri.size < keys.size - 1                               # some results are zero and leave


def test_random_pair_is_what_the_chain_needs():
    nrow, ncol, kx, vx, ky, vy = pc.random_pair()
    assert kx.size == ky.size == 3000 and np.intersect1d(kx, ky).size == 1000
    for v in (vx, vy):
        assert not (v == 0).any() and np.isnan(v).sum() >= 40 and (pc.isfun_values("is.nan", v) == 1).any()


def test_isfun_operand_has_the_specials_on_both_sides_of_the_tile_boundary():
    T = arith_tile()
    for t in pc.TYPES:
        nrow, (cp, ri, val) = pc.isfun_operand(T, t)
        assert val.size == T + 300
        for fn in pc.ISFUNS if t == "double" else ("is.na",):
            hit = np.flatnonzero(pc.isfun_values(fn, val))
            assert (hit < T).any() and (hit >= T).any(), (t, fn)
        assert (val == 0).any()


# ---------------------------------------------------------------------------
# Session.pmin / pmax / is_na / is_nan / is_infinite / sweep(..., "pmin"): the checks in their order, then one call
# ---------------------------------------------------------------------------
class Recorder:
    def __init__(self, answer=None):
        self.calls, self.answer = [], answer

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        return self.answer(*args) if callable(self.answer) else self.answer


def _typed(name, dim=(41, 29)):
    """an empty object of extents ``dim`` that says its type() is ``name`` (the package builds no object of a type
    outside logical / integer / double: the name is put on afterwards)"""
    x = SVT_SparseArray(dim, "double", [None] * int(np.prod(dim[1:])))
    x.type = name
    return x


def test_psummarize_drops_nulls_checks_na_rm_and_needs_an_input():
    rec = Recorder()
    s, d = Session(rec), cc.operand("d1")
    with pytest.raises(SparseArrayError, match="'na.rm' must be TRUE or FALSE"):
        s.pmin(d, d, na_rm=1)
    with pytest.raises(SparseArrayError, match="'na.rm' must be TRUE or FALSE"):
        s.pmax(None, na_rm=None)                                      # (checked before "no input", as in .psummarize)
    with pytest.raises(SparseArrayError, match="no input"):
        s.pmin(None, None)
    with pytest.raises(SparseArrayError, match="no input"):
        s.pmax()
    assert s.pmin(None, d, None) is d and s.pmax(d, na_rm=True) is d   # one object comes back as it is
    assert rec.calls == []


def test_two_objects_make_one_call_and_three_fold_from_the_right():
    a, b, c = cc.operand("d1"), cc.operand("i1"), cc.operand("d1s")
    marks = []

    def answer(x, y, op, na_rm):
        marks.append(_typed("double"))
        return marks[-1]

    rec = Recorder(answer)
    assert Session(rec).pmin(a, None, b, na_rm=True) is marks[0]
    assert rec.calls == [("C_pminmax_SVT1_SVT2", a, b, "pmin", True)]
    rec = Recorder(answer)
    del marks[:]
    # (the fold needs results that are SVT_SparseArray objects: hand back operands)
    rec.answer = lambda x, y, op, na_rm: marks.append(SVT_SparseArray(x.dim, "double", x.leaves)) or marks[-1]
    out = Session(rec).pmax(a, b, c)
    assert [call[:3] for call in rec.calls] == [("C_pminmax_SVT1_SVT2", b, c), ("C_pminmax_SVT1_SVT2", a, marks[0])]
    assert out is marks[1] and all(call[3:] == ("pmax", False) for call in rec.calls)


def _named(tag, dim=(41, 29)):
    x = _typed("double", dim)
    x.dimnames = [[f"{tag}r{i}" for i in range(dim[0])], None]
    return x


def test_dimnames_are_those_of_the_first_object_that_has_them():
    """get_first_non_NULL_dimnames of .pminmax2, through the fold: whatever the entry point hands back, the result carries
    the dimnames of the first object that has some; the scalar form and sweep(..., "pmin") keep those of x"""
    plain, a, b = _typed("double"), _named("a"), _named("b")
    answer = lambda *args: _typed("double")                             # noqa: E731  (a result without dimnames)
    for objects, want in (((plain, a), a), ((a, plain), a), ((a, b), a), ((b, a), b), ((plain, plain), None),
                          ((plain, a, b), a), ((plain, plain, b), b), ((b, plain, a), b), ((plain, None, a, 5.0), a),
                          ((3.0, a), a), ((a, 3.0), a), ((plain, 3.0), None)):
        for method in ("pmin", "pmax"):
            s = -1.0 if method == "pmax" else 1.0
            objs = tuple(o if isinstance(o, SVT_SparseArray) or o is None else s * o for o in objects)
            got = getattr(Session(Recorder(answer)), method)(*objs)
            assert got.dimnames == (None if want is None else want.dimnames), (method, objects)
    rec = Recorder(lambda *args: (_typed("double"), False))
    assert Session(rec).sweep(a, 2, np.ones(29), "pmin").dimnames == a.dimnames
    assert Session(rec).sweep(plain, 2, np.ones(29), "pmin").dimnames is None


def test_refusals_between_two_objects():
    rec = Recorder()
    s, d = Session(rec), cc.operand("d1")
    with pytest.raises(SparseArrayError, match="non-conformable arrays"):
        s.pmin(d, _typed("double", (41, 28)))
    with pytest.raises(SparseArrayError, match="non-conformable arrays"):
        s.pmin(d, _typed("double", (41, 29, 1)))
    for bad in ("character", "raw", "complex", "list"):
        with pytest.raises(SparseArrayUnsupported, match=f'type\\(\\) "{bad}"'):
            s.pmax(d, _typed(bad))
        with pytest.raises(SparseArrayUnsupported, match=f'type\\(\\) "{bad}"'):
            s.pmin(_typed(bad), d)
    na = SVT_SparseArray(d.dim, d.type, d.leaves, na_background=True)
    with pytest.raises(SparseArrayUnsupported, match="NaArray"):
        s.pmin(d, na)
    assert rec.calls == []


SCALAR_REFUSALS = [("pmin", -1.0, r"y is < 0 \(y = -1\.0"), ("pmin", -3, r"y is < 0 \(y = -3"), ("pmax", 0.5, r"y is > 0 \(y = 0\.5"),
                   ("pmax", True, r"y is > 0 \(y = True"), ("pmin", float("nan"), r"y is NA or NaN \(y = nan"),
                   ("pmax", NA_real, "y is NA or NaN"), ("pmin", np.int32(NA_integer), r"y is NA or NaN \(y = -2147483648"),
                   ("pmin", -np.inf, r"y is < 0 \(y = -inf")]


@pytest.mark.parametrize("k", range(len(SCALAR_REFUSALS)))
def test_a_scalar_that_would_fill_the_result_is_refused_and_named(k):
    name, s, msg = SCALAR_REFUSALS[k]
    rec = Recorder()
    for objects in ((cc.operand("d1"), s), (s, cc.operand("d1"))):
        with pytest.raises(SparseArrayError, match=msg) as e:
            getattr(Session(rec), name)(*objects)
        assert "result wouldn't be sparse" in str(e.value)
    assert rec.calls == []


def test_the_scalar_form_makes_one_call_with_the_scalars_type():
    d, marker = cc.operand("d1"), _typed("double")
    for name, s, stype in (("pmin", 10.0, "double"), ("pmin", 0, "integer"), ("pmin", np.inf, "double"), ("pmax", -0.0, "double"),
                           ("pmax", False, "logical"), ("pmax", -4, "integer"), ("pmin", True, "logical")):
        for flip in (False, True):
            rec = Recorder(marker)
            assert getattr(Session(rec), name)(*((s, d) if flip else (d, s)), na_rm=flip) is marker
            assert rec.calls == [("C_pminmax_SVT1_v2", d, float(s), stype, name, flip)]
    rec = Recorder()
    with pytest.raises(SparseArrayError, match="vector of length != 1"):
        Session(rec).pmin(d, [1.0, 2.0])
    with pytest.raises(SparseArrayUnsupported, match="character vector"):
        Session(rec).pmin(d, "a")
    with pytest.raises(SparseArrayUnsupported, match="complex vector"):
        Session(rec).pmax(d, 1j)
    with pytest.raises(SparseArrayError, match="needs an SVT_SparseArray object"):
        Session(rec).pmin(1.0, 2.0)
    assert rec.calls == []


def test_is_functions_check_and_call():
    d, marker = cc.operand("d1"), object()
    for method, fn in (("is_na", "is.na"), ("is_nan", "is.nan"), ("is_infinite", "is.infinite")):
        rec = Recorder(marker)
        s = Session(rec)
        assert getattr(s, method)(d) is marker and rec.calls == [("C_SVT_apply_isFUN", d, fn)]
        with pytest.raises(SparseArrayError, match="needs an SVT_SparseArray object"):
            getattr(s, method)(np.ones((2, 2)))
        with pytest.raises(SparseArrayUnsupported, match="NaArray"):
            getattr(s, method)(SVT_SparseArray(d.dim, d.type, d.leaves, na_background=True))
        for bad in ("character", "raw", "complex", "list"):
            with pytest.raises(SparseArrayUnsupported, match=f'type\\(\\) "{bad}"'):
                getattr(s, method)(_typed(bad))
        assert len(rec.calls) == 1


def _with(n, at, value, dtype=np.float64, base=2.0):
    s = (np.arange(n) + base).astype(dtype)
    s[list(at)] = value
    return s


SWEEP_REFUSALS = [("pmin", 2, _with(29, (7, 3), -1.0), "x pmin y: operation not supported on SparseArray object x when STATS[4] is < 0"),
                  ("pmin", 1, _with(41, (40, 12), np.nan), "when STATS[13] is NA or NaN"),
                  ("pmin", 2, _with(29, (28,), NA_integer, np.int32), "when STATS[29] is NA or NaN"),
                  ("pmax", 2, _with(29, (5, 6), 1.0, base=-40.0), "x pmax y: operation not supported on SparseArray object x when STATS[6] is > 0"),
                  ("pmax", 1, _with(41, (0,), True, np.bool_, base=0.0) | (np.arange(41) == 9), "when STATS[1] is > 0")]


@pytest.mark.parametrize("k", range(len(SWEEP_REFUSALS)))
def test_sweep_refuses_the_first_element_on_the_wrong_side_of_zero(k):
    op, margin, stats, msg = SWEEP_REFUSALS[k]
    rec = Recorder()
    with pytest.raises(SparseArrayError) as e:
        Session(rec).sweep(cc.operand("d1"), margin, stats, op)
    assert msg in str(e.value) and "(result wouldn't be sparse)" in str(e.value), str(e.value)
    assert rec.calls == []


def test_sweep_reaches_the_entry_point_with_the_vector_in_its_own_type():
    d, i, marker = cc.operand("d1"), cc.operand("i1"), _typed("double")
    for x, stats, stype, dtype in ((d, np.arange(29), "integer", np.int32), (i, np.arange(29.0), "double", np.float64),
                                   (i, np.ones(29, bool), "logical", np.int32)):
        rec = Recorder((marker, False))
        assert Session(rec).sweep(x, 2, stats, "pmin", na_rm=True) is marker
        (name, gx, gs, gt, gm, gop, gna), = rec.calls
        assert (name, gt, gm, gop, gna) == ("C_sweep_SVT", stype, (2,), "pmin", True) and gx is x
        assert gs.dtype == dtype and np.array_equal(gs, stats.astype(dtype))
    rec = Recorder()
    with pytest.raises(SparseArrayError, match="'na.rm' must be TRUE or FALSE"):
        Session(rec).sweep(d, 2, np.ones(29), "pmax", na_rm="yes")
    with pytest.raises(SparseArrayUnsupported, match='type\\(\\) "character"'):
        Session(rec).sweep(_typed("character"), 2, np.ones(29), "pmin")
    with pytest.raises(SparseArrayUnsupported, match="complex vector"):
        Session(rec).sweep(d, 2, np.ones(29) * 1j, "pmin")
    assert rec.calls == []


def test_dispatchers_without_the_entry_points_say_so(oracle):
    d = cc.operand("d1")
    for call, entry in ((lambda s: s.pmin(d, d), "C_pminmax_SVT1_SVT2"), (lambda s: s.pmax(d, 0.0), "C_pminmax_SVT1_v2"),
                        (lambda s: s.is_na(d), "C_SVT_apply_isFUN"), (lambda s: s.sweep(d, 2, np.ones(29), "pmin"), "C_sweep_SVT")):
        with pytest.raises(SparseArrayUnsupported, match=f"{entry} is not offered"):
            call(oracle)


# ---------------------------------------------------------------------------
# queries that need no GPU
# ---------------------------------------------------------------------------
def test_out_type_query_is_the_wider_of_the_two():
    from sparsearray_amd._hip import load_library
    lib = load_library()
    R = {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}
    for tx in pc.TYPES:
        for ty in pc.TYPES:
            assert lib.svt_dev_pminmax_out_Rtype(R[tx], R[ty]) == R[pc.out_type(tx, ty)]
        assert lib.svt_dev_pminmax_out_Rtype(R[tx], 16) == 0 and lib.svt_dev_pminmax_out_Rtype(15, R[tx]) == 0
