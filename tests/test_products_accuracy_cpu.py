"""The product rules of exact_products.py on the CPU: the checker verified by hand, the reference held to every rule on
every case of product_cases.py (the bounds are theorems about any order of the additions, the reference's included),
and what the rules reject that the bar of the oracle-parity tests, assert_equal(tol=1e-9, atol=1e-11), accepts."""
from fractions import Fraction

import numpy as np
import pytest

import exact_products as xp
import product_cases as pc
from helpers import assert_equal


def test_checker_by_hand():
    """x = [[.1, 0], [0, -4], [.2, 0]] (3 x 2), Y = [3, 7, .3]': cell 0 = fl(.1) 3 + fl(.2) fl(.3) (n = 2), cell 1 = -28
    (n = 1); a third, empty leaf has n = 0."""
    cp, ri, val = np.array([0, 2, 3, 3]), np.array([0, 2, 1]), np.array([0.1, 0.2, -4.0])
    Y = np.array([[3.0], [7.0], [0.3]])
    p = xp.exact_sparse_dense(cp, ri, val, Y)
    E = [Fraction(0.1) * 3 + Fraction(0.2) * Fraction(0.3), Fraction(-28), Fraction(0)]
    M = [Fraction(0.1) * 3 + Fraction(0.2) * Fraction(0.3), Fraction(28), Fraction(0)]
    assert p.E.to_fractions() == E and p.M.to_fractions() == M and list(p.n) == [2, 1, 0] and p.shape == (3, 1)
    good = np.array([[0.1 * 3 + 0.2 * 0.3], [-28.0], [0.0]])
    v = xp.check_product(good, p)
    assert v.ok and v.ncompared == 2
    # the bound of cell 0 is gamma(2) M = 2 u / (1 - 2 u) * 0.36 = 8e-17: one ulp of 0.36 (5.6e-17) from the exact value
    # may pass, three ulps (1.7e-16) cannot; cell 1 is a single exact product: gamma(1) * 28 = 3.1e-15 < ulp(28)
    e0 = float(E[0])
    far = np.nextafter(np.nextafter(np.nextafter(e0, 1), 1), 1)
    assert abs(Fraction(far) - E[0]) > Fraction(2, 2 ** 53 - 2) * M[0]
    assert not xp.check_product(np.array([[far], [-28.0], [0.0]]), p).ok
    assert not xp.check_product(np.array([[e0], [np.nextafter(-28.0, 0)], [0.0]]), p).ok
    assert xp.check_product(np.array([[e0], [-28.0], [-0.0]]), p).ok
    with pytest.raises(AssertionError, match="exactly zero"):
        xp.check_product(np.array([[e0], [-28.0], [1e-300]]), p)
    with pytest.raises(AssertionError, match="non-finite"):
        xp.check_product(np.array([[np.inf], [-28.0], [0.0]]), p)
    # the sparse x sparse form of the same cells: crossprod(x, y), y = Y as a one-column sparse operand
    q = xp.exact_sparse_sparse(3, (cp, ri, val), (np.array([0, 3]), np.array([0, 1, 2]), Y[:, 0]))
    assert q.E.to_fractions() == E and list(q.n) == [2, 1, 0]
    # ... and with a hole in y at row 2: only the rows both hold count
    q = xp.exact_sparse_sparse(3, (cp, ri, val), (np.array([0, 2]), np.array([0, 1]), Y[:2, 0]))
    assert q.E.to_fractions() == [Fraction(0.1) * 3, Fraction(-28), Fraction(0)] and list(q.n) == [1, 1, 0]
    # integers: identity
    pi = xp.exact_sparse_dense(cp, ri, np.array([2, 3, -4], dtype=np.int32), np.array([[5.0], [7.0], [11.0]]))
    assert xp.exact_int(pi).tolist() == [[43], [-28], [0]]
    xp.check_identical_product(np.array([[43.0], [-28.0], [0.0]]), xp.exact_int(pi))
    with pytest.raises(AssertionError, match="differ from the exact integer"):
        xp.check_identical_product(np.array([[43.0], [-27.0], [0.0]]), xp.exact_int(pi))
    E2, M2, n2 = xp.tracer_sparse_dense(cp, ri, np.array([2.0, 3.0, -4.0]), np.array([[5.0], [7.0], [11.0]]))
    assert E2.tolist() == [[43], [-28], [0]] and M2.tolist() == [[43], [28], [0]] and n2.tolist() == [[2], [1], [0]]


def test_tracer_tells_neighbours_apart():
    """A record against the next row, or attributed to the next column of its group, changes the integer."""
    st = pc.structure("small257")
    y = pc.tracer_y(st.nrow, 3)
    assert np.all(y[1:] != y[:-1])
    a = pc.tracer_a(st.ri, st.leaf)
    assert np.all(a != 0) and np.all(np.abs(a) <= 31)
    assert np.all(pc.tracer_a(st.ri, st.leaf + 1) != a)


@pytest.mark.parametrize("name", list(pc.DENSE_CASES))
def test_reference_meets_the_rules_sparse_dense(oracle, name):
    pc.run_dense_case_oracle(oracle, name)


@pytest.mark.parametrize("case", pc.HOST_CASES, ids=lambda c: "-".join(c))
def test_reference_meets_the_rules_host_entry_points(oracle, case):
    pc.run_host_case(oracle, *case)


@pytest.mark.parametrize("name", list(pc.NONFINITE_CASES))
@pytest.mark.parametrize("saturated", [False, True])
def test_reference_meets_the_nonfinite_rule(oracle, name, saturated):
    st, val, Y = pc.nonfinite_operands(name, saturated)
    want = np.asarray(oracle.crossprod(pc.svt_of(st, val), np.asfortranarray(Y)))
    assert np.any(~np.isfinite(want)) and np.any(np.isfinite(want))
    v = xp.check_with_nonfinite(want, want, st.cp, st.ri, val, Y).require()
    assert v.ncompared > 0
    # a finite cell turned NaN, and a NaN turned NA, are both refused
    bad = want.copy()
    bad[np.unravel_index(np.flatnonzero(np.isfinite(want))[0], want.shape)] = np.nan
    with pytest.raises(AssertionError, match="non-finite cells"):
        xp.check_with_nonfinite(bad, want, st.cp, st.ri, val, Y)
    plain_nan = np.isnan(want) & ~xp.is_NA_real(want)
    assert np.any(plain_nan)
    bad = want.copy()
    bad[np.unravel_index(np.flatnonzero(plain_nan)[0], want.shape)] = pc.NA_real
    with pytest.raises(AssertionError, match="NA / NaN class"):
        xp.check_with_nonfinite(bad, want, st.cp, st.ri, val, Y)
    if not saturated:                                       # (the planted NA: turned into a plain NaN)
        na = xp.is_NA_real(want)
        assert np.any(na)
        bad = want.copy()
        bad[np.unravel_index(np.flatnonzero(na)[0], want.shape)] = np.nan
        with pytest.raises(AssertionError, match="NA / NaN class"):
            xp.check_with_nonfinite(bad, want, st.cp, st.ri, val, Y)


@pytest.mark.parametrize("types", pc.TYPE_PAIRS, ids="-".join)
@pytest.mark.parametrize("nrow", pc.MATMUL_ROWS)
def test_reference_meets_the_rules_sparse_matmul(oracle, nrow, types):
    pc.run_matmul_case(pc.oracle_matmul(oracle), nrow, types)


@pytest.mark.parametrize("types", pc.TYPE_PAIRS, ids="-".join)
@pytest.mark.parametrize("name", list(pc.GRAM_ROWS))
def test_reference_meets_the_rules_sparse_crossprod(oracle, name, types):
    pc.run_gram_case(pc.oracle_gram(oracle), name, types)
    if types[0] == types[1]:
        pc.run_gram_case(pc.oracle_gram(oracle), name, types, sym=True)


def test_sparse_crossprod_cases_cover_the_lane_group_widths():
    """The general and the symmetric form, one block and panels, each at G = 8, 16 and 32: gram_operands asserts the
    width of every case by launch_gram's own arithmetic, and together the cases leave no combination out."""
    covered = set()
    for name, g in pc.GRAM_ROWS.items():
        pc.gram_operands(name)
        covered |= set(g["G"].items())
    assert covered == {(f"{form} {blocking}", G) for form in ("gen", "sym") for blocking in ("one", "pan")
                       for G in (8, 16, 32)}
    # the arithmetic itself, by hand: 700 columns in panels of 64 are 11 panels; 22400 nonzeros on 160 rows walk 140
    assert pc.gram_lane_group(22400, 160, 700, False, -1, -1) == 32
    assert pc.gram_lane_group(22400, 160, 700, False, 0, 6) == 8           # 140 / 11 = 12.7
    assert pc.gram_lane_group(22400, 160, 700, True, -1, -1) == 32         # 70
    assert pc.gram_lane_group(22400, 160, 700, False, 0, 8) == 16          # 140 / 3 = 46.7
    assert pc.gram_lane_group(10080, 160, 700, True, -1, -1) == 8          # 63 / 2 = 31.5


# ---------------------------------------------------------------------------
# mutants: wrong results that assert_equal(tol=1e-9, atol=1e-11) accepts and the rules refuse
# ---------------------------------------------------------------------------
def _cell(st, val, Y, c, k, drop=None, double=None, shift=None, f32=False):
    """Cell (c, k) added in the reference's order, with one defect."""
    lo, hi = int(st.cp[c]), int(st.cp[c + 1])
    acc = np.float32(0.0) if f32 else 0.0
    for i in range(lo, hi):
        if i == drop:
            continue
        r = int(st.ri[i]) + (1 if i == shift else 0)
        t = val[i] * Y[r, k]
        acc = np.float32(acc + np.float32(t)) if f32 else acc + t
        if i == double:
            acc = acc + t
    return float(acc)


def _both_halves(mutant, want, p, what):
    assert_equal(mutant, want, tol=1e-9, atol=1e-11, what=what)            # the old bar lets it through
    assert not xp.check_product(mutant, p, what).ok, f"{what}: the rule lets the mutant through"


def test_mutants_pass_the_old_bar_and_fail_the_rules(oracle):
    st = pc.structure("small383")
    K = 3

    def reference(val, Y):
        want = np.asarray(oracle.crossprod(pc.svt_of(st, val), np.asfortranarray(Y)))
        p = xp.exact_sparse_dense(st.cp, st.ri, val, Y)
        xp.check_product(want, p, "reference").require()
        return want, p

    # 1. the cells of the 2**-60 leaves never written
    val, Y = pc.palette(st, "tiny_leaves", K)
    want, p = reference(val, Y)
    m = want.copy()
    m[::3, :] = 0.0
    assert np.any(want[::3, :] != 0)
    _both_halves(m, want, p, "tiny leaves left at zero")
    # 5. a float32 accumulator for one cell (of a tiny leaf: far below the old bar's absolute floor)
    c = next(c for c in range(0, st.ncol, 3) if st.cp[c + 1] - st.cp[c] >= 8)
    m = want.copy()
    m[c, 1] = _cell(st, val, Y, c, 1, f32=True)
    assert m[c, 1] != want[c, 1]
    _both_halves(m, want, p, "float32 accumulator")
    # 2. the smallest-magnitude term of a leaf dropped, 4. a record doubled: one value of a leaf scaled by 2**-37, its
    # term is then ~1e-11 of the cell -- below the old bar, five orders above gamma(n) M
    val, Y = pc.palette(st, "full", K)
    c = next(c for c in range(st.ncol) if st.cp[c + 1] - st.cp[c] >= 8)
    lo, hi = int(st.cp[c]), int(st.cp[c + 1])
    i = lo + 3
    val[i] = np.sign(val[i]) * 2.0 ** -37
    assert lo + int(np.argmin(np.abs(val[lo:hi] * Y[st.ri[lo:hi], 0]))) == i
    want, p = reference(val, Y)
    m = want.copy()
    m[c, 0] = _cell(st, val, Y, c, 0, drop=i)
    _both_halves(m, want, p, "the smallest term dropped")
    m = want.copy()
    m[c, 0] = _cell(st, val, Y, c, 0, double=i)
    _both_halves(m, want, p, "a record doubled")
    # 3. one record taken against row r + 1, where Y[r + 1] is close to Y[r]
    val, _ = pc.palette(st, "full", K)
    Y = (1.0 + np.arange(st.nrow) * 2.0 ** -34)[:, None] * np.array([[1.5, -0.7, 3.1]])
    want, p = reference(val, Y)
    c = next(c for c in range(st.ncol) if st.cp[c + 1] - st.cp[c] >= 4 and abs(want[c, 0]) > 0.5)
    i = next(i for i in range(int(st.cp[c]), int(st.cp[c + 1])) if abs(val[i]) > 0.5 and st.ri[i] + 1 < st.nrow)
    m = want.copy()
    m[c, 0] = _cell(st, val, Y, c, 0, shift=i)
    assert m[c, 0] != want[c, 0]
    _both_halves(m, want, p, "a record against the next row")
    # and the tracer: each defect changes the integer
    val, Y = pc.palette(st, "tracer", K)
    E, _, _ = xp.tracer_sparse_dense(st.cp, st.ri, val, Y)
    xp.check_identical_product(np.asarray(oracle.crossprod(pc.svt_of(st, val), np.asfortranarray(Y))), E)
    for kw in (dict(drop=i), dict(double=i), dict(shift=i)):
        m = E.astype(np.float64)
        m[c, 0] = _cell(st, val, Y, c, 0, **kw)
        with pytest.raises(AssertionError, match="differ from the exact integer"):
            xp.check_identical_product(m, E)
