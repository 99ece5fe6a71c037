"""The seeded random cases of tests/random_cases.py without a GPU: the same seeds through the oracle session where it
offers the operation (subset, medians, quantiles, MADs, ranks) -- generator and dense expectation are validated against
an independent implementation -- and, for Arith / Math, which the oracle session does not offer, the structural claims of
the generator: pairs straddle a tile boundary, the weakest comparison class stays rare, every result type occurs.

The 40 000-row operands of the order statistics are run here as well (two columns each: a second or two in all).

tests/random_cases.py draws nine families; the five later ones -- Compare / Logic, sweep(), pmin / pmax and is*(),
subassignment by N-index, the L-index and M-index -- have their twin in tests/test_zzzzzzzzzzz_random_cases_cpu.py, which
stands last in the suite's order."""
import numpy as np
import pytest

import arith_cases as ac
import random_cases as rc
import subset_cases as sc
from helpers import assert_equal


@pytest.fixture(scope="module")
def tiles():
    return rc.tiles()


def _one_based(v):
    return None if v is None else (np.asarray(v, dtype=np.int64) + 1).astype(np.int32)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_subset_seed_through_the_oracle(oracle, tiles, seed):
    c = rc.SubsetCase(seed, tiles[0])
    x = rc.svt_of(c.nrow, c.type, c.cp, c.ri, c.val)
    for rows, cols in c.calls:
        want = c.expected((rows, cols))
        res = oracle.subset(x, _one_based(rows), _one_based(cols))
        assert res.type == c.type and res.dim == (c.nrow if rows is None else rows.size, c.lens.size if cols is None else cols.size)
        rc.same_csc(res.to_csc(), want, f"seed {seed} rows {None if rows is None else rows.size} cols {None if cols is None else cols.size}")


def test_subset_seeds_cover_what_the_generator_names(tiles):
    T = tiles[0]
    cases = [rc.SubsetCase(s, T) for s in rc.SEEDS]
    assert {c.type for c in cases} == set(rc.SUBSET_TYPES)
    assert {k for c in cases for k in c.row_kinds} == set(rc.ROW_KINDS) - {"none"} or \
        {k for c in cases for k in c.row_kinds} == set(rc.ROW_KINDS)
    assert {c.col_kind for c in cases} == set(rc.COL_KINDS) - {"none"}
    assert len({c.lens.size for c in cases}) >= 3 and any(c.lens.max() == c.nrow for c in cases)
    assert any(c.lens.max() >= 0.5 * c.total for c in cases if c.lens.size > 1)
    for c in cases:
        assert c.total in (T - 1, T, T + 1, 2 * T, 2 * T + 1) or 0 < abs(c.total - 3 * T) < 200
        assert c.lens.sum() == c.total == c.ri.size and c.nrow >= c.lens.max()
    # a repeated empty column in front of entries, and an empty run of more columns than a workgroup has threads
    assert any(c.col_kind == "repeats" and (c.lens == 0).any() for c in cases)
    assert any(np.diff(np.flatnonzero(np.concatenate([[1], c.lens, [1]]))).max() > 256 for c in cases)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_arith_seed_is_consistent(tiles, seed):
    """the expectation of every call computed, and met by itself placed as a CSC result; at most 1 % of the stored
    results of any call in the class where only NaN-ness is compared"""
    c = rc.ArithCase(seed, tiles[1])
    for call in c.calls:
        keys, e, _ = c.expected(call)
        at = e.stored
        assert at.any() or c.merged < 10 or call[1] != "neg"
        any_nan = int((e.cls[at] == ac.ANY_NAN).sum())
        assert any_nan <= 0.01 * max(int(at.sum()), 1), f"seed {seed} {call[0]}: {any_nan} of {int(at.sum())} results are ANY_NAN"
        cp, ri, val = ac._csc(keys[at], e.dense[at], c.nrow, c.ncol)
        c.compare(call, ((cp, ri, val), e.overflow))
        if at.sum() > 1:                                    # and the comparison rejects a dropped entry
            with pytest.raises(AssertionError):
                c.compare(call, (ac._csc(keys[at][1:], e.dense[at][1:], c.nrow, c.ncol), e.overflow))


def test_arith_seeds_cover_what_the_generator_names(tiles):
    T = tiles[1]
    cases = [rc.ArithCase(s, T) for s in rc.SEEDS]
    assert {c.types for c in cases} == set(rc.TYPE_PAIRS)
    assert sum(c.pairs_straddling_a_tile() >= 1 for c in cases) >= len(cases) // 2
    types = {c.expected(call)[1].type for c in cases for call in c.calls}
    assert types == {"double", "integer"}
    assert any(c.expected(call)[1].overflow for c in cases for call in c.calls)
    assert len({c.share for c in cases}) >= 3 and {k for c in cases for _, k, _ in c.calls} == {"merge", "scalar", "neg", "math"}
    for c in cases:
        assert c.merged in (T - 1, T, T + 1, 2 * T, 2 * T + 1) or 0 < abs(c.merged - 3 * T) < 200
        both = np.intersect1d(c.kx, c.ky).size
        assert abs(both - c.share * c.ky.size) <= 0.02 * c.ky.size + 1


@pytest.mark.parametrize("tall", [False, True])
@pytest.mark.parametrize("seed", rc.SEEDS)
def test_order_statistics_seed_through_the_oracle(oracle, seed, tall):
    c = rc.OrderStatCase(seed, tall)
    x = c.svt()
    for call in c.calls:
        _, f, na_rm = call
        want = c.expected(call)
        if f == "colmedians":
            got = oracle.colMedians(x, na_rm=na_rm)
        elif f == "colquantiles":
            got = oracle.colQuantiles(x, c.probs, na_rm=na_rm)
        else:
            got = oracle.colMads(x, center=c.center if f == "colmads_center" else None, na_rm=na_rm)
        assert_equal(got, want, tol=0, strict_na=True, what=f"seed {seed} {call[0]}")


def test_order_statistics_seeds_cover_what_the_generator_names():
    cases = [rc.OrderStatCase(s) for s in rc.SEEDS]
    assert {c.type for c in cases} == {"double", "integer"}
    for c in cases:
        assert sorted(c.classes) == sorted(rc.CLASSES * 2) and c.nrow == 5000 and 1 <= len(c.probs) <= 7
        lens = np.diff(c.cp)
        few = [j for j, k in enumerate(c.classes) if k == "few_distinct" and lens[j] == 5000]
        for j in few:
            assert np.unique(c.dense[:, j], return_counts=True)[1].max() > 1024
        assert np.isnan(c.dense).any() and ((c.val == 0).any())
        assert not np.isfinite(c.center).all()
    assert any(rc.OrderStatCase(s, True).nrow == 40_000 for s in rc.SEEDS)
    assert len({len(c.probs) for c in cases}) >= 3 and len({np.diff(c.cp)[j] for c in cases for j in range(16)}) == 4


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_ranks_seed_through_the_oracle(oracle, tiles, seed):
    c = rc.RanksCase(seed, tiles[2])
    x = c.svt()
    for call in c.calls:
        got = oracle.colRanks(x, ties_method=call[1], preserve_shape=True)
        assert_equal(got, c.expected(call), tol=0, strict_na=True, what=f"seed {seed} {call[0]}")


def test_ranks_seeds_cover_what_the_generator_names(tiles):
    f0, f1 = tiles[2]
    cases = [rc.RanksCase(s, tiles[2]) for s in rc.SEEDS]
    assert {c.type for c in cases} == {"double", "integer"} and {c.stored_zeros for c in cases} == {False, True}
    assert {(c.type, c.stored_zeros) for c in cases} == {(t, z) for t in ("double", "integer") for z in (False, True)}
    for c in cases:
        lens = np.diff(c.cp).tolist()
        assert {f0, f0 + 1, f1} <= set(lens) and lens.count(f1 + 1) <= 1 and max(lens) <= f1 + 1 <= c.nrow <= f1 + 3000
        assert c.stored_zeros == bool((c.val == 0).any())
    assert any(f1 + 1 in np.diff(c.cp) for c in cases)
    # the compact form of the dense ranks expands to them (the expansion the GPU test uses)
    c = cases[1]
    r = c.expected(c.calls[0])
    col = np.repeat(np.arange(c.cp.size - 1), np.diff(c.cp))
    zero = np.array([r[np.flatnonzero(c.dense[:, j] == 0)[0], j] for j in range(c.cp.size - 1)], dtype=r.dtype)
    assert np.array_equal(c.expand(r[c.ri, col], zero), r)
