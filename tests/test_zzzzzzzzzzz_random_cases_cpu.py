"""The seeded random cases of tests/random_cases.py for the five families on the merge, map and sweep tile kernels --
Compare / Logic, sweep(), pmin / pmax and is*(), subassignment by N-index, the L-index and M-index -- without a GPU (the
four earlier families: tests/test_random_cases_cpu.py).  The oracle session offers none of the five, so what is checked
are the structural claims of the generator: the expectation of every call is computed and met by itself placed as a CSC
result, it agrees with a second statement where the family's case module has one (pminmax_cases.steps, numpy's own
indexing on the dense array, lindex_cases.dense_*), the comparison rejects a dropped entry and a changed value, and over
the eight seeds every condition the generator names occurs -- pairs straddle a tile boundary and are dropped there, a
tile spans hundreds of leaves, both routes of the placement are taken, the weakest comparison class stays rare, every
type pair and operation occurs.  Each ``..._cover_what_the_generator_names`` test prints the table of which seed meets
which condition (``pytest -s``).

The module stands last in the suite's order, like every module added since the suite grew long: the tests in front of
it keep their places in a run."""
import numpy as np
import pytest

import arith_cases as ac
import compare_cases as cc
import lindex_cases as lc
import pminmax_cases as pc
import random_cases as rc
import subassign_cases as sa
import subset_cases as sc
import sweep_cases as sw


@pytest.fixture(scope="module")
def tiles():
    return rc.tiles()


@pytest.fixture(scope="module")
def more_tiles():
    return rc.more_tiles()


def _table(family, rows):
    """prints which seed meets which condition; returns the columns as lists"""
    names = list(rows[0])
    print(f"\n{family}: conditions met per seed")
    print("seed  " + "  ".join(names))
    for seed, row in zip(rc.SEEDS, rows):
        print(f"{seed:4d}  " + "  ".join(str(row[n]).rjust(len(n)) for n in names))
    return {n: [row[n] for row in rows] for n in names}


def _rejects_a_dropped_entry_and_a_changed_value(same, want, ncol):
    """``same(got)`` asserts got against want: it must refuse want without its first entry and want with one value
    changed"""
    cp, ri, val = want
    if ri.size == 0:
        return
    first = int(np.repeat(np.arange(ncol), np.diff(cp))[0])
    less = cp.copy()
    less[first + 1:] -= 1
    with pytest.raises(AssertionError):
        same((less, ri[1:], val[1:]))
    other = val.copy()
    other[-1] = 5 if other[-1] != 5 else 6
    with pytest.raises(AssertionError):
        same((cp, ri, other))


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_compare_seed_is_consistent(tiles, seed):
    c = rc.CompareCase(seed, tiles[1])
    for call in c.calls:
        want = c.expected(call)
        assert want[2].dtype == np.int32 and np.all((want[2] == 1) | (want[2] == cc.NA)), call[0]
        assert np.isin(rc.keys_of(want, c.nrow), c.kx if call[1] == "scalar" else np.union1d(c.kx, c.ky)).all()
        rc.same_csc(want, c.expected(call), call[0])
        _rejects_a_dropped_entry_and_a_changed_value(lambda got: rc.same_csc(got, want, call[0]), want, c.ncol)
        if call[1] == "scalar":                             # the scalar keeps the rule: 0 op s is FALSE
            op, s, st = call[2]
            assert cc.compare_values(op, np.zeros(1, np.int32), cc.scalar_value(s, st))[0] == 0, call[0]
    op, s, st = c.refused
    assert cc.compare_values(op, np.zeros(1, np.int32), cc.scalar_value(s, st))[0] != 0, c.refused


def test_compare_seeds_cover_what_the_generator_names(tiles):
    T = tiles[1]
    cases = [rc.CompareCase(s, T) for s in rc.SEEDS]
    rows = []
    for c in cases:
        kept = [rc.keys_of(c.expected(call), c.nrow).size / max(c.positions(call), 1) for call in c.calls]
        rows.append({"types": "/".join(t[:3] for t in c.types), "share": c.share, "equal": c.equal, "merged": c.merged,
                     "straddling": c.pairs_straddling_a_tile(),
                     "dropped_at_edge": max(c.straddling_pairs_dropped(call) for call in c.calls if call[1] != "scalar"),
                     "least_kept": round(min(kept), 3), "most_kept": round(max(kept), 3)})
    col = _table("Compare / Logic", rows)
    assert {c.types for c in cases} == set(rc.COMPARE_TYPE_PAIRS) and sum(c.types == ("logical", "logical") for c in cases) >= 2
    assert {t for c in cases for t in c.types} == {"double", "integer", "logical"}
    for c in cases:
        ops = [(k, a if k != "scalar" else a[0]) for _, k, a in c.calls]
        assert {o for k, o in ops if k == "merge"} == set(cc.MERGE_OPS) and {o for k, o in ops if k == "scalar"} == set(cc.COMPARE_OPS)
        assert ({o for k, o in ops if k == "logic"} == set(cc.LOGIC_OPS)) == (c.types == ("logical", "logical"))
        assert c.merged in (T - 1, T, T + 1, 2 * T, 2 * T + 1) or 0 < abs(c.merged - 3 * T) < 200
        assert abs(np.intersect1d(c.kx, c.ky).size - c.share * c.ky.size) <= 0.02 * c.ky.size + 1
    assert {c.share for c in cases} == set(rc.SHARES) and {st for c in cases for _, k, a in c.calls if k == "scalar" for st in [a[2]]} == \
        {"double", "integer", "logical"}
    assert sum(n >= 1 for n in col["straddling"]) >= len(cases) // 2
    assert any(n >= 1 for n in col["dropped_at_edge"])
    assert min(col["least_kept"]) < 0.05 and max(col["most_kept"]) > 0.95


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_pminmax_seed_is_consistent(tiles, seed):
    c = rc.PminmaxCase(seed, tiles[1])
    for call in c.calls:
        want, t = c.expected(call)
        assert want[2].dtype == pc.np_dtype(t) and np.all(pc.kept(want[2])), call[0]
        pc.same(want, c.expected(call)[0], call[0])
        _rejects_a_dropped_entry_and_a_changed_value(lambda got: pc.same(got, want, call[0]), want, c.ncol)
        if call[1] == "isfun" and call[2] != "is.na" and c.types[0] != "double":
            assert want[1].size == 0, call[0]
        if call[1] == "merge" and c.merged <= 3 * tiles[1]:     # the other statement of the rule, step by step
            op, na_rm = call[2]
            keys = np.union1d(c.kx, c.ky)
            dx, dy = np.zeros(keys.size, c.vx.dtype), np.zeros(keys.size, c.vy.dtype)
            dx[np.searchsorted(keys, c.kx)], dy[np.searchsorted(keys, c.ky)] = c.vx, c.vy
            v = pc.steps(op, na_rm, dx, dy, t)
            assert np.array_equal(pc.bits(v[pc.kept(v)]), pc.bits(want[2])), call[0]


def test_pminmax_seeds_cover_what_the_generator_names(tiles):
    T = tiles[1]
    cases = [rc.PminmaxCase(s, T) for s in rc.SEEDS]
    rows = []
    for c in cases:
        isf = {call[2]: c.expected(call)[0][1].size for call in c.calls if call[1] == "isfun"}
        rows.append({"types": "/".join(t[:3] for t in c.types), "share": c.share, "merged": c.merged,
                     "straddling": c.pairs_straddling_a_tile(), "is.na": isf["is.na"], "is.nan": isf["is.nan"],
                     "is.infinite": isf["is.infinite"],
                     "scalar_types": "".join(sorted({a[3][0] for _, k, a in c.calls if k == "scalar"}))})
    col = _table("pmin / pmax / is*()", rows)
    assert {c.types for c in cases} == set(rc.PMINMAX_TYPE_PAIRS) and {t for c in cases for t in c.types} == set(pc.TYPES)
    for c in cases:
        assert {a for _, k, a in c.calls if k == "merge"} == set(rc.PMINMAX_VARIANTS)
        assert {a[:2] for _, k, a in c.calls if k == "scalar"} == set(rc.PMINMAX_VARIANTS)
        assert {a for _, k, a in c.calls if k == "isfun"} == set(pc.ISFUNS)
        assert c.merged in (T - 1, T, T + 1, 2 * T, 2 * T + 1) or 0 < abs(c.merged - 3 * T) < 200
    assert {c.share for c in cases} == set(rc.SHARES) and any(n >= 1 for n in col["straddling"])
    assert set("".join(col["scalar_types"])) == {"d", "i", "l"}
    for c, nan, inf in zip(cases, col["is.nan"], col["is.infinite"]):
        assert (nan > 0 and inf > 0) if c.types[0] == "double" else (nan == 0 and inf == 0), c.seed


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_sweep_seed_is_consistent(tiles, seed):
    """as for Arith: at most 1 % of the stored results of a call in the class where only NaN-ness is compared"""
    from test_hip_arith import MAX_ULPS
    c = rc.SweepCase(seed, tiles[1])
    assert c.lens.sum() == c.total == c.ri.size and int(np.prod(c.dim[1:])) == c.ncol
    for call in c.calls:
        want, cls, t, over = c.expected(call)
        what = f"seed {seed}: {call[0]}"
        if cls is None:
            pc.same(want, c.expected(call)[0], what)
            _rejects_a_dropped_entry_and_a_changed_value(lambda got: pc.same(got, want, what), want, c.ncol)
        else:
            assert int((cls == ac.ANY_NAN).sum()) <= 0.01 * max(cls.size, 1), what
            ulps = MAX_ULPS["^"] if call[2] == "^" else 0
            rc.same_csc_by_class(want, want, cls, what, ulps)
            _rejects_a_dropped_entry_and_a_changed_value(lambda got: rc.same_csc_by_class(got, want, cls, what, ulps), want, c.ncol)
    (name, rule, op, na_rm, st, bad), first = c.refused
    good = next(call for call in c.calls if call[0] == name)[5]
    assert np.flatnonzero(sc.bits(bad) != sc.bits(good)).min() == first


def test_sweep_seeds_cover_what_the_generator_names(tiles):
    T = tiles[1]
    cases = [rc.SweepCase(s, T) for s in rc.SEEDS]
    rows = []
    for c in cases:
        tl = c.tiles()
        rows.append({"type": c.type[:3], "dim": "x".join(map(str, c.dim)), "margin": ",".join(map(str, c.margin)),
                     "with_rows": c.with_rows, "stride": c.stride, "len": c.len, "recycles": c.len < c.ncol // c.stride,
                     "tile_in_one_leaf": any(q0 == q1 for q0, q1, _, _ in tl),
                     "most_leaf_starts": max(n for _, _, n, _ in tl), "starts_behind_empty": any(a for _, _, _, a in tl),
                     "ops": " ".join(f"{call[2]}:{call[4][0]}" for call in c.calls)})
    col = _table("sweep()", rows)
    calls = [call for c in cases for call in c.calls]
    assert {call[2] for call in calls} == set(sw.ARITH_OPS) | set(sw.COMPARE_OPS) | {"pmin", "pmax"}
    assert {(call[2], call[3]) for call in calls if call[1] == "pminmax"} == set(rc.PMINMAX_VARIANTS)
    assert {call[4] for call in calls if call[1] == "arith"} == {"double", "integer"}
    assert {call[4] for call in calls if call[1] != "arith"} == {"double", "integer", "logical"}
    assert {c.type for c in cases} == {"double", "integer"} and {len(c.dim) for c in cases} >= {2, 3, 4}
    assert {c.refused[0][1] for c in cases} == {"arith", "compare", "pminmax"}
    assert set(col["with_rows"]) == {0, 1} and max(col["stride"]) > 1 and any(col["recycles"])
    assert any(col["tile_in_one_leaf"]) and max(col["most_leaf_starts"]) > 256 and any(col["starts_behind_empty"])
    for c in cases:
        assert c.total in (T - 1, T, T + 1, 2 * T, 2 * T + 1) or 0 < abs(c.total - 3 * T) < 200


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_subassign_seed_is_consistent(tiles, more_tiles, seed):
    c = rc.SubassignCase(seed, tiles[1], more_tiles[0])
    for call in c.calls:
        want, t = c.expected(call)
        what = f"seed {seed}: {call[0]}"
        assert want[2].dtype == sc.NP_DTYPE[t] and t == sa.wider(*c.types), what
        rc.same_csc(want, c.expected(call)[0], what)
        _rejects_a_dropped_entry_and_a_changed_value(lambda got: rc.same_csc(got, want, what), want, c.ncol)
        # numpy's own statement on the dense array, where the subscripts have no repeats
        name, rows, leaves, value = call
        if name in ("delete", "scalar", "empty_cover") and c.nrow * c.ncol <= rc.CELLS:
            r = np.arange(c.nrow) if rows is None else rows
            q = np.arange(c.ncol) if leaves is None else leaves
            if np.unique(r).size == r.size:
                dense = np.zeros((c.nrow, c.ncol), sc.NP_DTYPE[t], order="F")
                stored = np.zeros((c.nrow, c.ncol), bool, order="F")
                col = np.repeat(np.arange(c.ncol), c.lens)
                dense[c.ri, col], stored[c.ri, col] = sa.widen(c.val, c.types[0], t), True
                if r.size and q.size:
                    v = sa.widen(value, c.types[1], t)[np.arange(r.size) % value.size]
                    dense[np.ix_(r, q)] = v[:, None]
                    stored[:, q] = (dense[:, q] != 0) | (dense[:, q] != dense[:, q])
                at = np.flatnonzero(stored.reshape(-1, order="F"))
                assert np.array_equal(at, rc.keys_of(want, c.nrow)), what
                assert np.array_equal(sc.bits(dense.reshape(-1, order="F")[at]), sc.bits(want[2])), what


def test_subassign_seeds_cover_what_the_generator_names(tiles, more_tiles):
    T, P = tiles[1], more_tiles[0]
    cases = [rc.SubassignCase(s, T, P) for s in rc.SEEDS]
    rows = []
    for c in cases:
        by = {call[0]: call for call in c.calls}
        deleted = c.total + 0 - rc.keys_of(c.expected(by["delete"])[0], c.nrow).size
        rows.append({"types": "/".join(t[:3] for t in c.types), "rows": c.row_kind, "leaves": c.leaf_kind, "zeros": c.zeros,
                     "cover": c.cover, "pure_deletion": deleted > 0, "empty_Y_over_x": c.total > 0,
                     "no_entry_under_cover": c.entries_under(by["empty_cover"]) == 0,
                     "repeat_ends_in_zero": c.repeated_rows_ending_in_zero(by["vector"]) > 0,
                     "svt_entries": int(by["svt"][3][2].size)})
    col = _table("subassignment by N-index", rows)
    assert {c.types for c in cases} == set(rc.ASSIGN_TYPE_PAIRS)
    assert any(sa.wider(*c.types) != c.types[0] for c in cases) and any(sa.wider(*c.types) != c.types[1] for c in cases)
    assert {c.row_kind for c in cases} == set(rc.ASSIGN_ROW_KINDS) and {c.leaf_kind for c in cases} == set(rc.ASSIGN_LEAF_KINDS)
    assert {c.zeros for c in cases} == {0.0, 0.3, 1.0}
    for name in ("pure_deletion", "empty_Y_over_x", "no_entry_under_cover", "repeat_ends_in_zero"):
        assert any(col[name]), name
    for c in cases:
        assert c.cover in (P - 1, P, P + 1, 2 * P, 2 * P + 1) or 0 < abs(c.cover - 3 * P) < 200
        name, r, q, v = c.calls[-1]
        assert name == "svt" and np.all(np.diff(r) > 0) and np.unique(q).size == q.size and v[0] == r.size and v[1].size == q.size + 1
    assert all((c.calls[-1][3][3] == 0).any() for c in cases), "a value operand without a stored zero"
    assert any(np.any(np.diff(c.calls[-1][2]) < 0) for c in cases), "the leaves of every SVT form ascend"


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_cells_seed_is_consistent(tiles, more_tiles, seed):
    """lindex_cases' statement on the cells against its statement on the dense array, where there is one"""
    c = rc.CellIndexCase(seed, tiles[1], more_tiles[1])
    want = c.expected_assign()
    rc.same_cells(c.expected_assign(), want, f"seed {seed}")
    if want[1].size:
        with pytest.raises(AssertionError):
            rc.same_cells((want[0], want[1][1:], want[2][1:]), want, "a dropped entry")
        other = want[2].copy()
        other[0] = 5 if other[0] != 5 else 6
        with pytest.raises(AssertionError):
            rc.same_cells((want[0], want[1], other), want, "a changed value")
    g = c.expected_gather()
    assert g.size == c.gather.size and g.dtype == sc.NP_DTYPE[c.types[0]]
    if c.op.has_dense:
        assert np.array_equal(sc.bits(lc.dense_subset(c.op, c.gather)), sc.bits(g))
        t, flat, stored = lc.dense_subassign(c.op, c.L, c.value, c.types[1])
        assert t == want[0] and lc.same_as_dense(want[1], want[2], flat, stored)
    if c.with_mindex:
        M = lc.mindex_of(c.op.dim, c.L)
        back = sum(M[:, a].astype(np.int64) * int(np.prod(c.op.dim[:a], dtype=np.int64)) for a in range(len(c.op.dim)))
        assert np.array_equal(back, c.L)


def test_cells_seeds_cover_what_the_generator_names(tiles, more_tiles):
    T = tiles[1]
    cases = [rc.CellIndexCase(s, T, more_tiles[1]) for s in rc.SEEDS]
    rows = [{"types": "/".join(t[:3] for t in c.types), "dim": "x".join(map(str, c.op.dim)), "K": c.K, "index": c.L.size,
             "kind": c.kind, "nvals": c.value.size, "route": "sorted" if c.sorted_route else "sort", "passes": c.passes,
             "NA_in_gather": int((c.gather == lc.LINDEX_NA).sum()), "M_index": c.with_mindex,
             "last_deletes_stored": c.last_value_deletes_a_stored_entry()} for c in cases]
    col = _table("L-index / M-index", rows)
    assert {c.types for c in cases} == set(rc.ASSIGN_TYPE_PAIRS) and {c.kind for c in cases} == set(rc.CELL_KINDS)
    assert set(col["route"]) == {"sorted", "sort"} and len(set(col["passes"])) >= 2 and any(col["last_deletes_stored"])
    assert any(col["NA_in_gather"]) and any(col["M_index"]) and {len(c.op.dim) for c in cases} >= {2, 3}
    assert {1, 3} <= set(col["nvals"]) and any(c.value.size == c.L.size > 3 for c in cases)
    for c in cases:
        assert c.K in (1, 255, 256, 257) or 0 < abs(c.K - T) < 200 or c.K == c.op.ncells
        assert c.sorted_route == (c.kind == "increasing" or c.L.size == 1)
        if c.kind == "repeats":
            assert int((c.L == c.repeated).sum()) > T and c.value.size == c.L.size
