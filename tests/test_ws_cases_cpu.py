"""What tests/ws_cases.py claims, asserted without a GPU: the form every row case takes (through the host-only queries),
the panel arithmetic of the spmm and gram cases restated, the exactness of every sum, the leaf every flag placement
lies in -- and every case through the oracle, which pins the expectations the GPU half
(test_hip_ws_discipline.py) compares bits against."""
import numpy as np
import pytest

import product_cases as pc
import ws_cases as wc
from sparsearray_amd import NA_integer
from sparsearray_amd._hip import rowstats_form, rowsum_prepare_form, rowsum_prepared_form

LIMIT = 2 ** 53


def _cases(*entries):
    return [c["name"] for c in wc.CASES if c["entry"] in entries]


def test_the_table_is_well_formed():
    assert len(set(wc.NAMES)) == len(wc.NAMES)
    for c in wc.CASES:
        o = wc.other_case(c)
        assert o["entry"] == c["entry"] and o["name"] != c["name"] and "deg" not in o
    assert set(wc.ENTRIES) == {"gram", "spmm", "spmm_prepared", "rowsums", "rowsums_prepared", "rowstats", "colmedians",
                               "rowsum_prepared", "csc_dense", "pbc"}


def test_every_rowstats_form_has_an_operand():
    seen = set()
    for name, r in wc.ROW_OPERANDS.items():
        nrow, nleaf = r["dim"][0], int(np.prod(r["dim"][1:]))
        assert r["inner"] == int(np.prod(r["dim"][1:-1])) and nleaf % r["inner"] == 0
        for op, want in r["forms"].items():
            got = rowstats_form(nrow, nleaf, r["nnz"], op, r["inner"])
            assert got == want, f"{name}: a pass of {op} takes {got}, the table says {want}"
            seen.add(got[0])
        ops = r.get("ops", wc.ROW_OPS)
        assert all(p in r["forms"] for op in ops for p in wc.ROW_PASSES[op]), f"{name}: a pass without a stated form"
        if "var1" in ops:
            n = nleaf // r["inner"]
            assert n > 1 and n & (n - 1) == 0
    assert seen == {"pipe_units", "pipe", "whole_column", "panel", "memory_atomics"}
    assert any(r["forms"]["sum"][2] > 1 for r in wc.ROW_OPERANDS.values()), "no case adds strata ranges to a zeroed result"
    assert wc.ROW_OPERANDS["f4_atomics"]["inner"] > 65535 and wc.ROW_OPERANDS["f4_atomics"]["dim"][0] == 2


@pytest.mark.parametrize("name", _cases("rowsums", "rowsums_prepared", "rowstats"))
def test_row_case_operand(name):
    c = wc.BY_NAME[name]
    x = wc.operands(c)["A"]
    if "row" in c:
        r = wc.ROW_OPERANDS[c["row"]]
        assert (x.nrow, x.ncol, x.nnz) == (r["dim"][0], int(np.prod(r["dim"][1:])), r["nnz"])
    assert x.type == c["type"] and np.all(x.val != 0) and np.abs(x.val.astype(np.int64)).max(initial=0) <= 9
    _, big = wc.row_expected(x, c["inner"], c["op"], np.float64, parts=True)
    assert np.abs(big).max(initial=0) < LIMIT


def test_rowsum_id_forms():
    seen = set()
    for name in _cases("rowsum_prepared"):
        c = wc.BY_NAME[name]
        x = wc.operands(c)["A"]
        if "form" in c:
            got = rowsum_prepare_form(x.nrow, x.ncol, x.nnz, c["ngroup"])
            assert got == c["form"], f"{name}: the ids take {got}, the table says {c['form']}"
            seen.add(got[0])
        assert rowsum_prepared_form(x.ncol, c["ngroup"])[0]
        g, slot = wc.group_of(x.nrow, c["ngroup"])
        assert np.all((g == NA_integer) == (slot == c["ngroup"] - 1))
    assert seen == {"flat", "windowed"}


def _spmm_shape(nrow):
    """spmm_shape() of kernels_spmm.hip: panels of 8192 rows, shorter for operands a smaller power of two holds"""
    ps = 13
    while ps > 6 and (1 << ps) >= 2 * nrow:
        ps -= 1
    return ps, (nrow + (1 << ps) - 1) >> ps


@pytest.mark.parametrize("name", _cases("spmm", "spmm_prepared"))
def test_spmm_case(name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    A, B, B2 = o["A"], o["B"], o["B2"]
    assert (A.type, B.type, B2.type) == (c["types"][0], c["types"][1], c["types"][1])
    assert A.ncol == B.nrow == B2.nrow and B.ncol == B2.ncol
    if "deg" not in c:
        assert _spmm_shape(A.nrow) == (c["ps"], c["npan"])
        assert set(B.ri) == set(range(wc.SPMM_REFERENCED)) and B.ncol in (1, 16, 17)
        assert np.any(A.col >= wc.SPMM_REFERENCED), "no nonzero in a leaf B does not name"
        assert not np.array_equal(B.val, B2.val) or not np.array_equal(B.ri, B2.ri)
    assert (np.abs(A.dense()) @ np.abs(B.dense())).max(initial=0) < LIMIT
    assert (np.abs(A.dense()) @ np.abs(B2.dense())).max(initial=0) < LIMIT


def test_spmm_rows_sit_on_both_sides_of_the_one_split():
    assert _spmm_shape(8192) == (13, 1) and _spmm_shape(8193) == (13, 2)
    assert all(_spmm_shape(n)[1] == 1 for n in (1, 2, 63, 64, 65, 4096, 4097, 8191))


def _gram_blocking(nx, sym, panel):
    """(one block?, panels, cells of the last panel) of launch_gram under set_sparse_crossprod_panel(*panel)"""
    one_max, ps = pc.GRAM_PANEL_DEFAULT if panel is None else (min(panel[0], pc.GRAM_PANEL_DEFAULT[0]), panel[1])
    if nx <= (min(one_max, 16384) if sym else one_max):
        return True, 1, nx
    npan = (nx + (1 << ps) - 1) >> ps
    return False, npan, nx - ((npan - 1) << ps)


@pytest.mark.parametrize("name", _cases("gram"))
def test_gram_case(name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    X, Y = o["X"], o["Y"]
    assert (X.type, Y.type) == c["types"] and (Y is X) == c["sym"] and X.nrow == Y.nrow
    one, npan, last = _gram_blocking(X.ncol, c["sym"], c["panel"])
    if "route" in c:
        assert one == c["route"].endswith("one")
        if not one:
            assert (npan, last) == c["panels"]
        if c["route"] == "sym_one":
            assert c["middle_pairs_itself"] == (X.ncol % 2 == 1)        # columns j and nx - 1 - j share a workgroup
        # the lane-group width has no query: the arithmetic of product_cases.gram_lane_group, on a non-empty operand
        assert pc.gram_lane_group(X.nnz, X.nrow, X.ncol, c["sym"], *(c["panel"] or (-1, -1))) in (8, 16, 32)
    elif X.ncol > 0:
        assert one == (c["panel"] is None)
    assert (np.abs(Y.dense()).T @ np.abs(X.dense())).max(initial=0) < LIMIT


def test_gram_panel_cases_cover_the_panel_edges():
    panels = {wc.BY_NAME[n]["panels"] for n in _cases("gram") if wc.BY_NAME[n].get("route") == "gen_pan"}
    assert panels == {(1, 40), (1, 64), (2, 1), (3, 1)}         # a partial panel, exactly one, one + a cell, two + a cell
    assert {wc.BY_NAME[n]["types"] for n in _cases("gram") if wc.BY_NAME[n].get("route") == "gen_one"} == set(pc.TYPE_PAIRS)


@pytest.mark.parametrize("name", _cases("csc_dense", "pbc"))
def test_dense_case(name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    A, Y = o["A"], o["Y"]
    assert Y.shape == (A.nrow, c["K"]) and np.all(Y == np.rint(Y))
    assert (np.abs(Y).astype(np.int64).T @ np.abs(A.dense())).max(initial=0) < LIMIT
    if c["entry"] == "pbc":
        # pbc_kind() of kernels_mult_pbc.hip; the GPU half asserts the same through PbcPlan.plan()
        CBW, WPB, logR = c["layout"]
        kind = ("dma" if 256 <= A.nrow < 1 << 28 else "none") if (WPB, logR) == (16, 7) else "gather"
        assert 1 <= CBW <= 40 and kind == c["kind"]


@pytest.mark.parametrize("form,place,value", wc.FLAG_CASES)
def test_flag_placement(form, place, value):
    clean, dirty, k = wc.flag_operands(form, place, value)
    type, bad = wc.FLAG_VALUES[value]
    key = "Y" if place == "y" else "B" if place == "b" else "X" if form.startswith("gram") else "A"
    d, c = dirty[key], clean[key]
    assert d.type == c.type == type
    differs = np.flatnonzero(d.val.view(np.int64 if type == "double" else np.int32) !=
                             c.val.view(np.int64 if type == "double" else np.int32))
    assert list(differs) == [k]
    assert d.val[k] == NA_integer if type == "integer" else not np.isfinite(d.val[k])
    for other in set(clean) - {key, "B2"}:
        assert dirty[other] is clean[other] or (form == "gram_sym" and dirty["X"] is dirty["Y"])
    if place.endswith("first"):
        assert k == 0
    if place.endswith("last"):
        assert k == d.nnz - 1
    if place in wc.FLAG_LEAF:
        leaf, referenced = wc.FLAG_LEAF[place]
        assert d.col[k] == leaf
        assert (leaf in set(clean["B"].ri)) == referenced, f"leaf {leaf}: some column of B names it: {not referenced}"
    wc.flag_expected(form, clean)                               # (finite, integer-valued: dense() asserts it)


# ---------------------------------------------------------------------------
# every case through the oracle
# ---------------------------------------------------------------------------
def _same(got, want, what):
    got = np.asarray(got, dtype=np.float64).reshape(-1, order="F")
    want = np.asarray(want, dtype=np.float64).reshape(-1, order="F")
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    assert np.array_equal(got.view(np.int64), want.view(np.int64)) or np.array_equal(got, want), what


@pytest.mark.parametrize("name", _cases("gram"))
def test_oracle_gram(oracle, name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    x = o["X"].svt()
    got = oracle.crossprod(x) if c["sym"] else oracle.crossprod(x, o["Y"].svt())
    _same(got, wc.expected(c)[0].T, name)                       # (nx, ny)


@pytest.mark.parametrize("name", _cases("spmm_prepared"))
def test_oracle_matmul(oracle, name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    want = wc.expected(c)
    _same(oracle.matmul(o["A"].svt(), o["B"].svt()), want[0].T, name)
    _same(oracle.matmul(o["A"].svt(), o["B2"].svt()), want[2].T, name + " second B")
    one = wc.BY_NAME[name.replace("spmm_prepared", "spmm")]
    assert np.array_equal(wc.expected(one)[0], want[0])


ROW_METHOD = {"sum": "rowSums", "min": "rowMins", "range": "rowRanges", "mean": "rowMeans", "var1": "rowVars"}


@pytest.mark.parametrize("name", _cases("rowsums", "rowstats"))
def test_oracle_row_statistic(oracle, name):
    c = wc.BY_NAME[name]
    x = wc.operands(c)["A"]
    dim = wc.ROW_OPERANDS[c["row"]]["dim"] if "row" in c else (x.nrow, x.ncol)
    got = getattr(oracle, ROW_METHOD[c["op"]])(x.svt(dim), dims=len(dim) - 1)
    _same(got, wc.expected(c)[0], name)
    if c["entry"] == "rowsums":
        assert np.array_equal(wc.expected(wc.BY_NAME[name.replace("rowsums", "rowsums_prepared")])[0], wc.expected(c)[0])


@pytest.mark.parametrize("name", _cases("colmedians"))
def test_oracle_colmedians(oracle, name):
    c = wc.BY_NAME[name]
    _same(oracle.colMedians(wc.operands(c)["A"].svt()), wc.expected(c)[0], name)


@pytest.mark.parametrize("name", _cases("rowsum_prepared"))
def test_oracle_rowsum(oracle, name):
    c = wc.BY_NAME[name]
    x, want = wc.operands(c)["A"], wc.expected(c)[0]           # (ncol, ngroup)
    g, slot = wc.group_of(x.nrow, c["ngroup"])
    got, ugroup = oracle.rowsum(x.svt(), [None if v == NA_integer else int(s) for v, s in zip(g, slot)])
    present = [c["ngroup"] - 1 if u is None else u for u in ugroup]
    _same(np.asarray(got), want[:, present].T, name)
    absent = [s for s in range(c["ngroup"]) if s not in present]
    assert not want[:, absent].any()


@pytest.mark.parametrize("name", _cases("csc_dense"))
def test_oracle_sparse_dense(oracle, name):
    c, o = wc.BY_NAME[name], wc.operands(wc.BY_NAME[name])
    _same(oracle.crossprod(o["A"].svt(), np.asfortranarray(o["Y"])), wc.expected(c)[0].T, name)
    twin = wc.BY_NAME.get(name.replace("csc_dense", "pbc"))
    if twin is not None:
        assert np.array_equal(wc.expected(twin)[0], wc.expected(c)[0])


def test_oracle_shard_block_clean(oracle):
    A, B = wc.shard_operands("clean", None)
    _same(oracle.crossprod(A.svt(), B.svt()), A.dense().T @ B.dense(), "clean block")
