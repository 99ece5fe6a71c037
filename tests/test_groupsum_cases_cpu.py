"""The rowsum / colsum cases of groupsum_cases.py without a GPU: the CPU reference runs every case and is held to the
same expectations as the kernels; every case's launch form and columns per workgroup are asserted through the host
queries; operands one step apart land on different forms; and the checker rejects six wrong results that a relative
1e-9 on random data lets through."""
import numpy as np
import pytest

import groupsum_cases as gc
from sparsearray_amd._hip import rowsum_form, rowsum_prepare_form, rowsum_prepared_form


@pytest.mark.parametrize("name", list(gc.ROWSUM_CASES))
def test_case_takes_its_form(name):
    """Form and C of the unprepared call, of the ids and of the prepared call, and what the case must hold."""
    c = gc.rowsum_layout(name)
    assert gc.assert_rowsum_form(c) == c.form
    assert gc.assert_rowsum_form(c, type="integer") == "atomic"
    assert gc.assert_rowsum_form(c, col_ptr32=True) == "atomic"
    gc.assert_prepare_form(c)
    gc.assert_prepared_form(c)
    want = {"lds_table": gc.LDS_LENGTHS, "lds_g16": gc.LDS_LENGTHS, "windowed": gc.WAVE_LENGTHS,
            "atomic": gc.WAVE_LENGTHS}[c.form]
    if name.startswith("prepared"):
        want = gc.PREPARED_LENGTHS
    if name != "lds_table_g8192":
        assert set(want) <= set(c.lengths.tolist())
    else:
        assert c.ncol == 4 and c.lengths.min() >= 2048 and c.ngroup * 8 == 64 * 1024


def test_every_form_is_reached():
    forms = {gc.rowsum_layout(n).form for n in gc.ROWSUM_CASES}
    assert forms == {"atomic", "lds_table", "lds_g16", "windowed"}
    assert {gc.rowsum_layout(n).C for n in gc.ROWSUM_CASES if gc.rowsum_layout(n).form == "windowed"} == {4, 5, 16}
    assert {gc.rowsum_layout(n).nrow for n in gc.ROWSUM_CASES if gc.rowsum_layout(n).form == "windowed"} == \
        {65536, 2 * gc.W, 2 * gc.W + 1}
    assert {gc.assert_prepare_form(gc.rowsum_layout(n))[0] for n in gc.ROWSUM_CASES} == {"flat", "windowed"}
    assert {1, 4} <= {gc.assert_prepared_form(gc.rowsum_layout(n)) for n in gc.ROWSUM_CASES}
    # the three requests of the full 160 KiB
    assert rowsum_form(2 * gc.W + 1, 66, 66 * 1300, 5120)[:2] == ("windowed", 4)
    assert rowsum_form(65536, 4000, 4000 * 330, 1280)[:2] == ("windowed", 16)
    assert rowsum_prepared_form(19, 20480) == (True, 1) and rowsum_prepared_form(19, 20481) == (False, 0)


@pytest.mark.parametrize("name,param,other,form_there", gc.BOUNDARY_PAIRS)
def test_boundary_pairs(name, param, other, form_there):
    gc.assert_boundary_pair(name, param, other, form_there)


def test_boundary_pairs_cover_every_threshold():
    assert {(p, min(o, getattr(gc.rowsum_layout(n), p))) for n, p, o, _ in gc.BOUNDARY_PAIRS} == \
        {("nrow", 65535), ("ncol", 63), ("ngroup", 5120), ("ngroup", 8192), ("nnz", 15999)}
    # the ids: 65536 rows and 64 columns; the prepared sums: 5120 / 5121 groups (C = 4 / at most 3), 20480 / 20481
    assert rowsum_prepare_form(65535, 66, 6000, 7)[0] == "flat" and rowsum_prepare_form(65536, 66, 6000, 7)[0] == "windowed"
    assert rowsum_prepare_form(65536, 63, 6000, 7)[0] == "flat" and rowsum_prepare_form(65536, 64, 6000, 7)[0] == "windowed"
    assert rowsum_prepared_form(19, 5120) == (True, 4) and rowsum_prepared_form(19, 5121) == (True, 1)


@pytest.mark.parametrize("name,palette", gc.ROWSUM_PARAMS)
def test_oracle_rowsum_cases(oracle, name, palette):
    gc.run_rowsum_case(oracle, name, palette)


@pytest.mark.parametrize("palette", gc.ALL)
@pytest.mark.parametrize("name", ["lds_table_g1000", "windowed_2W1"])
def test_oracle_dgcmatrix(oracle, name, palette):
    gc.run_dgc_case(oracle, name, palette)


def test_oracle_integer_rowsum(oracle):
    gc.run_int_rowsum_case(oracle, None, "windowed_2W1")


@pytest.mark.parametrize("palette", gc.COLSUM_PALETTES)
@pytest.mark.parametrize("ngroup", gc.COLSUM_NGROUPS)
def test_oracle_colsum(oracle, ngroup, palette):
    gc.run_colsum_case(oracle, ngroup, palette)


# ---------------------------------------------------------------------------
# the checker has teeth
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("palette", ["tracer", "a"])
def test_mutants_fail(oracle, palette):
    """Six mutations of a correct result of the windowed case with a row past the second window edge; each changes
    one or two cells of 462 and none may pass.  ("a" with na_rm: the planted values are out of the way.  On "d" a
    doubled value of 2**-60 beside one of 2**60 is within the rounding bound of any sum: that is what the tracer
    palette is for.)"""
    name = "windowed_2W1"
    c = gc.rowsum_layout(name)
    na_rm = palette == "a"
    e = gc.rowsum_expect(name, palette, na_rm)
    val = np.nan_to_num(gc.case_values(name, c.nnz, palette), nan=0.0)
    right = gc.call_xsum(oracle, "rowsum_SVT", gc.case_svt(name, palette), c.group32, c.ngroup, na_rm, e.ncell)
    e.check(right, "the reference")

    def rejected(wrong, why):
        with pytest.raises(AssertionError):
            e.check(wrong, why)

    def moved(k, to_cell):
        assert val[k] != 0
        m = right.copy()
        m[c.cell[k]] -= val[k]
        m[to_cell] += val[k]
        return m

    # 1. the nonzero at row W of window column 4 dropped
    k = int(np.flatnonzero((c.col == 3) & (c.row_idx == gc.W))[0])
    m = right.copy()
    m[c.cell[k]] -= val[k]
    rejected(m, "the nonzero at row W dropped")
    # 2. one nonzero (the last of a full chunk of 64) added twice
    k = int(c.col_ptr[4] + 63)
    m = right.copy()
    m[c.cell[k]] += val[k]
    rejected(m, "a nonzero added twice")
    # 3. one nonzero added to the next group
    k = int(c.col_ptr[20] + 7)
    g, j = c.cell[k] % c.ngroup, c.cell[k] // c.ngroup
    rejected(moved(k, (g + 1) % c.ngroup + c.ngroup * j), "a nonzero in group g + 1")
    # 4. a row of the NA group added to group 1 instead of the last group
    k = int(np.flatnonzero(c.na[c.row_idx])[0])
    assert c.cell[k] % c.ngroup == c.ngroup - 1
    rejected(moved(k, c.ngroup * (c.cell[k] // c.ngroup)), "an NA-group row in group 1")
    # 5. a cell nobody wrote
    m = right.copy()
    m[int(np.flatnonzero(e.stored >= 2)[3])] = gc.SENTINEL
    rejected(m, "an unwritten cell")
    # 6. -0.0 in a cell without a nonzero
    empty = np.flatnonzero(e.stored == 0)
    assert len(empty)
    m = right.copy()
    m[empty[0]] = -0.0
    rejected(m, "-0.0 in an empty cell")
    # (and a cell of one value that is off by one unit in the last place)
    one = int(e.one_cell[0])
    m = right.copy()
    m[one] = np.nextafter(m[one], np.inf)
    rejected(m, "a single value, one ulp off")


def test_left_out_cells_are_counted():
    """At most four cells per case are compared by class; more is an error of the case, not of the result."""
    e = gc.rowsum_expect("windowed_2W1", "a", False)
    assert 1 <= e.poisoned.sum() <= 4
    assert gc.rowsum_expect("windowed_2W1", "a", True).poisoned.sum() == 0
    got = np.where(e.poisoned, np.nan, 0.0)
    with pytest.raises(AssertionError, match="compared by class"):
        e.check(got, "x", max_poisoned=0)


@pytest.mark.parametrize("palette", ["a", "d"])
def test_expectations_agree_with_the_whole_cell_table(oracle, palette):
    """Expect bounds only the cells of two or more values and compares the others bit for bit; exact_stats.rowsum_cells
    and colsum_cells bound every cell.  Both must accept the reference, and both must see a wrong cell."""
    import exact_stats as ex
    c = gc.colsum_layout(40)
    val = gc.case_values(c.name, c.nnz, palette)
    x = gc.SVT_SparseArray.from_csc((c.nrow, c.ncol), "double", c.col_ptr, c.row_idx, val)
    got = gc.call_xsum(oracle, "colsum_SVT", x, c.cgroup32, 40, True, c.nrow * 40)
    cells = ex.colsum_cells(c.col_ptr, c.row_idx, val, c.cslot, 40, c.nrow, na_rm=True)
    v = ex.check_sum(got, cells, "colsum").require()
    assert v.ncompared == c.nrow * 40
    r = gc.rowsum_layout("lds_table_g3")
    val = gc.case_values(r.name, r.nnz, palette)
    got = gc.call_xsum(oracle, "rowsum_SVT", gc.case_svt(r.name, palette), r.group32, 3, True, 3 * r.ncol)
    cells = ex.rowsum_cells(r.col_ptr, r.row_idx, val, r.slot, 3, na_rm=True)
    ex.check_sum(got, cells, "rowsum").require()
    k = int(r.col_ptr[20] + np.nanargmax(np.abs(val[r.col_ptr[20]:r.col_ptr[21]])))       # (the largest of its cell)
    got[r.cell[k]] += val[k]
    assert not ex.check_sum(got, cells, "rowsum").ok
    with pytest.raises(AssertionError):
        gc.rowsum_expect(r.name, palette, True).check(got, "rowsum")
