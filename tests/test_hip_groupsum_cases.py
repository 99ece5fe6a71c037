"""rowsum() / colsum() on the device, one asserted case per launch form: the cases of groupsum_cases.py through
svt_dev_rowsum, the prepared ids and sums (svt_dev_rowsum_prepare / _prepared) and the host entry points
(svt_rowsum_SVT, svt_colsum_SVT, the dgCMatrix pair).  Every test asserts through the host queries which kernel it is
about to run, hands over an output filled with a sentinel and holds every cell to an exact expectation (Expect.check).
test_groupsum_cases_cpu.py holds the CPU reference to the same expectations and shows what they reject."""
import numpy as np
import pytest

import groupsum_cases as gc

pytestmark = pytest.mark.gpu

REC = {}            # worst err / bound per (who, entry, form): tools/debug/groupsum_accuracy_record.py prints it


def _operand(c, val):
    from sparsearray_amd.device import DeviceCSC
    return DeviceCSC.from_host(c.nrow, c.col_ptr, c.row_idx, val)


def _sentinel_out(c):
    import torch
    return torch.full((c.ncol, c.ngroup), gc.SENTINEL, dtype=torch.float64, device="cuda")


def _group(c):
    import torch
    return torch.as_tensor(c.group32, device="cuda")


def _flat(out):
    # (ncol, ngroup) C-contiguous = the column-major ngroup x ncol matrix: cell g + ngroup * j
    return out.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("name,palette", gc.ROWSUM_PARAMS)
def test_device_rowsum(hip, name, palette):
    """svt_dev_rowsum on the resident operand: the form and C the case names, then every cell."""
    from sparsearray_amd import device
    c = gc.rowsum_layout(name)
    gc.assert_rowsum_form(c)
    A = _operand(c, gc.case_values(name, c.nnz, palette))
    form, C, _ = device.rowsum_form(A, c.ngroup)
    assert (form, C) == (c.form, c.C)
    g = _group(c)
    for na_rm in gc.na_rms(palette):
        out = _sentinel_out(c)
        assert device.rowsum(A, g, c.ngroup, na_rm=na_rm, out=out) is out
        worst = gc.rowsum_expect(name, palette, na_rm).check(_flat(out), f"{name}/{palette} svt_dev_rowsum na_rm={na_rm}")
        gc._note(REC, ("hip device level", "svt_dev_rowsum", form), worst)


@pytest.mark.parametrize("name,palette", gc.ROWSUM_PARAMS)
def test_host_rowsum(hip, name, palette):
    gc.run_rowsum_case(hip, name, palette, REC, "hip")


def _check_ids(c, A, ids_form, C):
    """RowsumPlan into a poisoned buffer: the ids element for element, the bytes past them untouched."""
    import torch
    from sparsearray_amd import device
    assert device.rowsum_prepare_form(A, c.ngroup) == (ids_form, C)
    nbytes = 2 * A.nnz + 16
    gid = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    plan = device.RowsumPlan(A, _group(c), c.ngroup, gid=gid)
    assert plan.gid is gid
    raw = gid.cpu().numpy()
    want = gc.expected_ids(c)[:A.nnz]
    assert want.max() < 0xFFFF
    assert np.array_equal(raw[:2 * A.nnz].view(np.uint16), want), f"{c.name}: ids differ"
    assert (raw[2 * A.nnz:] == 0xFF).all(), f"{c.name}: bytes past the ids were written"
    return plan


@pytest.mark.parametrize("name", list(gc.ROWSUM_CASES))
def test_prepared_ids(hip, name):
    """svt_dev_rowsum_prepare: the flat kernel below 65536 rows or 64 columns (an even and an odd count of nonzeros: its
    threads store two ids at once), the windowed walk with the queried C elsewhere."""
    from sparsearray_amd.device import DeviceCSC
    c = gc.rowsum_layout(name)
    form, C = gc.assert_prepare_form(c)
    val = gc.case_values(name, c.nnz, "tracer")
    _check_ids(c, _operand(c, val), form, C)
    if form == "flat":                                      # the other parity: the operand without its last nonzero
        assert c.lengths[-1] > 0
        cp = c.col_ptr.copy()
        cp[-1] -= 1
        assert gc.rowsum_prepare_form(c.nrow, c.ncol, c.nnz - 1, c.ngroup)[0] == "flat"
        _check_ids(c, DeviceCSC.from_host(c.nrow, cp, c.row_idx[:-1], val[:-1]), "flat", 0)


@pytest.mark.parametrize("name,palette", gc.ROWSUM_PARAMS)
def test_prepared_sums(hip, name, palette):
    """svt_dev_rowsum_prepared on ids prepared into a poisoned buffer: C as queried (4, 1 and 1 with the full LDS for
    the prepared_* cases), every cell."""
    c = gc.rowsum_layout(name)
    C = gc.assert_prepared_form(c)
    form, idC = gc.assert_prepare_form(c)
    A = _operand(c, gc.case_values(name, c.nnz, palette))
    plan = _check_ids(c, A, form, idC)
    for na_rm in gc.na_rms(palette):
        out = _sentinel_out(c)
        assert plan.run(na_rm=na_rm, out=out) is out
        worst = gc.rowsum_expect(name, palette, na_rm).check(_flat(out), f"{name}/{palette} prepared na_rm={na_rm}")
        gc._note(REC, ("hip device level", "svt_dev_rowsum_prepared", f"C={C}"), worst)


def test_prepared_refuses_more_groups_than_lds_holds(hip):
    import torch
    from sparsearray_amd import device
    from sparsearray_amd.api import SparseArrayError
    c = gc.rowsum_layout("prepared_g20480")
    assert gc.rowsum_prepared_form(c.ncol, 20481) == (False, 0)
    A = _operand(c, gc.case_values(c.name, c.nnz, "tracer"))
    plan = device.RowsumPlan(A, _group(c), 20481)           # (the ids: up to 65535 groups)
    out = torch.full((c.ncol, 20481), gc.SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(SparseArrayError, match="more groups than a workgroup's LDS holds"):
        plan.run(out=out)
    assert bool((out == gc.SENTINEL).all())


@pytest.mark.parametrize("palette", gc.ALL)
@pytest.mark.parametrize("name", ["lds_table_g1000", "windowed_2W1"])
def test_dgcmatrix(hip, name, palette):
    gc.run_dgc_case(hip, name, palette, REC, "hip")


def test_integer_rowsum(hip, oracle):
    gc.run_int_rowsum_case(hip, oracle, "windowed_2W1")


@pytest.mark.parametrize("palette", gc.COLSUM_PALETTES)
@pytest.mark.parametrize("ngroup", gc.COLSUM_NGROUPS)
def test_colsum(hip, oracle, ngroup, palette):
    gc.run_colsum_case(hip, ngroup, palette, REC, "hip", oracle=oracle)
