"""The branches of the sparse-result product on the GPU that tests/test_zzzzzzzz_spgemm_hip.py leaves unrun: the cases
of tests/spgemm_branch_cases.py (metadata batches of 64 pairs, runs at the lane count, the split forms of the table
pass, the second trip of its value scan, operands too tall for the LDS table, integers near 2^31), each through the
whole route of ``through_the_whole_route``.  The expectation is ``spgemm_branch_cases.expect_csc``, proved equal to
``spgemm_cases.expect`` in tests/test_zzzzzzzzzz_spgemm_branches_cpu.py; which branch a case takes is asserted there
from its shape, not observed here."""
import numpy as np
import pytest

import spgemm_branch_cases as bc
import spgemm_cases as gc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_zzzzzzzz_spgemm_hip import Raw, _device, panel, through_the_whole_route  # noqa: E402,F401  (panel: the fixture)


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_through_the_whole_route(panel, name):
    c = bc.case(panel, name)
    r, got = through_the_whole_route(c.A, c.B, c.want, name)
    assert r.nnz.value == c.want.csc[1].size > 0
    if name in bc.NA_NAMES:
        assert int(r.flag.body()[0]) == 1 and np.isnan(got[2]).any()
    if name in bc.TALL:                         # the workspace of the advertised size holds the layout of the header
        assert r.nb >= bc.ws_least(panel, c.A.shape[0], c.A.shape[1], 3)


def _rewritten(A_dev, at, value, dtype):
    """one value of a resident operand rewritten in place; returns the value that stood there"""
    old = A_dev.val[at:at + 1].clone()
    A_dev.val[at:at + 1].copy_(torch.as_tensor(np.array([value], dtype), device="cuda"))
    return old


def _flag_variants(panel, c, places, what):
    """per type of A: the clean operand (flag 0), then one special value at a time -- the operand is uploaded once and
    only ``val`` is rewritten on the device -- through count and fill: the flag is 1, the arrays by class, the guards
    intact"""
    B = _device(c.B)
    for type in ("double", "integer"):
        A0 = bc.sparse(c.A) if type == "double" else bc.as_integer(c.A, 3900)
        A = _device(A0)
        runs = [("clean", None, None, None)] + [(f"{where}, {tag}", j, pos, v) for where, j, pos in places
                                                for tag, v in bc.SPECIALS[type]]
        for label, j, pos, v in runs:
            label = f"{what}, {type}, {label}"
            host, old, at = A0, None, None
            if j is not None:
                host, at = bc.with_special(A0, j, pos, v)
                old = _rewritten(A, at, v, host.csc[2].dtype)
            want = bc.ExpectedCSC(host, c.B)
            assert want.not_finite == (j is not None)
            r = Raw(A, B)
            assert r.count() == 0
            assert int(r.flag.body()[0]) == int(want.not_finite), f"{label}: not_finite"
            assert r.nnz.value == want.csc[1].size and np.array_equal(r.cp.body(), want.csc[0]), f"{label}: count"
            assert r.fill() == 0
            assert r.cp.intact() and r.flag.intact() and r.ri.intact() and r.vv.intact() and r.ws_guard_intact(), label
            gc.expected_mask_check(r.arrays(), want, label)
            if old is not None:
                A.val[at:at + 1].copy_(old)


@pytest.mark.parametrize("form", bc.FLAG_FORMS)
def test_one_special_value_by_position_in_the_table_forms(panel, form):
    """the value scan inside the table kernel (SCAN 1 and 2) under split 4, split 2 and no split: position 0, 4095,
    4096, the middle and the end of a long leaf, the last leaf, a leaf nobody refers to"""
    c = bc.case(panel, form)
    _flag_variants(panel, c, bc.flag_places(c), form)


@pytest.mark.parametrize("name", bc.TALL)
def test_one_special_value_at_either_end_of_a_tall_operand(panel, name):
    """past 1023 panels spgemm_scan_values() answers for A: a special at its first and at its last value"""
    c = bc.case(panel, name)
    _flag_variants(panel, c, bc.tall_flag_places(c), name)
