"""The seeded random cases of tests/random_cases.py on the GPU: subset, Arith / Math, the order statistics and the ranks
at the device level, eight seeds each, one seed one test.  Whatever a seed draws is compared -- nothing is filtered,
skipped or retried -- against the generator's dense expectation: bits for subset, arith_cases.compare for Arith (ulps
for log1p, expm1 and ^ with the measured MAX_ULPS of tests/test_hip_arith.py), tolerance 0 for medians, quantiles, MADs
and ranks.  tests/test_random_cases_cpu.py validates generators and expectations without a GPU.

tests/random_cases.py draws nine families; the five later ones -- Compare / Logic, sweep(), pmin / pmax and is*(),
subassignment by N-index, the L-index and M-index -- run in tests/test_zzzzzzzzzzz_random_cases_hip.py, which stands
last in the suite's order."""
import numpy as np
import pytest

import random_cases as rc
from helpers import assert_equal
from test_hip_arith import MAX_ULPS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiles(hip):
    return rc.tiles()


def _device(nrow, cp, ri, val, logical=False):
    from sparsearray_amd.device import DeviceCSC
    return DeviceCSC(nrow, torch.as_tensor(np.array(cp), device="cuda"), torch.as_tensor(np.array(ri), device="cuda"),
                     torch.as_tensor(np.array(val), device="cuda"), logical=logical)


def _host(R):
    torch.cuda.synchronize()
    return R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy()


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_subset_seed(tiles, seed):
    from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP
    c = rc.SubsetCase(seed, tiles[0])
    A = _device(c.nrow, c.cp, c.ri, c.val, logical=c.type == "logical")
    for rows, cols in c.calls:
        R = A.subset(rows=rows, cols=cols)
        what = (f"seed {seed} ({c.type}, {c.nrow} x {c.lens.size}, {c.total} nonzeros), rows {c.row_kinds} "
                f"{None if rows is None else rows.size}, cols {c.col_kind} {None if cols is None else cols.size}")
        assert R.Rtype == {"double": REALSXP, "integer": INTSXP, "logical": LGLSXP}[c.type], what
        assert R.nrow == (c.nrow if rows is None else rows.size) and R.ncol == (c.lens.size if cols is None else cols.size), what
        rc.same_csc(_host(R), c.expected((rows, cols)), what)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_arith_seed(tiles, seed):
    c = rc.ArithCase(seed, tiles[1])
    x, y = _device(c.nrow, *c.csc("x")), _device(c.nrow, *c.csc("y"))
    for call in c.calls:
        _, kind, arg = call
        if kind == "merge":
            R = x.arith(arg, y)
        elif kind == "neg":
            R = x.neg()
        elif kind == "math":
            R = x.math(arg)
        else:
            op, s, st = arg
            R = x.arith(op, int(s) if st == "integer" else float(s))
        ulps_of = c.expected(call)[2]
        got = _host(R)
        assert R.nrow == c.nrow and R.ncol == c.ncol
        worst = c.compare(call, (got, bool(R.ovflow.item())), max_ulps=MAX_ULPS.get(ulps_of, 0))
        if ulps_of:
            print(f"seed {seed}: {call[0]}: at most {worst} ulps from the correctly rounded value")


@pytest.mark.parametrize("tall", [False, True], ids=["5000_rows", "40000_rows"])
@pytest.mark.parametrize("seed", rc.SEEDS)
def test_order_statistics_seed(hip, seed, tall):
    from sparsearray_amd import device
    c = rc.OrderStatCase(seed, tall)
    A = _device(c.nrow, c.cp, c.ri, c.val)
    center = torch.as_tensor(c.center, device="cuda")
    for call in c.calls:
        _, f, na_rm = call
        if f == "colmedians":
            got = device.colmedians(A, na_rm=na_rm).cpu().numpy()
        elif f == "colquantiles":
            got = device.colquantiles(A, c.probs, na_rm=na_rm).cpu().numpy().T
        else:
            got = device.colmads(A, center=center if f == "colmads_center" else None, na_rm=na_rm).cpu().numpy()
        assert_equal(got, c.expected(call), tol=0, strict_na=True, what=f"seed {seed} ({c.type}) {call[0]} probs {c.probs}")


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_ranks_seed(tiles, seed):
    from sparsearray_amd import device
    c = rc.RanksCase(seed, tiles[2])
    A = _device(c.nrow, c.cp, c.ri, c.val)
    for call in c.calls:
        rank_nz, zero_rank = (t.cpu().numpy() for t in device.colranks(A, ties_method=call[1]))
        dtype = np.float64 if call[1] == "average" else np.int32
        assert rank_nz.dtype == dtype and zero_rank.dtype == dtype
        assert_equal(c.expand(rank_nz, zero_rank), c.expected(call), tol=0, strict_na=True,
                     what=f"seed {seed} ({c.type}, lengths {c.lengths}) {call[0]}")
