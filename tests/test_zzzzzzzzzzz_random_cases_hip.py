"""The seeded random cases of tests/random_cases.py for the five families on the merge, map and sweep tile kernels --
Compare / Logic, sweep(), pmin / pmax and is*(), subassignment by N-index, the L-index and M-index -- on the GPU, eight
seeds each, one seed one test (the four earlier families: tests/test_hip_random_cases.py, whose pattern these follow).
Whatever a seed draws is compared -- nothing is filtered, skipped or retried -- against the generator's dense expectation:
arith_cases.compare for the Arith sweep (ulps for ^ with the measured MAX_ULPS of tests/test_hip_arith.py), bits and the
stored entries exactly for Compare, Logic, pmin / pmax, is*() and both subassignments; extents, Rtype, the overflow word
and the route of the cell placement are asserted.  tests/test_zzzzzzzzzzz_random_cases_cpu.py validates generators and
expectations without a GPU.

The module stands last in the suite's order, like every module added since the suite grew long: the tests in front of
it keep their places in a run."""
import numpy as np
import pytest

import lindex_cases as lc
import pminmax_cases as pc
import random_cases as rc
import subset_cases as sc
from test_hip_arith import MAX_ULPS
from test_hip_random_cases import _device, _host

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiles(hip):
    return rc.tiles()


@pytest.fixture(scope="module")
def more_tiles(hip):
    return rc.more_tiles()


def _rtype(name):
    from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP
    return {"double": REALSXP, "integer": INTSXP, "logical": LGLSXP}[name]


def _scalar(s, st):
    """the scalar as the Python value whose class names its R type"""
    return bool(s) if st == "logical" else int(s) if st == "integer" else float(s)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_compare_seed(tiles, seed):
    from sparsearray_amd import SparseArrayError
    c = rc.CompareCase(seed, tiles[1])
    x = _device(c.nrow, *c.csc("x"), logical=c.types[0] == "logical")
    y = _device(c.nrow, *c.csc("y"), logical=c.types[1] == "logical")
    for call in c.calls:
        name, kind, arg = call
        if kind == "merge":
            R = x.compare(arg, y)
        elif kind == "logic":
            R = x.logic(arg, y)
        else:
            R = x.compare(arg[0], _scalar(*arg[1:]))
        what = f"seed {seed} ({c.types}, {c.nrow} x {c.ncol}, merged {c.merged}, share {c.share}, equal {c.equal}): {name}"
        assert R.Rtype == _rtype("logical") and R.nrow == c.nrow and R.ncol == c.ncol, what
        rc.same_csc(_host(R), c.expected(call), what)
    op, s, st = c.refused
    with pytest.raises(SparseArrayError, match="result wouldn't be sparse"):
        x.compare(op, _scalar(s, st))


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_sweep_seed(tiles, seed):
    from sparsearray_amd import SparseArrayError
    c = rc.SweepCase(seed, tiles[1])
    x = _device(c.nrow, *c.csc())

    def run(call):
        _, rule, op, na_rm, st, stats = call
        return x.sweep(op, torch.as_tensor(stats, device="cuda"), c.margin, dim=c.dim, logical=st == "logical", na_rm=na_rm)

    for call in c.calls:
        want, cls, t, over = c.expected(call)
        R = run(call)
        what = f"seed {seed} ({c.type}, dim {c.dim}, {c.total} nonzeros): {call[0]}"
        got = _host(R)
        assert R.Rtype == _rtype(t) and R.nrow == c.nrow and R.ncol == c.ncol, what
        if cls is None:
            pc.same(got, want, what)
        else:
            worst = rc.same_csc_by_class(got, want, cls, what, MAX_ULPS["^"] if call[2] == "^" else 0)
            if call[2] == "^":
                print(f"{what}: at most {worst} ulps from the correctly rounded value")
        if over is not None:
            assert bool(R.ovflow.item()) == over, f"{what}: the overflow word"
    refused, first = c.refused
    with pytest.raises(SparseArrayError, match=rf"stats\[{first}\] = .*does not keep the result sparse"):
        run(refused)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_pminmax_seed(tiles, seed):
    c = rc.PminmaxCase(seed, tiles[1])
    x = _device(c.nrow, *c.csc("x"), logical=c.types[0] == "logical")
    y = _device(c.nrow, *c.csc("y"), logical=c.types[1] == "logical")
    for call in c.calls:
        name, kind, arg = call
        if kind == "merge":
            R = getattr(x, arg[0])(y, na_rm=arg[1])
        elif kind == "scalar":
            R = getattr(x, arg[0])(_scalar(*arg[2:]), na_rm=arg[1])
        else:
            R = {"is.na": x.is_na, "is.nan": x.is_nan, "is.infinite": x.is_infinite}[arg]()
        want, t = c.expected(call)
        what = f"seed {seed} ({c.types}, {c.nrow} x {c.ncol}, merged {c.merged}, share {c.share}): {name}"
        assert R.Rtype == _rtype(t) and R.nrow == c.nrow and R.ncol == c.ncol, what
        pc.same(_host(R), want, what)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_subassign_seed(tiles, more_tiles, seed):
    c = rc.SubassignCase(seed, tiles[1], more_tiles[0])
    tx, tv = c.types
    x = _device(c.nrow, *c.csc(), logical=tx == "logical")
    for call in c.calls:
        name, rows, leaves, value = call
        if isinstance(value, tuple):
            value = _device(*value, logical=tv == "logical")
        R = x.subassign(rows, leaves, value, logical=tv == "logical")
        want, t = c.expected(call)
        what = (f"seed {seed} ({c.types}, {c.nrow} x {c.ncol}, {c.total} nonzeros, cover {c.cover}): {name}, rows {c.row_kind} "
                f"{None if rows is None else rows.size}, leaves {c.leaf_kind} {None if leaves is None else leaves.size}")
        assert R.Rtype == _rtype(t) and R.nrow == c.nrow and R.ncol == c.ncol, what
        rc.same_csc(_host(R), want, what)


def _cells(R, nrow):
    from sparsearray_amd.svt import LGLSXP, REALSXP
    got = _host(R)
    return "double" if R.Rtype == REALSXP else "logical" if R.Rtype == LGLSXP else "integer", rc.keys_of(got, nrow), got[2]


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_cells_seed(tiles, more_tiles, seed):
    from sparsearray_amd.device import lindex_route_counts
    c = rc.CellIndexCase(seed, tiles[1], more_tiles[1])
    op, (tx, tv) = c.op, c.types
    x = _device(op.nrow, *op.csc(), logical=tx == "logical")
    what = f"seed {seed} ({c.types}, dim {op.dim}, {op.cells.size} nonzeros, {c.kind} index of {c.L.size}, {c.value.size} values)"
    got = x.subset_lindex(torch.as_tensor(c.gather, device="cuda")).cpu().numpy()
    want = c.expected_gather()
    assert got.dtype == want.dtype and np.array_equal(sc.bits(got), sc.bits(want)), f"{what}: gather by L-index"
    route = {"sorted": int(c.sorted_route), "unsorted": int(not c.sorted_route)}
    want = c.expected_assign()
    lindex_route_counts(reset=True)
    R = x.subassign_lindex(torch.as_tensor(c.L, device="cuda"), c.value, logical=tv == "logical")
    assert R.nrow == op.nrow and R.ncol == op.ncol
    rc.same_cells(_cells(R, op.nrow), want, f"{what}: subassign by L-index")
    assert lindex_route_counts(reset=True) == route, f"{what}: the route of the L-index"
    if c.with_mindex:
        M = lc.mindex_of(op.dim, c.L)
        got = x.subset_mindex(M, dim=op.dim).cpu().numpy()
        assert np.array_equal(sc.bits(got), sc.bits(c.expected_gather(with_na=False))), f"{what}: gather by M-index"
        R = x.subassign_mindex(torch.as_tensor(M, device="cuda"), c.value, dim=op.dim, logical=tv == "logical")
        rc.same_cells(_cells(R, op.nrow), want, f"{what}: subassign by M-index")
        assert lindex_route_counts(reset=True) == route, f"{what}: the route of the M-index"
