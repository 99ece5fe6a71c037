"""Every case of tests/transpose_cases.py on the GPU: t() and aperm() of hand-built operands, for double, integer and
logical values in the tracer and the specials palette, against the plain 64-bit reference at tolerance 0 (values as
bits), with the route-count delta of the one call equal to the dict the table states and no boxed call.  Then t(t(A)),
and one case of each route inside a 0xA5 arena with guards around the workspace and the three outputs.
tests/test_transpose_cases_cpu.py has asserted, without a GPU, that every case sits on the branch it names."""
import numpy as np
import pytest

import transpose_cases as tc
from helpers import Arena

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in tc.CASES]
TORCH_DTYPE = {"double": torch.float64, "integer": torch.int32, "logical": torch.int32}


def _operand(name, dtype, val):
    from sparsearray_amd.device import DeviceCSC
    c = tc.BY_NAME[name]
    cp, ri = tc.csc_of(c["dim"], tc.pattern(name))
    return DeviceCSC(c["dim"][0], torch.as_tensor(cp, device="cuda"), torch.as_tensor(ri, device="cuda"),
                     torch.as_tensor(val, device="cuda"), logical=dtype == "logical")


def _call(A, c, **kw):
    if c["perm"] is None:
        return A.t(**kw), (c["dim"][1], c["dim"][0])
    return A.aperm(c["dim"], c["perm"], **kw)


def _host(T):
    from sparsearray_amd.svt import LGLSXP
    return T.col_ptr.cpu().numpy(), T.row_idx.cpu().numpy(), T.val.cpu().numpy(), T.Rtype == LGLSXP


def _routed(c, A, **kw):
    """the call, with its route-count delta and the boxed-call count checked against the table"""
    from sparsearray_amd.device import aperm_route_counts, boxed_calls
    aperm_route_counts(reset=True)
    b0 = boxed_calls()
    T, new_dim = _call(A, c, **kw)
    torch.cuda.synchronize()
    delta = {k: v for k, v in aperm_route_counts().items() if v}
    assert delta == c["route"], f"{c['name']} ({c['branch']}): took {delta}, the table says {c['route']}"
    assert boxed_calls() == b0
    assert tuple(new_dim) == tuple(c["dim"][p - 1] for p in (c["perm"] or (2, 1))) and T.nrow == new_dim[0]
    return T


@pytest.mark.parametrize("palette", tc.PALETTES)
@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_case(hip, name, dtype, palette):
    c = tc.BY_NAME[name]
    want, val = tc.expected(name, dtype, palette)
    T = _routed(c, _operand(name, dtype, val))
    assert T.val.dtype == TORCH_DTYPE[dtype]
    tc.compare(_host(T), want, what=f"{name} {dtype} {palette}")


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("name", ["t_pass2_rounds_group", "t_pass2_rounds_two_columns", "t_pass3_rounds",
                                  "t_pass3_rounds_last_row"])
def test_t_of_t_is_the_operand(hip, name, dtype):
    c, lin = tc.BY_NAME[name], tc.pattern(name)
    val = tc.values("tracer", dtype, lin)
    A = _operand(name, dtype, val)
    back = A.t().t()
    torch.cuda.synchronize()
    cp, ri = tc.csc_of(c["dim"], lin)
    tc.compare(_host(back), (cp, ri, val, dtype == "logical"), what=f"t(t({name}))")


# ---------------------------------------------------------------------------
# the arena
# ---------------------------------------------------------------------------
def _ws_bytes(c, nnz):
    from sparsearray_amd.device import _lib
    if c["perm"] is None:
        return _lib().svt_dev_transpose_ws_bytes(c["dim"][0], nnz)
    dim, perm = np.asarray(c["dim"], dtype=np.int64), np.asarray(c["perm"], dtype=np.int32)
    return _lib().svt_dev_aperm_perm_ws_bytes(nnz, len(dim), dim.ctypes.data, perm.ctypes.data)


def _arena_case(name, dtype, boxed=False):
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd.device import boxed_calls
    c, lin = tc.BY_NAME[name], tc.pattern(name)
    want, val = tc.expected(name, dtype, "tracer")
    A = _operand(name, dtype, val)
    nbytes, esz = _ws_bytes(c, lin.size), 8 if dtype == "double" else 4
    assert nbytes > 1
    ar = Arena([nbytes, want[0].size * 8, lin.size * 4, lin.size * esz])
    out = (ar.part(1, torch.int64), ar.part(2, torch.int32), ar.part(3, TORCH_DTYPE[dtype]))
    if boxed:
        b0 = boxed_calls()
        T, _ = _call(A, c, ws=ar.part(0), out=out)
        torch.cuda.synchronize()
        assert boxed_calls() == b0 + 1
    else:
        T = _routed(c, A, ws=ar.part(0), out=out)
    assert T.col_ptr.data_ptr() == out[0].data_ptr() and T.val.data_ptr() == out[2].data_ptr()
    tc.compare(_host(T), want, what=f"{name} in the arena")
    assert ar.guards_intact(), f"{name}: a byte outside the workspace and the outputs was written"
    # one byte short: the entry point's own error, before anything is written
    ar.mem.fill_(0xA5)
    with pytest.raises(SparseArrayError, match="workspace too small"):
        _call(A, c, ws=ar.part(0)[:nbytes - 1], out=out)
    torch.cuda.synchronize()
    assert ar.untouched()


ARENA = sorted((c["arena"], c["name"]) for c in tc.CASES if c["arena"])


@pytest.mark.parametrize("route,name", ARENA, ids=[n for _, n in ARENA])
def test_stays_inside_its_workspace_and_outputs(hip, route, name):
    _arena_case(name, "double")
    _arena_case(name, "integer")


@pytest.mark.parametrize("name", ["t_plain_staged", "a_swap01_refused_to_slab"])
def test_boxed_driver_stays_inside_its_workspace_and_outputs(hip, name):
    """t() and a row-moving aperm() through the boxed driver (boxes of 4096 nonzeros): the workspace is sized and
    checked under the same box limit"""
    from sparsearray_amd.device import set_box_nnz
    assert tc.pattern(name).size > 4 * 4096
    try:
        set_box_nnz(4096)
        _arena_case(name, "double", boxed=True)
    finally:
        set_box_nnz(0)
