"""A failed allocation in the middle of a composition, on the device (tests/alloc_fail_cases.py): the allocator is the
production one, _TorchBlocks, with a countdown -- stream-ordered torch allocations, so a block released while an earlier
kernel of the stream still runs is safe.  Per entry point: one successful call counts the allocations n and keeps the
result; for every k in 3..n a call whose k-th allocation fails returns -1 with the message that names the entry point,
leaves no block live and the outputs untouched; a last successful call gives the first result bit for bit.  (k = 1 and 2,
before anything is launched, are tests/test_zzzzzzzzz_alloc_failure_cpu.py.)  Nothing here faults: every failure is a host function
that returns NULL on a path the library handles.

Operands: 5 x 4 double with 6 entries, column 1 (and 3) empty, column 2 full; the second operand of the merges shares
two positions with the first; the product is 5 x 4 times 4 x 3."""
import numpy as np
import pytest
import torch

from alloc_fail_cases import GPU_ROWS, Operands, Outputs, check_failure
from sparsearray_amd.device import DeviceCSC, _TorchBlocks, _lib, _stream

pytestmark = pytest.mark.gpu


class CountdownBlocks(_TorchBlocks):
    """_TorchBlocks whose ``fail_at``-th request (0: none) is answered with NULL"""

    def __init__(self, device, fail_at=0):
        super().__init__(device)
        self.fail_at, self.asked = fail_at, 0

    def _alloc(self, nbytes, ctx):
        self.asked += 1
        return None if self.asked == self.fail_at else super()._alloc(nbytes, ctx)


def _csc(nrow, ncol, entries, logical=False):
    """DeviceCSC of the (row, col, value) triples, column-major order"""
    entries = sorted(entries, key=lambda e: (e[1], e[0]))
    cp = np.zeros(ncol + 1, np.int64)
    for _, c, _ in entries:
        cp[c + 1:] += 1
    ri = np.array([e[0] for e in entries], np.int32)
    val = np.array([e[2] for e in entries], np.int32 if logical else np.float64)
    return DeviceCSC(nrow, *[torch.as_tensor(a, device="cuda") for a in (cp, ri, val)], logical=logical)


@pytest.fixture(scope="module")
def operands():
    xe = [(1, 0, 1.5)] + [(r, 2, float(r + 2)) for r in range(5)]
    ye = [(1, 0, -1.5), (3, 0, 4.0), (2, 2, 9.0), (0, 3, 0.25)]
    csc = dict(x=_csc(5, 4, xe), y=_csc(5, 4, ye), lx=_csc(5, 4, [(r, c, 1) for r, c, _ in xe], logical=True),
               ly=_csc(5, 4, [(r, c, 1) for r, c, _ in ye], logical=True),
               b=_csc(4, 3, [(0, 0, 2.0), (2, 0, -1.0), (2, 1, 0.5), (3, 2, 3.0)]), v=_csc(2, 2, [(0, 0, 8.0), (1, 1, -8.0)]))
    dense = np.zeros((5, 4))
    for r, c, v in xe:
        dense[r, c] = v
    arrays = dict(dense=dense.reshape(-1, order="F"), stats=np.array([1.0, 2.0, 3.0, 4.0]), vals=np.full(1, 7.0),
                  rows=np.array([1, 3], np.int32), leaves=np.array([0, 2], np.int32), cols=np.array([2, 0], np.int32),
                  rows3=np.array([0, 2, 3], np.int32), rows_general=np.array([3, 1, 1], np.int32),
                  L=np.array([2, 11], np.int64), M=np.array([2, 1, 0, 2], np.int32), word=np.zeros(4, np.int32))
    tensors = {k: torch.as_tensor(a, device="cuda") for k, a in arrays.items()}
    return Operands(**{k: o.handle for k, o in csc.items()}, **{k: t.data_ptr() for k, t in tensors.items()}, stream=_stream(),
                    keep=(csc, tensors))


def _result(mem, outs, ncol, val_bytes):
    """the three result arrays as integers, copied"""
    nnz = outs.nnz.value
    blocks = [mem.live[p.value] for p in outs.ptr]
    return (blocks[0][:(ncol + 1) * 8].view(torch.int64).clone(), blocks[1][:nnz * 4].view(torch.int32).clone(),
            blocks[2][:nnz * val_bytes].view(torch.int64 if val_bytes == 8 else torch.int32).clone())


@pytest.mark.parametrize("name,entry,ncol,val_bytes,call", GPU_ROWS, ids=[r[0] for r in GPU_ROWS])
def test_every_allocation_of_a_composition_may_fail(operands, name, entry, ncol, val_bytes, call):
    lib, dev = _lib(), torch.device("cuda")

    def run(fail_at):
        mem, outs = CountdownBlocks(dev, fail_at), Outputs()
        return call(lib, operands, [mem.alloc_fn, mem.free_fn, None] + outs.byref()), mem, outs

    rc, mem, outs = run(0)
    assert rc == 0, lib.svt_last_error().decode()
    n, first = mem.asked, _result(mem, outs, ncol, val_bytes)
    assert n >= 4 and len(mem.live) == 3                    # col_ptr, a workspace, row_idx, val at the least; the three are kept
    for k in range(3, n + 1):
        rc, mem, outs = run(k)
        check_failure(lib, entry, rc, mem.live, outs)
    rc, mem, outs = run(0)
    assert rc == 0 and mem.asked == n
    for a, b in zip(first, _result(mem, outs, ncol, val_bytes)):
        assert torch.equal(a, b)
