"""A failed allocation in a composition, without a GPU (tests/alloc_fail_cases.py): for every entry point that leaves a
new sparse operand in the caller's allocator, a host allocator that returns NULL on its first call, then one that
returns NULL on its second.  Both failures come before anything is launched (col_ptr, then the workspace), so the
operands -- 5 x 4 handles without entries whose arrays are never read -- need no device.  The status is -1, the message
names the entry point that was called, every block handed out was released again and the outputs keep their sentinels."""
import ctypes

import numpy as np
import pytest

from alloc_fail_cases import ROWS, Operands, Outputs, check_failure
from sparsearray_amd._abi import ALLOC_FN, FREE_FN
from sparsearray_amd.svt import LGLSXP, REALSXP


@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


@pytest.fixture(scope="module")
def operands(lib):
    shapes = dict(x=(REALSXP, 5, 4), y=(REALSXP, 5, 4), lx=(LGLSXP, 5, 4), ly=(LGLSXP, 5, 4), b=(REALSXP, 4, 3),
                  v=(REALSXP, 2, 2))
    handles = {k: lib.svt_wrap_device_csc(rt, nr, nc, 0, None, None, None) for k, (rt, nr, nc) in shapes.items()}
    arrays = dict(dense=np.zeros(20), stats=np.ones(4), vals=np.full(1, 7.0), rows=np.array([1, 3], np.int32),
                  leaves=np.array([0, 2], np.int32), cols=np.array([2, 0], np.int32), rows3=np.array([0, 2, 3], np.int32),
                  L=np.array([2, 11], np.int64), M=np.array([2, 1, 0, 2], np.int32))
    yield Operands(**handles, **{k: a.ctypes.data for k, a in arrays.items()}, word=None, stream=None, keep=arrays)
    for h in handles.values():
        lib.svt_release(h)


class HostBlocks:
    """svt_dev_alloc_fn / svt_dev_free_fn over host buffers; the ``fail_at``-th request is answered with NULL"""

    def __init__(self, fail_at):
        self.fail_at, self.asked, self.live, self.keep = fail_at, 0, {}, []
        self.alloc_fn, self.free_fn = ALLOC_FN(self._alloc), FREE_FN(self._release)

    def _alloc(self, nbytes, _ctx):
        self.asked += 1
        if self.asked == self.fail_at:
            return None
        buf = ctypes.create_string_buffer(max(int(nbytes), 16))
        self.keep.append(buf)
        self.live[ctypes.addressof(buf)] = buf
        return ctypes.addressof(buf)

    def _release(self, p, _ctx):
        del self.live[p]                                    # (a block released twice, or one never handed out, raises)


@pytest.mark.parametrize("fail_at", [1, 2])
@pytest.mark.parametrize("name,entry,ncol,val_bytes,call", ROWS, ids=[r[0] for r in ROWS])
def test_a_failed_allocation_releases_everything_and_names_the_entry_point(lib, operands, name, entry, ncol, val_bytes, call,
                                                                          fail_at):
    mem, outs = HostBlocks(fail_at), Outputs()
    rc = call(lib, operands, [mem.alloc_fn, mem.free_fn, None] + outs.byref())
    assert mem.asked == fail_at                             # the composition stopped at the allocation that failed
    check_failure(lib, entry, rc, mem.live, outs)
