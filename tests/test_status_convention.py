"""Status convention of the C ABI (include/svt_hip.h): 0 done, < 0 error, > 0 "not supported here" -- the R glue
answers the latter with the reference's CPU body (tests/test_glue_executes.py runs that half on the CPU).  Here: the
library really returns 1, with a message, for operations its device kernels do not implement, and -1 for errors."""
import ctypes

import numpy as np
import pytest

from helpers import random_csc
from sparsearray_amd.svt import make_view_from_csc

pytestmark = pytest.mark.gpu


def test_unsupported_is_status_one_and_errors_are_minus_one(hip):
    from sparsearray_amd import SparseArrayError, SparseArrayUnsupported, _hip
    lib = _hip.init()
    cp, ri, v = random_csc(500, 40, 0.1, seed=3)
    view = make_view_from_csc((500, 40), "double", cp, ri, v)
    out = np.zeros(80)
    warn = ctypes.c_int(0)
    f = lib.svt_colStats_SVT
    # SVT_OP_RANGE = 7: never sent by the R API for col stats (copy_result_to_out() keeps the first scalar only,
    # src/SparseArray_matrixStats.c:179-197); not implemented on the device -> "not supported here"
    rc = f(ctypes.addressof(view), 7, 0, float("nan"), 1, out.ctypes.data, ctypes.byref(warn))
    assert rc == 1 and b"not implemented on the device" in lib.svt_last_error()
    # an error stays an error: dims out of range
    rc = f(ctypes.addressof(view), 8, 0, float("nan"), 5, out.ctypes.data, ctypes.byref(warn))
    assert rc == -1 and b"'dims'" in lib.svt_last_error()
    # and a supported call after both is clean
    rc = f(ctypes.addressof(view), 8, 0, float("nan"), 1, out.ctypes.data, ctypes.byref(warn))
    assert rc == 0
    # device level: the Python wrappers raise the matching exception classes
    from sparsearray_amd.device import DeviceCSC, _check, _lib, _stream
    A = DeviceCSC.from_host(500, cp, ri, v)
    import torch
    o = torch.zeros(80, dtype=torch.float64, device="cuda")
    w = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(SparseArrayUnsupported):
        _check(_lib().svt_dev_colstats(A.handle, 7, 0, float("nan"), 1, o.data_ptr(), w.data_ptr(), _stream()))
    assert issubclass(SparseArrayUnsupported, SparseArrayError)
