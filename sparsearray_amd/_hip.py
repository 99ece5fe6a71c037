"""ctypes binding of libsvt_hip.so (include/svt_hip.h).

There is deliberately no fallback here: a missing library, a missing symbol or
a box without an MI355X raises ``HipBackendError`` at first use.
"""
from __future__ import annotations

import ctypes
import os

from ._abi import PROTOTYPES

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVT_HIP_TUNING=1: the tuning build (make -C sparsearray_amd/csrc TUNING=1) with the knobs of
# tools/tune_pbc.py compiled in; never what the product, the tests or the bench load.
LIB_PATH = os.path.join(_HERE, "libsvt_hip_tuning.so" if os.environ.get("SVT_HIP_TUNING") == "1"
                        else "libsvt_hip.so")

# Every symbol include/svt_hip.h declares (checked by tests/test_abi.py).
EXPORTS = list(PROTOTYPES)


class HipBackendError(RuntimeError):
    pass


_lib = None
_ready = False


def declare(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Sets the prototype of every function of the C ABI on ``lib`` (sparsearray_amd/_abi.py); a symbol the library
    lacks raises."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            raise HipBackendError(f"{lib._name} does not export {name}") from None
        f.restype, f.argtypes = restype, argtypes
    return lib


def load_library() -> ctypes.CDLL:
    """dlopen only -- no GPU needed (used by the ABI tests on CPU boxes)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipBackendError(
                f"{LIB_PATH} is missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  sparsearray_amd has no CPU path.")
        # torch ships a HIP runtime of its own; when libsvt_hip.so brings in the system one first, torch's
        # later initialisation finds "no HIP GPUs".  Device memory and streams come from torch
        # (sparsearray_amd/device.py), so load it first and let both use one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = declare(ctypes.CDLL(LIB_PATH))
    return _lib


def init(device: int | None = None) -> ctypes.CDLL:
    """Load the library and bind this process to one GPU (LOCAL_RANK by default)."""
    global _ready
    lib = load_library()
    if not _ready:
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        if lib.svt_init(device) != 0:
            raise HipBackendError(lib.svt_last_error().decode())
        _ready = True
    return lib


def set_devices(ordinals) -> None:
    """Device list of the host-level entry points (include/svt_hip.h, svt_set_devices): more than one entry
    shards crossprod(x, y), x %*% y, the col statistics and rowsum() over them; repeated ordinals are separate
    shards on one device; [] restores the device of init()."""
    lib = init()
    ords = [int(d) for d in ordinals]
    arr = (ctypes.c_int * max(1, len(ords)))(*ords)
    if lib.svt_set_devices(arr, len(ords)) != 0:
        raise HipBackendError(lib.svt_last_error().decode())


def get_devices() -> list:
    lib = init()
    arr = (ctypes.c_int * 16)()
    n = lib.svt_get_devices(arr, 16)
    return [arr[i] for i in range(min(n, 16))]


def set_shard_min_nnz(n: int) -> None:
    """Operands with fewer nonzeros stay on the first device of the list (0: always shard)."""
    lib = init()
    lib.svt_set_shard_min_nnz(int(n))


COLSTATS_FORMS = ("thread", "lanes16", "wavefront", "workgroup_cached", "workgroup_streaming", "split")
ROWSTATS_FORMS = ("pipe_units", "pipe", "whole_column", "panel", "memory_atomics")


def colstats_form(nseg: int, nnz: int):
    """(form, nchunk): the launch form of the column statistics for ``nseg`` generalized columns with ``nnz``
    nonzeros in all, one of COLSTATS_FORMS (include/svt_hip.h, svt_dev_colstats_form).  Needs no GPU."""
    lib = load_library()
    nchunk = ctypes.c_int(1)
    form = lib.svt_dev_colstats_form(int(nseg), int(nnz), ctypes.byref(nchunk))
    return COLSTATS_FORMS[form], nchunk.value


def rowstats_form(nrow: int, ncol: int, nnz: int, op: str, inner: int = 1, na_background: bool = False):
    """(form, panel_shift, nsplit): the form one pass of the row statistics takes, one of ROWSTATS_FORMS
    (include/svt_hip.h, svt_dev_rowstats_form).  ``ncol`` counts leaves.  Needs no GPU."""
    from .api import OPCODES
    lib = load_library()
    ps, nsplit = ctypes.c_int(0), ctypes.c_int64(1)
    form = lib.svt_dev_rowstats_form(int(nrow), int(ncol), int(nnz), int(bool(na_background)), OPCODES[op], int(inner),
                                     ctypes.byref(ps), ctypes.byref(nsplit))
    return ROWSTATS_FORMS[form], ps.value, nsplit.value


ROWSUM_FORMS = ("atomic", "lds_table", "lds_g16", "windowed")
ROWSUM_ID_FORMS = ("flat", "windowed")


def rowsum_form(nrow: int, ncol: int, nnz: int, ngroup: int, type: str = "double", col_ptr32: bool = False):
    """(form, cols_per_wg, window_rows): the launch form of rowsum() for an ``nrow`` x ``ncol`` operand of ``nnz``
    nonzeros, one of ROWSUM_FORMS (include/svt_hip.h, svt_dev_rowsum_form); ``col_ptr32``: the dgCMatrix entry point.
    Needs no GPU."""
    from .svt import INTSXP, REALSXP
    lib = load_library()
    C, win = ctypes.c_int(0), ctypes.c_int64(0)
    form = lib.svt_dev_rowsum_form(int(nrow), int(ncol), int(nnz), int(ngroup), REALSXP if type == "double" else INTSXP,
                                   int(bool(col_ptr32)), ctypes.byref(C), ctypes.byref(win))
    return ROWSUM_FORMS[form], C.value, win.value


def rowsum_prepare_form(nrow: int, ncol: int, nnz: int, ngroup: int):
    """(form, cols_per_wg) of svt_dev_rowsum_prepare(), one of ROWSUM_ID_FORMS.  Needs no GPU."""
    lib = load_library()
    C = ctypes.c_int(0)
    form = lib.svt_dev_rowsum_prepare_form(int(nrow), int(ncol), int(nnz), int(ngroup), ctypes.byref(C))
    return ROWSUM_ID_FORMS[form], C.value


def rowsum_prepared_form(ncol: int, ngroup: int):
    """(supported, cols_per_wg) of svt_dev_rowsum_prepared() (svt_dev_rowsum_prepared_form).  Needs no GPU."""
    lib = load_library()
    C = ctypes.c_int(0)
    rc = lib.svt_dev_rowsum_prepared_form(int(ncol), int(ngroup), ctypes.byref(C))
    return rc == 0, C.value


PBC_KINDS = ("none", "dma", "gather")
PBC_KERNELS = ("general", "dma", "gather", "gather2", "gatherx")


class _PbcPlanStruct(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("kernel", ctypes.c_int), ("NV", ctypes.c_int), ("nsplit", ctypes.c_int),
                ("panels_per_split", ctypes.c_int64), ("direct", ctypes.c_int), ("launches", ctypes.c_int),
                ("tail_splits", ctypes.c_int), ("tail_blocks", ctypes.c_int)]


def pbc_plan(handle, K: int, tr_y: bool, stride_c: int, stride_k: int, first_col: int = 0) -> dict:
    """What svt_dev_crossprod_pbc_from() with these arguments launches on the layout ``handle`` (include/svt_hip.h,
    svt_dev_crossprod_pbc_plan): kind one of PBC_KINDS, kernel one of PBC_KERNELS, NV, nsplit, panels_per_split,
    direct, launches, tail_splits, tail_blocks.  Launches nothing."""
    lib = init()
    st = _PbcPlanStruct()
    if lib.svt_dev_crossprod_pbc_plan(handle, int(K), int(bool(tr_y)), int(stride_c), int(stride_k), int(first_col),
                                      ctypes.byref(st)) != 0:
        raise HipBackendError(lib.svt_last_error().decode())
    d = {f: int(getattr(st, f)) for f, _ in _PbcPlanStruct._fields_}
    d["kind"], d["kernel"], d["direct"] = PBC_KINDS[st.kind], PBC_KERNELS[st.kernel], bool(st.direct)
    return d


TRANSPOSE_PLAN_FIELDS = ("bucketed", "fbits", "cbits", "nfb", "ncoarse", "ngroups", "key_sort_passes", "why_not")
TRANSPOSE_PLAN_WHY = ("taken", "shape", "reserve")


def transpose_plan(nrow: int, ncol: int, nnz: int, nslab: int = 1) -> dict:
    """The form t() takes for an ``nrow`` x ``ncol`` operand of ``nnz`` nonzeros, or (``nslab`` > 1) the step "first
    two axes change places" of aperm() for ``nslab`` such matrices holding ``nnz`` nonzeros in all (include/svt_hip.h,
    svt_dev_transpose_plan): bucketed, fbits, cbits, nfb, ncoarse, ngroups, key_sort_passes, why_not (one of
    TRANSPOSE_PLAN_WHY).  Needs no GPU."""
    lib = load_library()
    out = (ctypes.c_int64 * 8)()
    if lib.svt_dev_transpose_plan(int(nrow), int(ncol), int(nnz), int(nslab), out) != 0:
        raise HipBackendError(lib.svt_last_error().decode())
    d = dict(zip(TRANSPOSE_PLAN_FIELDS, (int(x) for x in out)))
    d["bucketed"], d["why_not"] = bool(d["bucketed"]), TRANSPOSE_PLAN_WHY[d["why_not"]]
    return d


def hip_dispatcher():
    from ._dispatch import CAbiDispatcher
    return CAbiDispatcher(init(), "svt_")
