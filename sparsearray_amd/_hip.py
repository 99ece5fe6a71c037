"""ctypes binding of libsvt_hip.so (include/svt_hip.h).

There is deliberately no fallback here: a missing library, a missing symbol or
a box without an MI355X raises ``HipBackendError`` at first use.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVT_HIP_TUNING=1: the tuning build (make -C sparsearray_amd/csrc TUNING=1) with the knobs of
# tools/tune_pbc.py compiled in; never what the product, the tests or the bench load.
LIB_PATH = os.path.join(_HERE, "libsvt_hip_tuning.so" if os.environ.get("SVT_HIP_TUNING") == "1"
                        else "libsvt_hip.so")

# Every symbol include/svt_hip.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "svt_init", "svt_last_error", "svt_device_arch", "svt_set_devices", "svt_get_devices", "svt_set_shard_min_nnz",
    "svt_crossprod2_SVT_mat", "svt_crossprod2_mat_SVT",
    "svt_crossprod2_SVT_SVT", "svt_crossprod1_SVT",
    "svt_matmul_SVT_mat", "svt_matmul_SVT_SVT", "svt_tcrossprod1_SVT", "svt_tcrossprod2_SVT_SVT",
    "svt_colMedians_SVT", "svt_rowMedians_SVT", "svt_dev_colmedians_ws_bytes", "svt_dev_colmedians",
    "svt_colQuantiles_SVT", "svt_rowQuantiles_SVT", "svt_dev_colquantiles_ws_bytes", "svt_dev_colquantiles",
    "svt_colMads_SVT", "svt_rowMads_SVT", "svt_dev_colmads_ws_bytes", "svt_dev_colmads",
    "svt_colRanks_SVT", "svt_rowRanks_SVT", "svt_dev_colranks_form", "svt_dev_colranks_ws_bytes", "svt_dev_colranks",
    "svt_resident_set_limit", "svt_resident_clear", "svt_resident_stats", "svt_dev_pbc_bytes", "svt_dev_pbc_set_spare_cus", "svt_dev_pbc_spare_cus", "svt_dev_pbc_set_gather_pacing", "svt_dev_pbc_set_round_launches", "svt_dev_matmul_csc_csc_ws_bytes", "svt_dev_matmul_csc_csc", "svt_dev_rowsums_prepare", "svt_dev_rowsums_prepared", "svt_dev_rowsum_gid_bytes", "svt_dev_rowsum_prepare", "svt_dev_rowsum_prepared", "svt_dev_matmul_csc_csc_prepare", "svt_dev_matmul_csc_csc_prepared",
    "svt_dev_crossprod_csc_csc_ws_bytes", "svt_dev_crossprod_csc_csc", "svt_dev_crossprod_csc_csc_set_panel", "svt_sparse_crossprod_set_cost", "svt_dev_crossprod_csc_csc_dense_buffer",
    "svt_summarize_SVT", "svt_colStats_out_Rtype", "svt_colStats_SVT",
    "svt_rowStats_SVT", "svt_rowsum_SVT", "svt_colsum_SVT",
    "svt_rowsum_dgCMatrix", "svt_colsum_dgCMatrix",
    "svt_colMins_dgCMatrix", "svt_colMaxs_dgCMatrix", "svt_colRanges_dgCMatrix", "svt_colVars_dgCMatrix",
    "svt_upload", "svt_wrap_device_csc", "svt_release",
    "svt_dev_crossprod_ws_bytes", "svt_dev_crossprod_csc_dense",
    "svt_dev_dense_prepare", "svt_dev_crossprod_prepared",
    "svt_dev_pbc_build", "svt_dev_pbc_release", "svt_dev_pbc_trim",
    "svt_dev_crossprod_pbc_ws_bytes", "svt_dev_crossprod_pbc", "svt_dev_crossprod_pbc_phase", "svt_dev_crossprod_pbc_from",
    "svt_dev_crossprod_pbc_plan",
    "svt_get_num_procs", "svt_get_max_threads", "svt_set_max_threads", "svt_dev_aperm_ws_bytes", "svt_dev_aperm_perm_ws_bytes", "svt_dev_aperm", "svt_dev_aperm_route_counts", "svt_aperm_SVT", "svt_transpose_2D_SVT", "svt_dev_transpose_ws_bytes", "svt_dev_transpose", "svt_dev_transpose_plan", "svt_dev_set_box_nnz", "svt_dev_boxed_calls", "svt_dev_colstats", "svt_dev_rowstats_ws_bytes", "svt_dev_rowsums", "svt_dev_rowsum",
    "svt_rowStatsFull_SVT", "svt_dev_rowstats_ws_bytes_op", "svt_dev_rowstats",
    "svt_dev_colstats_form", "svt_dev_rowstats_form",
    "svt_dev_subset_tile", "svt_dev_subset_cols_ws_bytes", "svt_dev_subset_cols_count", "svt_dev_subset_cols_fill",
    "svt_dev_subset_rows_ws_bytes", "svt_dev_subset_rows_count", "svt_dev_subset_rows_fill", "svt_dev_subset",
    "svt_dev_subset_route_counts", "svt_subset_SVT_begin", "svt_subset_SVT_end",
]


class HipBackendError(RuntimeError):
    pass


_lib = None
_ready = False


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
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.svt_last_error.restype = ctypes.c_char_p
        _lib.svt_device_arch.restype = ctypes.c_char_p
        _lib.svt_init.argtypes = [ctypes.c_int]
        _lib.svt_init.restype = ctypes.c_int
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
    lib.svt_set_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    if lib.svt_set_devices(arr, len(ords)) != 0:
        raise HipBackendError(lib.svt_last_error().decode())


def get_devices() -> list:
    lib = init()
    lib.svt_get_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    arr = (ctypes.c_int * 16)()
    n = lib.svt_get_devices(arr, 16)
    return [arr[i] for i in range(min(n, 16))]


def set_shard_min_nnz(n: int) -> None:
    """Operands with fewer nonzeros stay on the first device of the list (0: always shard)."""
    lib = init()
    lib.svt_set_shard_min_nnz.argtypes = [ctypes.c_int64]
    lib.svt_set_shard_min_nnz.restype = None
    lib.svt_set_shard_min_nnz(int(n))


COLSTATS_FORMS = ("thread", "lanes16", "wavefront", "workgroup_cached", "workgroup_streaming", "split")
ROWSTATS_FORMS = ("pipe_units", "pipe", "whole_column", "panel", "memory_atomics")


def colstats_form(nseg: int, nnz: int):
    """(form, nchunk): the launch form of the column statistics for ``nseg`` generalized columns with ``nnz``
    nonzeros in all, one of COLSTATS_FORMS (include/svt_hip.h, svt_dev_colstats_form).  Needs no GPU."""
    lib = load_library()
    lib.svt_dev_colstats_form.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]
    lib.svt_dev_colstats_form.restype = ctypes.c_int
    nchunk = ctypes.c_int(1)
    form = lib.svt_dev_colstats_form(int(nseg), int(nnz), ctypes.byref(nchunk))
    return COLSTATS_FORMS[form], nchunk.value


def rowstats_form(nrow: int, ncol: int, nnz: int, op: str, inner: int = 1, na_background: bool = False):
    """(form, panel_shift, nsplit): the form one pass of the row statistics takes, one of ROWSTATS_FORMS
    (include/svt_hip.h, svt_dev_rowstats_form).  ``ncol`` counts leaves.  Needs no GPU."""
    from .api import OPCODES
    lib = load_library()
    lib.svt_dev_rowstats_form.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)]
    lib.svt_dev_rowstats_form.restype = ctypes.c_int
    ps, nsplit = ctypes.c_int(0), ctypes.c_int64(1)
    form = lib.svt_dev_rowstats_form(int(nrow), int(ncol), int(nnz), int(bool(na_background)), OPCODES[op], int(inner),
                                     ctypes.byref(ps), ctypes.byref(nsplit))
    return ROWSTATS_FORMS[form], ps.value, nsplit.value


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
    lib.svt_dev_crossprod_pbc_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(_PbcPlanStruct)]
    lib.svt_dev_crossprod_pbc_plan.restype = ctypes.c_int
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
    lib.svt_dev_transpose_plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    lib.svt_dev_transpose_plan.restype = ctypes.c_int
    out = (ctypes.c_int64 * 8)()
    if lib.svt_dev_transpose_plan(int(nrow), int(ncol), int(nnz), int(nslab), out) != 0:
        raise HipBackendError(lib.svt_last_error().decode())
    d = dict(zip(TRANSPOSE_PLAN_FIELDS, (int(x) for x in out)))
    d["bucketed"], d["why_not"] = bool(d["bucketed"]), TRANSPOSE_PLAN_WHY[d["why_not"]]
    return d


def hip_dispatcher():
    from ._dispatch import CAbiDispatcher
    return CAbiDispatcher(init(), "svt_")
