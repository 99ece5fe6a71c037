"""Coercion dense array <-> sparse operand and nzwhich without a GPU: the numpy expectations of tests/coerce_cases.py
against the host container (SVT_SparseArray.from_dense / from_csc / to_dense), the ``__host__`` side of the element rules
(sparsearray_amd/csrc/svt_coerce_rules.h, through tests/coerce_rules_main.cpp), and what the library answers without a
device: the tile, the workspace query and every refusal that is decided on the host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coerce_cases as cc
from subset_cases import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGLSXP, INTSXP, REALSXP = 10, 13, 14


# ---------------------------------------------------------------------------
# the expectations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_expectation_is_what_the_host_container_makes(name):
    from sparsearray_amd import SVT_SparseArray
    a, type_, na, ans_type, (col_ptr, row_idx, val, pos) = cc.case(name)
    x = SVT_SparseArray.from_dense(a, type=type_, lacunar=False, na_background=na)
    cp, ri, vv = x.to_csc()
    assert np.array_equal(cp, col_ptr) and cp.dtype == col_ptr.dtype
    assert np.array_equal(ri, row_idx) and ri.dtype == row_idx.dtype
    vv = cc.widen(vv, type_, ans_type)
    assert vv.dtype == val.dtype and np.array_equal(bits(vv), bits(val))
    # and back: the container of the expected arrays has the dense form of the case
    back = SVT_SparseArray.from_csc(a.shape, ans_type, col_ptr, row_idx, val)
    back.na_background = na
    want = cc.dense_of(a, type_, na, ans_type)
    got = back.to_dense()
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))
    if not na and type_ == ans_type:
        assert np.array_equal(want == 0, a == 0)        # an ordinary background gives the array back up to the sign of zero


def test_every_shape_the_issue_names_is_a_case():
    T = cc.T
    shapes = {c[0] for c in cc.CASES.values()}
    assert {(1, 5000), (7, 3000), (64, 130), (65, 130), (T, 2), (T + 1, 3), (3 * T + 5, 2), (2 * T - 1,), (2 * T,),
            (2 * T + 1,), (0, 5), (5, 0), (4, 0, 3), (5, 4, 3), (3, 4, 2, 5)} <= shapes
    assert all(name + "_na" in cc.CASES for name in cc.SHAPES)
    a, _, _, _, (cp, ri, vv, pos) = cc.case("all_background")
    assert pos.size == 0 and not cp.any()
    a, _, _, _, (cp, ri, vv, pos) = cc.case("all_kept")
    assert pos.size == a.size
    for name in ("more_entry_tiles_than_the_grid", "more_entry_tiles_than_the_grid_na"):
        assert cc.case(name)[4][3].size > cc.GRID * T      # entries, not only cells: the tiles of nzwhich
    assert cc.case("more_tiles_than_the_grid")[0].size > cc.GRID * T
    cp = cc.case("empty_leaves_first_last_and_in_runs")[4][0]
    lens = np.diff(cp)
    assert not lens[:10].any() and not lens[100:300].any() and not lens[380:].any() and lens[10:100].all()
    for f, t in cc.WIDENINGS:
        assert f"widen_{f}_to_{t}" in cc.CASES and f"widen_{f}_to_{t}_na" in cc.CASES


# ---------------------------------------------------------------------------
# the host side of the rule functions
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/coerce_rules_main.cpp, built with the host compiler"""
    exe = tmp_path_factory.mktemp("coerce_rules") / "coerce_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "coerce_rules_main.cpp")], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:-1]
    return ask


def _hex(v):
    return f"{int(np.asarray(v, dtype=np.float64).reshape(1).view(np.uint64)[0]):016x}"


def test_keep_rule_on_the_special_values(rules):
    from sparsearray_amd.svt import NA_integer, NA_real
    doubles = [0.0, -0.0, 1.5, np.nan, NA_real, cc.NAN_PAYLOAD, np.inf, -np.inf, 5e-324, -5e-324]
    ints = [0, 1, -1, int(NA_integer), 2 ** 31 - 1]
    asked, want = [], []
    for na in (0, 1):
        for v in doubles:
            asked.append(f"keepd {_hex(v)} {na}")
            want.append(str(int(cc.keep_mask(np.array([v]), "double", bool(na))[0])))
        for v in ints:
            asked.append(f"keepi {v} {na}")
            want.append(str(int(cc.keep_mask(np.array([v], dtype=np.int32), "integer", bool(na))[0])))
    assert rules(asked) == want
    # spelled out: what the reference's collect_offsets_of_nonzero_* / _nonNA_* keep
    assert rules([f"keepd {_hex(-0.0)} 0", f"keepd {_hex(NA_real)} 0", f"keepd {_hex(5e-324)} 0", f"keepd {_hex(0.0)} 1",
                  f"keepd {_hex(NA_real)} 1", f"keepd {_hex(np.nan)} 1", f"keepd {_hex(cc.NAN_PAYLOAD)} 1",
                  f"keepi 0 0", f"keepi {int(NA_integer)} 0", f"keepi 0 1", f"keepi {int(NA_integer)} 1"]) == \
        ["0", "1", "1", "1", "0", "1", "1", "0", "1", "1", "0"]


def test_widen_move_and_background_rules(rules):
    from sparsearray_amd.svt import NA_integer, NA_real
    ints = [0, 1, -7, 2 ** 31 - 1, -2 ** 31 + 1, int(NA_integer)]
    want = [_hex(NA_real) if v == int(NA_integer) else _hex(float(v)) for v in ints]
    assert rules([f"widen {v}" for v in ints]) == want
    assert rules([f"movei {v}" for v in ints]) == [str(v) for v in ints]
    doubles = [-0.0, np.nan, NA_real, cc.NAN_PAYLOAD, np.inf, 5e-324]
    assert rules([f"moved {_hex(v)}" for v in doubles]) == [_hex(v) for v in doubles]
    assert rules(["bgd 0", "bgd 1", "bgi 0", "bgi 1"]) == [_hex(0.0), _hex(NA_real), "0", str(int(NA_integer))]


def test_type_status_rule(rules):
    types = [LGLSXP, INTSXP, REALSXP]
    asked = [f"status {f} {t}" for f in types for t in types] + [f"status {REALSXP} 16", f"status 15 {REALSXP}", "status 0 0"]
    want = ["0" if types.index(t) >= types.index(f) else "1" for f in types for t in types] + ["-1", "-1", "-1"]
    assert rules(asked) == want


# ---------------------------------------------------------------------------
# what the library answers without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


def test_tile_and_python_surface_need_no_gpu(lib):
    from sparsearray_amd import device
    assert lib.svt_dev_coerce_tile() == cc.T == device.coerce_tile()
    for name in ("from_dense", "to_dense", "nzwhich"):
        assert callable(getattr(device.DeviceCSC, name))


def test_ws_bytes_is_monotone_and_a_multiple_of_256(lib):
    T = cc.T
    sizes = [-5, 0, 1, 63, 64, T - 1, T, T + 1, 2 * T, 100 * T + 1, T * T, T * T + 1, 10 ** 9, 2 ** 31, 2 ** 33 + 7, 2 ** 40]
    got = [lib.svt_dev_from_dense_ws_bytes(n) for n in sizes]
    assert all(b % 256 == 0 and b > 0 for b in got)
    assert all(x <= y for x, y in zip(got, got[1:]))
    assert got[0] == got[1]
    for n, b in zip(sizes, got):                        # a base per tile and one bit per cell fit
        ntiles = max(0, -(-n // T))
        assert b >= 256 + 8 * (ntiles + 1) + 8 * 64 * ntiles


def _refused(lib, call, msg, positive=False):
    rc = call()
    assert (rc > 0) if positive else (rc < 0), rc
    assert msg in lib.svt_last_error().decode(), lib.svt_last_error().decode()


def test_from_dense_refusals_are_answered_on_the_host(lib):
    """No device is needed for any of them: nothing is launched, out_col_ptr and *out_nnz keep their contents (host
    memory here, which a launch could not have written anyway)."""
    cp = (ctypes.c_int64 * 4)(-3, -3, -3, -3)
    nnz = ctypes.c_int64(-7)
    ws_bytes = lib.svt_dev_from_dense_ws_bytes(12)
    x = 4096                                            # never read

    def count(x_type, nrow, nleaves, ans, ws=ws_bytes):
        return lambda: lib.svt_dev_from_dense_count(x, x_type, nrow, nleaves, ans, 0, cp, ctypes.byref(nnz), 8192, ws, None)

    def fill(x_type, nrow, nleaves, ans, ws=ws_bytes):
        return lambda: lib.svt_dev_from_dense_fill(x, x_type, nrow, nleaves, ans, 0, cp, 8192, 8192, 8192, ws, None)

    def whole(x_type, nrow, nleaves, ans):
        from sparsearray_amd._abi import ALLOC_FN, FREE_FN
        return lambda: lib.svt_dev_from_dense(x, x_type, nrow, nleaves, ans, 0, ALLOC_FN(), FREE_FN(), None, ctypes.byref(nnz),
                                              None, None, None, None)          # (NULL function pointers)
    for make in (count, fill, whole):
        _refused(lib, make(16, 4, 3, REALSXP), "the types must be logical, integer or double")
        _refused(lib, make(REALSXP, 4, 3, 9), "the types must be logical, integer or double")
        _refused(lib, make(REALSXP, 4, 3, INTSXP), "coercion to a narrower type is not supported here", positive=True)
        _refused(lib, make(INTSXP, 4, 3, LGLSXP), "coercion to a narrower type is not supported here", positive=True)
        _refused(lib, make(REALSXP, -1, 3, REALSXP), "negative extent")
        _refused(lib, make(REALSXP, 4, -3, REALSXP), "negative extent")
        _refused(lib, make(REALSXP, 2 ** 31, 3, REALSXP), "more than 2^31 - 1 rows")
        _refused(lib, make(REALSXP, 2 ** 31 - 1, 2 ** 33, REALSXP), "nrow * nleaves overflows 64 bits")
    for make in (count, fill):
        _refused(lib, make(REALSXP, 4, 3, REALSXP, ws=ws_bytes - 1), "workspace too small")
        _refused(lib, make(REALSXP, 0, 3, REALSXP, ws=lib.svt_dev_from_dense_ws_bytes(0) - 1), "workspace too small")
    _refused(lib, whole(REALSXP, 4, 3, REALSXP), "an allocator is needed")
    assert list(cp) == [-3, -3, -3, -3] and nnz.value == -7


def _bare(lib, Rtype, nrow, ncol, nnz):
    h = lib.svt_wrap_device_csc(Rtype, nrow, ncol, nnz, 4096, 4096, 4096)      # pointers that are never followed
    assert h
    return h


def test_to_dense_refusals_are_answered_on_the_host(lib):
    h = _bare(lib, INTSXP, 5, 4, 3)
    d = _bare(lib, REALSXP, 5, 4, 3)
    try:
        _refused(lib, lambda: lib.svt_dev_to_dense(None, 0, REALSXP, 4096, None, None), "the operand is NULL")
        _refused(lib, lambda: lib.svt_dev_to_dense(h, 0, 9, 4096, None, None), "the types must be logical, integer or double")
        _refused(lib, lambda: lib.svt_dev_to_dense(h, 0, LGLSXP, 4096, None, None), "narrower type", positive=True)
        _refused(lib, lambda: lib.svt_dev_to_dense(d, 0, INTSXP, 4096, None, None), "narrower type", positive=True)
        _refused(lib, lambda: lib.svt_dev_to_dense(d, 0, REALSXP, 4096 + 8, None, None), "aligned to 16 bytes")
    finally:
        lib.svt_release(h)
        lib.svt_release(d)
    # an output without cells: done, and nothing launched (there is no device to launch on)
    for nrow, ncol in ((0, 4), (5, 0)):
        e = _bare(lib, REALSXP, nrow, ncol, 0)
        try:
            assert lib.svt_dev_to_dense(e, 0, REALSXP, None, None, None) == 0
        finally:
            lib.svt_release(e)


def test_nzwhich_refusals_are_answered_on_the_host(lib):
    dims = lambda *d: (ctypes.c_int64 * len(d))(*d)                             # noqa: E731
    h = _bare(lib, REALSXP, 5, 12, 3)
    big = _bare(lib, REALSXP, 5, 12, 2 ** 31)
    empty = _bare(lib, REALSXP, 5, 12, 0)
    try:
        call = lambda hh, nd, d, ai: (lambda: lib.svt_dev_nzwhich(hh, nd, d, ai, 4096, None))     # noqa: E731
        _refused(lib, call(None, 2, dims(5, 12), 0), "the operand is NULL")
        _refused(lib, call(h, 0, dims(5, 12), 0), "between 1 and 8 dimensions")
        _refused(lib, call(h, 9, dims(*([1] * 9)), 0), "between 1 and 8 dimensions")
        for bad in ((4, 12), (5, 11), (5, 3, 5), (5, -3, -4)):
            _refused(lib, call(h, len(bad), dims(*bad), 0), "'dim' does not match" if min(bad) >= 0 else "an extent outside")
        _refused(lib, call(h, 1, dims(5), 1), "'dim' does not match the operand's rows and leaves")
        wide = _bare(lib, REALSXP, 1, 2 ** 31, 3)
        try:
            _refused(lib, call(wide, 3, dims(1, 65536, 32768), 0), "more than 2^31 - 1 leaves")
        finally:
            lib.svt_release(wide)
        _refused(lib, call(big, 3, dims(5, 3, 4), 1),
                 'too many nonzero elements in SVT_SparseArray object to return their "array coordinates" (n-tuples) in a matrix')
        for ai in (0, 1):                               # no entries: done, nothing launched
            assert lib.svt_dev_nzwhich(empty, 3, dims(5, 3, 4), ai, None, None) == 0
    finally:
        for x in (h, big, empty):
            lib.svt_release(x)


def test_abi_table_has_the_new_rows():
    from sparsearray_amd._abi import PROTOTYPES
    for name in ("svt_dev_coerce_tile", "svt_dev_from_dense_ws_bytes", "svt_dev_from_dense_count", "svt_dev_from_dense_fill",
                 "svt_dev_from_dense", "svt_dev_to_dense", "svt_dev_nzwhich"):
        assert name in PROTOTYPES
