"""abind / cbind / rbind without a GPU: the R-level logic of Session.abind (.abind_SparseArray_objects,
R/SparseArray-abind.R:53-85) against a recording dispatcher, the expectation of tests/abind_cases.py (numpy's
concatenation) against a per-leaf restatement of concatenate_leaves / concatenate_SVTs, and what the library answers
without a device: the tile, the workspace sizes and every refusal (all of them are decided on the host).

(The file name sorts last, like test_z_compare_cpu.py: the files of the CPU suite that were there before keep their
place in the run.)"""
import ctypes

import numpy as np
import pytest

import abind_cases as ab
from sparsearray_amd import SVT_SparseArray, SparseArrayError, SparseArrayUnsupported
from sparsearray_amd.api import Session
from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP

ENTRY = "C_abind_SVT_SparseArray_objects"


class Recorder:
    """offers every entry point, records the calls and answers abind by the per-leaf restatement"""

    def __init__(self):
        self.calls = []

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        assert name == ENTRY
        objects, along, ans_type = args
        return ab.restate(objects, along, ans_type)


@pytest.fixture()
def rec():
    r = Recorder()
    return Session(r), r


def _named(x, names):
    return SVT_SparseArray(x.dim, x.type, x.leaves, dimnames=names, na_background=x.na_background)


# ---------------------------------------------------------------------------
# the expectation itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ab.NAMES)
def test_numpy_expectation_agrees_with_the_per_leaf_restatement(name):
    along, objects, ans_type, _, _ = ab.case(name)
    ndim = max(along, max(x.ndim for x in objects))
    ab.check(ab.restate([Session._add_missing_dims(x, ndim) for x in objects], along, ans_type), name)


@pytest.mark.parametrize("name", ab.NAMES)
def test_session_passes_the_case_through_one_call(rec, name):
    s, r = rec
    along, objects, ans_type, _, _ = ab.case(name)
    res = s.abind(*objects, along=along)
    if len(objects) == 1:
        assert res is objects[0] and r.calls == []
        return
    ab.check(res, name)
    (call,) = r.calls
    assert call[0] == ENTRY and call[2] == along and call[3] == ans_type
    assert [x.dim for x in call[1]] == ab.padded_dims(name)


def test_tile_constant_is_the_library_s():
    from sparsearray_amd.device import abind_tile
    assert abind_tile() == ab.T


# ---------------------------------------------------------------------------
# the Session logic
# ---------------------------------------------------------------------------
def test_none_objects_zero_objects_one_object(rec):
    s, r = rec
    a, b = ab.obj((5, 3), seed=1), ab.obj((7, 3), seed=2)
    assert s.abind() is None and s.abind(None, None) is None and s.cbind() is None and s.rbind(None) is None
    assert s.abind(None, a, None) is a and s.rbind(a) is a and s.cbind(None, a) is a
    assert r.calls == []
    res = s.abind(None, a, None, b, along=1)
    assert res.dim == (12, 3) and len(r.calls) == 1 and [x is y for x, y in zip(r.calls[0][1], (a, b))] == [True, True]
    padded = s.abind(a, along=3)                        # one object, a new dimension: the object with its trailing 1
    assert padded.dim == (5, 3, 1) and padded.leaves is a.leaves and len(r.calls) == 1


def test_along_default_new_dimension_and_rev_along(rec):
    s, r = rec
    a, b = ab.obj((4, 3, 2), seed=1), ab.obj((4, 3, 2), seed=2)
    assert s.abind(a, b).dim == (4, 3, 4) and r.calls[-1][2] == 3                  # default: the last dimension
    assert s.abind(a, b, along=4).dim == (4, 3, 2, 2) and r.calls[-1][2] == 4      # N + 1
    assert [x.dim for x in r.calls[-1][1]] == [(4, 3, 2, 1)] * 2
    assert s.abind(a, b, rev_along=0).dim == (4, 3, 2, 2) and r.calls[-1][2] == 4
    assert s.abind(a, b, rev_along=1).dim == (4, 3, 4) and r.calls[-1][2] == 3
    assert s.abind(a, b, rev_along=3).dim == (8, 3, 2) and r.calls[-1][2] == 1
    assert s.abind(a, b, along=np.int64(2)).dim == (4, 6, 2) and r.calls[-1][2] == 2
    assert s.cbind(a, b).dim == (4, 6, 2) and s.rbind(a, b).dim == (8, 3, 2)


def test_objects_of_fewer_dimensions_get_trailing_ones(rec):
    s, r = rec
    a, m = ab.obj((4, 3, 2), seed=1), ab.obj((4, 3), seed=2)
    res = s.abind(a, m)                                 # N = 3: the matrix is a 4 x 3 x 1 slab
    assert res.dim == (4, 3, 3) and [x.dim for x in r.calls[-1][1]] == [(4, 3, 2), (4, 3, 1)]
    want = np.concatenate([a.to_dense(), m.to_dense()[:, :, None]], axis=2)
    assert np.array_equal(res.to_dense(), want)
    v = ab.obj((4,), seed=3)
    assert s.abind(v, m, along=2).dim == (4, 4) and [x.dim for x in r.calls[-1][1]] == [(4, 1), (4, 3)]


@pytest.mark.parametrize("t1", ab.TYPE_ORDER)
@pytest.mark.parametrize("t2", ab.TYPE_ORDER)
def test_type_rule_for_every_pair(rec, t1, t2):
    s, r = rec
    res = s.rbind(ab.obj((5, 3), t1, seed=1, palette="specials"), ab.obj((4, 3), t2, seed=2, palette="specials"))
    want = ab.TYPE_ORDER[max(ab.TYPE_ORDER.index(t1), ab.TYPE_ORDER.index(t2))]
    assert res.type == want and r.calls[-1][3] == want
    assert [x.type for x in r.calls[-1][1]] == [t1, t2]         # the objects go over as they are: the library widens


def test_dimnames_off_the_binding_dimension_are_the_first_non_null(rec):
    s, _ = rec
    a, b, c = ab.obj((2, 3), seed=1), ab.obj((4, 3), seed=2), ab.obj((1, 3), seed=3)
    assert s.rbind(a, b, c).dimnames is None
    res = s.rbind(a, _named(b, [None, ["x", "y", "z"]]), _named(c, [None, ["p", "q", "r"]]))
    assert res.dimnames == [None, ["x", "y", "z"]]
    res = s.abind(_named(ab.obj((2, 3), seed=1), [["r1", "r2"], None]), ab.obj((2, 3), seed=2), along=3)
    assert res.dimnames == [["r1", "r2"], None, None]


def test_dimnames_along_the_binding_dimension_are_concatenated_with_blanks(rec):
    s, _ = rec
    a, b, c = ab.obj((2, 3), seed=1), ab.obj((4, 3), seed=2), ab.obj((1, 3), seed=3)
    res = s.rbind(a, _named(b, [["b1", "b2", "b3", "b4"], None]), c)
    assert res.dimnames == [["", "", "b1", "b2", "b3", "b4", ""], None]
    res = s.rbind(_named(a, [["a1", "a2"], ["x", "y", "z"]]), _named(b, [None, ["no", "no", "no"]]),
                  _named(c, [["c1"], None]))
    assert res.dimnames == [["a1", "a2", "", "", "", "", "c1"], ["x", "y", "z"]]
    res = s.cbind(_named(ab.obj((2, 0)), [["r1", "r2"], []]), _named(ab.obj((2, 2), seed=4), [None, ["u", "v"]]))
    assert res.dimnames == [["r1", "r2"], ["u", "v"]]


def test_every_error_is_raised_before_a_call():
    from test_arith_cpu import NoCall
    s = Session(NoCall())
    a, b = ab.obj((4, 3, 2), seed=1), ab.obj((4, 3, 2), seed=2)
    for bad in (0, -1, 5):
        with pytest.raises(SparseArrayError, match="'along' must be >= 1 and <= the largest number of dimensions"):
            s.abind(a, b, along=bad)
    with pytest.raises(SparseArrayError, match="'rev.along' must be >= 0"):
        s.abind(a, b, rev_along=-1)
    with pytest.raises(SparseArrayError, match="'along' must be >= 1"):
        s.abind(a, b, rev_along=4)
    with pytest.raises(SparseArrayError, match="'along' must be a single integer"):
        s.abind(a, b, along=1.5)
    with pytest.raises(SparseArrayError, match="'rev.along' must be a single integer"):
        s.abind(a, b, rev_along=True)
    with pytest.raises(SparseArrayError, match="only one of 'along' and 'rev.along'"):
        s.abind(a, b, along=1, rev_along=1)
    with pytest.raises(SparseArrayError, match=r"same extent along dimension 2 \(they are bound along dimension 1\)"):
        s.rbind(a, ab.obj((4, 2, 2)))
    with pytest.raises(SparseArrayError, match=r"same extent along dimension 1 \(they are bound along dimension 2\)"):
        s.cbind(ab.obj((4, 3)), ab.obj((5, 3)))
    with pytest.raises(SparseArrayError, match=r"same extent along dimension 3 \(they are bound along dimension 1\)"):
        s.rbind(a, ab.obj((4, 3)))                      # the matrix is 4 x 3 x 1
    with pytest.raises(SparseArrayError, match="NaArray objects and ordinary SparseArray objects cannot be bound"):
        s.rbind(ab.obj((4, 3)), ab.obj((4, 3), na_background=True))
    with pytest.raises(SparseArrayUnsupported, match="dense array"):
        s.rbind(ab.obj((4, 3)), np.zeros((4, 3)))
    with pytest.raises(SparseArrayError, match="takes SVT_SparseArray objects"):
        s.rbind(ab.obj((4, 3)), "x")


def test_a_library_without_the_entry_is_unsupported():
    class Lacking:
        def has_entry(self, name):
            return False

        def __call__(self, name, *args):
            raise AssertionError(f"{name} was called")

    s = Session(Lacking())
    with pytest.raises(SparseArrayUnsupported, match="C_abind_SVT_SparseArray_objects is not offered"):
        s.rbind(ab.obj((4, 3)), ab.obj((5, 3)))
    a = ab.obj((4, 3))
    assert s.rbind(a) is a and s.abind() is None         # no call: no entry needed

    class NoQuery:                                      # a dispatcher that cannot say: the entry counts as missing
        def __call__(self, name, *args):
            raise AssertionError(f"{name} was called")
    with pytest.raises(SparseArrayUnsupported):
        Session(NoQuery()).cbind(a, a)


# ---------------------------------------------------------------------------
# the library without a device: sizes and refusals (all decided on the host, before a launch)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


def test_ws_bytes(lib):
    f = lib.svt_dev_abind_ws_bytes
    assert f(1, 0, 0) % 256 == 0 and f(1, 0, 0) >= 3 * 256
    # carved at multiples of 256: the head, 64 bytes per object, 8 per piece start, 24 per piece, the scan's scratch
    assert f(4, 0, 0) == f(1, 0, 0) and f(5, 0, 0) == f(1, 0, 0) + 256
    for nobj, nl in ((2, 1000), (70, 333), (3, 100000)):
        rows, leaf = f(nobj, nl, 1), f(nobj, nl, 0)
        assert rows % 256 == 0 and leaf % 256 == 0
        assert rows == f(nobj, nl * nobj, 0)            # the rows form has nobj pieces per leaf
        assert leaf >= 256 + 64 * nobj + 8 * (nl + 1) + 24 * nl
    assert all(f(2, n + 1, 0) >= f(2, n, 0) for n in range(0, 9000, 61))
    assert f(-1, -5, 0) == f(0, 0, 0)


_host_handles = ab.bare_handles


REFUSALS = ab.REFUSALS


@pytest.mark.parametrize("what,specs,nobj,inner,ext,ans,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_gpu(lib, what, specs, nobj, inner, ext, ans, msg):
    """status < 0 with the outputs untouched, from the count call, the fill call and the composition alike; the
    allocator of the composition is never asked"""
    import re
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN
    hs, table = _host_handles(lib, specs)
    try:
        n = len(hs) if nobj is None else nobj
        e = None if ext is None else (ctypes.c_int64 * len(ext))(*ext)
        cp = np.full(8, -7, dtype=np.int64)
        nnz = ctypes.c_int64(-7)
        ws = np.full(1 << 16, 0xA5, dtype=np.uint8)
        assert lib.svt_dev_abind_count(table, n, inner, e, ans, cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data, ws.size,
                                       None) < 0
        assert re.search(msg, lib.svt_last_error().decode()), lib.svt_last_error().decode()
        assert lib.svt_dev_abind_fill(table, n, inner, e, ans, cp.ctypes.data, None, None, ws.ctypes.data, ws.size, None) < 0
        asked = []
        alloc = ALLOC_FN(lambda nbytes, ctx: asked.append(nbytes))
        release = FREE_FN(lambda p, ctx: None)
        outs = [ctypes.c_int64(-7) for _ in range(3)] + [ctypes.c_void_p(0) for _ in range(3)]
        assert lib.svt_dev_abind(table, n, inner, e, ans, alloc, release, None, *[ctypes.byref(o) for o in outs], None) < 0
        assert asked == [] and [o.value for o in outs[:3]] == [-7] * 3 and not any(o.value for o in outs[3:])
        assert (cp == -7).all() and nnz.value == -7 and (ws == 0xA5).all()
    finally:
        for h in hs:
            lib.svt_release(h)


def test_null_object_mixed_background_and_small_workspace_need_no_gpu(lib):
    from sparsearray_amd._hip import load_library  # noqa: F401
    hs, table = _host_handles(lib, [(REALSXP, 4, 3), (REALSXP, 5, 3)])
    try:
        cp = np.full(8, -7, dtype=np.int64)
        nnz = ctypes.c_int64(-7)
        ws = np.full(1 << 16, 0xA5, dtype=np.uint8)
        args = (1, None, REALSXP, cp.ctypes.data, ctypes.byref(nnz), ws.ctypes.data)
        with_null = (ctypes.c_void_p * 2)(hs[0], None)
        assert lib.svt_dev_abind_count(with_null, 2, *args, ws.size, None) < 0
        assert "object 2 is NULL" in lib.svt_last_error().decode()
        assert lib.svt_dev_abind_count(None, 2, *args, ws.size, None) < 0
        need = lib.svt_dev_abind_ws_bytes(2, 3, 1)
        assert lib.svt_dev_abind_count(table, 2, *args, need - 1, None) < 0
        assert "workspace too small" in lib.svt_last_error().decode()
        assert lib.svt_dev_abind_fill(table, 2, 1, None, REALSXP, cp.ctypes.data, None, None, ws.ctypes.data, need - 1, None) < 0
        assert "workspace too small" in lib.svt_last_error().decode()
        # struct svt_dev_csc: na_background is the int32 after the three pointers (include/svt_hip.h)
        ctypes.c_int32.from_address(hs[1] + 56).value = 1
        assert lib.svt_dev_abind_count(table, 2, *args, ws.size, None) < 0
        assert "NaArray objects and ordinary objects" in lib.svt_last_error().decode()
        assert (cp == -7).all() and nnz.value == -7 and (ws == 0xA5).all()
    finally:
        for h in hs:
            lib.svt_release(h)
