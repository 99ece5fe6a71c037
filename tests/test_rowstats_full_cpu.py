"""The Python side of the one-call row statistics (Session._rowStats over C_rowStatsFull_SVT), without a GPU.

A dispatcher that offers C_rowStatsFull_SVT is stood in by a stub around the oracle's: one that refuses every call
(status > 0: the generics must fall back to the composition of the R methods and return exactly what the plain
oracle session returns), and one that answers with a canned buffer (the generics must shape it: column-major,
and for rowRanges the minima and the maxima stacked on a new last axis)."""
import warnings

import numpy as np
import pytest

from sparsearray_amd import NA_integer, NA_real, SparseArrayError, SVT_SparseArray
from sparsearray_amd.api import Session, SparseArrayUnsupported
from helpers import assert_identical

GENERICS = ["rowAnys", "rowAlls", "rowProds", "rowMeans", "rowVars", "rowSds", "rowRanges"]


class _Stub:
    """The oracle dispatcher plus a C_rowStatsFull_SVT entry that refuses (canned is None) or answers `canned`."""

    def __init__(self, inner, canned=None, warn=False):
        self._inner, self._canned, self._warn = inner, canned, warn
        self.calls = []

    def has_entry(self, name):
        return name == "C_rowStatsFull_SVT" or self._inner.has_entry(name)

    def __call__(self, name, *args):
        self.calls.append(name)
        if name == "C_rowStatsFull_SVT":
            if self._canned is None:
                raise SparseArrayUnsupported("stub: not supported here")
            return self._canned, self._warn
        return self._inner(name, *args)

    def __getattr__(self, name):
        return getattr(self._inner, name)


def _operands():
    rng = np.random.default_rng(7)
    out = []
    for dim in [(40, 7), (12, 4, 3)]:
        mask = rng.random(dim) < 0.5
        d = np.asfortranarray(np.where(mask, rng.uniform(0.5, 2.0, dim), 0.0))
        d.reshape(-1, order="F")[[3, 17]] = [NA_real, np.nan]
        i = np.asfortranarray(np.where(mask, rng.integers(-3, 4, dim), 0).astype(np.int32))
        i.reshape(-1, order="F")[[5, 11]] = NA_integer
        i[1, ...] = 2                                        # a fully covered row
        out.append(SVT_SparseArray.from_dense(d, type="double"))
        out.append(SVT_SparseArray.from_dense(i, type="integer"))
        out.append(SVT_SparseArray.from_dense(i != 0, type="logical"))
    return out


@pytest.mark.parametrize("na_rm", [False, True])
def test_refused_call_falls_back_to_the_composition(oracle, na_rm):
    stub = _Stub(oracle._call)
    s = Session(stub)
    for x in _operands():
        for dims in range(1, x.ndim):
            for fn in GENERICS:
                if x.type == "double" and fn in ("rowAnys", "rowAlls"):
                    continue
                stub.calls.clear()
                got = getattr(s, fn)(x, na_rm=na_rm, dims=dims)
                want = getattr(oracle, fn)(x, na_rm=na_rm, dims=dims)
                assert_identical(got, want, f"{fn} {x.type} {x.dim} dims={dims}")
                assert stub.calls[0] == "C_rowStatsFull_SVT" and stub.calls.count("C_rowStatsFull_SVT") == 1
                assert len(stub.calls) > 1


def test_refused_call_keeps_center_and_checks(oracle):
    s = Session(_Stub(oracle._call))
    x = _operands()[0]
    center = np.linspace(0.0, 1.0, x.dim[0])
    for fn in ("rowVars", "rowSds"):
        assert_identical(getattr(s, fn)(x, center=center), getattr(oracle, fn)(x, center=center), fn)
        assert_identical(getattr(s, fn)(x, center=0.25), getattr(oracle, fn)(x, center=0.25), fn)
        with pytest.raises(SparseArrayError, match="unexpected 'center' length"):
            getattr(s, fn)(x, center=np.zeros(3))
    with pytest.raises(SparseArrayError, match="'dims' must be a single integer"):
        s.rowMeans(x, dims=2)
    # dims = 0 is the col*() form over everything: never the row entry point
    stub = _Stub(oracle._call)
    assert_identical(Session(stub).rowMeans(x, dims=0), oracle.rowMeans(x, dims=0))
    assert "C_rowStatsFull_SVT" not in stub.calls


def test_naarray_errors_stay(oracle):
    d = np.full((6, 3), NA_real)
    d[1, :] = 2.0
    x = SVT_SparseArray.from_dense(d, type="double", na_background=True)
    stub = _Stub(oracle._call)
    s = Session(stub)
    for fn in ("rowAnys", "rowAlls", "rowProds", "rowMeans", "rowVars", "rowSds"):
        with pytest.raises(SparseArrayError, match="unable to find an inherited method"):
            getattr(s, fn)(x)
    assert stub.calls == []
    assert_identical(s.rowRanges(x), oracle.rowRanges(x))    # refused: rowMins and rowMaxs, stacked


def test_canned_answer_is_shaped(oracle):
    x3 = SVT_SparseArray.from_dense(np.ones((3, 2, 4)), type="double")
    n = 6
    canned = np.arange(n, dtype=np.float64)
    for fn in ("rowProds", "rowMeans", "rowVars", "rowSds"):
        stub = _Stub(oracle._call, canned)
        got = getattr(Session(stub), fn)(x3, dims=2)
        assert stub.calls == ["C_rowStatsFull_SVT"]
        assert got.shape == (3, 2)
        assert_identical(got, canned.reshape((3, 2), order="F"), fn)
        got = getattr(Session(_Stub(oracle._call, canned[:3])), fn)(x3, dims=1)
        assert got.shape == (3,)
        assert_identical(got, canned[:3], fn)
    both = np.arange(2 * n, dtype=np.float64)
    stub = _Stub(oracle._call, both)
    got = Session(stub).rowRanges(x3, dims=2)
    assert stub.calls == ["C_rowStatsFull_SVT"]
    assert got.shape == (3, 2, 2)
    assert_identical(got[..., 0], both[:n].reshape((3, 2), order="F"), "minima")
    assert_identical(got[..., 1], both[n:].reshape((3, 2), order="F"), "maxima")
    got = Session(_Stub(oracle._call, both[:6])).rowRanges(x3, dims=1)
    assert got.shape == (3, 2)
    assert_identical(got, np.stack([both[:3], both[3:6]], axis=-1), "rowRanges dims=1")
    xi = SVT_SparseArray.from_dense(np.ones((3, 2), dtype=np.int32), type="integer")
    flags = np.array([1, 0, NA_integer], dtype=np.int32)
    assert_identical(Session(_Stub(oracle._call, flags)).rowAnys(xi), flags)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        Session(_Stub(oracle._call, np.zeros(6, np.int32), warn=True)).rowRanges(xi)
    assert any("NAs introduced" in str(m.message) for m in w)


def test_na_rm_check_of_the_composed_route_stays(oracle):
    """rowAnys / rowAlls / rowProds reached .colStats_SparseArray's "'na.rm' must be TRUE or FALSE" through the
    composition; the one-call route raises it too, before the call."""
    xi = SVT_SparseArray.from_dense(np.ones((3, 2), dtype=np.int32), type="integer")
    stub = _Stub(oracle._call, np.zeros(3, np.int32))
    s = Session(stub)
    for fn in ("rowAnys", "rowAlls", "rowProds"):
        for bad in (1, None, "yes"):
            for session in (oracle, s):
                with pytest.raises(SparseArrayError, match="'na.rm' must be TRUE or FALSE"):
                    getattr(session, fn)(xi, na_rm=bad)
    assert stub.calls == []
    assert_identical(s.rowAnys(xi, na_rm=np.bool_(True)), np.zeros(3, np.int32))
