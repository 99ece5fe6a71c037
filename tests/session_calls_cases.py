"""What tests/test_session_calls_cpu.py and tests/test_hip_session_calls.py share: the operands, a dispatcher that records
the ``.Call`` names a Session issues, and the list of calls whose results tests/golden/session_calls.json holds.

The operands are the smallest that have an NA, a stored zero and an empty leaf in different columns, plus an empty row.
Every value is a small integer ("tracer" values, tests/exact_stats.py: every sum of a row or a column is exact in any
order), and every row's mean is an integer, with the NA or without it, so the centred sums of the rows are integers too:
whatever route computes a statistic of them, the answer is the same bits."""
from __future__ import annotations

import numpy as np

from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray
from sparsearray_amd.api import SparseArrayError, SparseArrayUnsupported

FULL = "C_rowStatsFull_SVT"


def _five_by_four(type_):
    na, dt = (NA_real, np.float64) if type_ == "double" else (NA_integer, np.int32)
    leaf = lambda offs, vals: (np.asarray(offs, dtype=np.int32), np.asarray(vals, dtype=dt))
    leaves = [leaf([0, 1, 2], [4, na, -8]),          # the NA
              leaf([0, 2, 3], [12, 0, 2]),           # the stored zero
              None,                                  # the empty column
              leaf([0, 1, 2, 3], [-4, 6, 16, -6])]   # (row 5 is empty)
    return SVT_SparseArray((5, 4), type_, leaves)


def _na_twin(x):
    d = x.to_dense()
    stored = np.zeros(d.shape, dtype=bool)
    for j, lf in enumerate(x.leaves):
        if lf is not None:
            stored[lf[0], j] = True
    d[~stored] = NA_real if x.type == "double" else NA_integer
    return SVT_SparseArray.from_dense(d, type=x.type, na_background=True)


def operands():
    x, xi = _five_by_four("double"), _five_by_four("integer")
    d3 = np.asfortranarray(np.array([[[1, 0], [0, 2], [3, -4]], [[0, 5], [-6, 0], [0, 0]]], dtype=np.float64))
    return {"X": x, "XI": xi, "XNA": _na_twin(x), "XINA": _na_twin(xi), "X3": SVT_SparseArray.from_dense(d3),
            "Z04": SVT_SparseArray((0, 4), "double", [None] * 4), "Z50": SVT_SparseArray((5, 0), "double", [])}


class Recorder:
    """A dispatcher around ``inner`` that records the name of every ``.Call`` a Session issues through it.  ``full``:
    None leaves C_rowStatsFull_SVT to ``inner``; "no" denies the entry; "refuse" claims it and answers "not supported
    here" (status > 0); "answer" claims it and answers 1, 2, 3, ... in the length the call asks for."""

    def __init__(self, inner, full=None):
        self._inner, self.full, self.calls = inner, full, []

    def has_entry(self, name):
        if name == FULL and self.full is not None:
            return self.full != "no"
        return self._inner.has_entry(name)

    def __call__(self, name, *args):
        self.calls.append(name)
        if name == FULL and self.full is not None:
            if self.full != "answer":
                raise SparseArrayUnsupported("recorder: not supported here")
            x, op, _, _, dims = args
            n = int(np.prod(x.dim[:dims])) * (2 if op == "range" else 1)
            return np.arange(1, n + 1, dtype=np.float64), False
        return self._inner(name, *args)

    def __getattr__(self, name):
        return getattr(self._inner, name)


# ---- the order statistics and subset(): (method, args, kwargs), run on X and on XI -----------------------------------
TIES = ("max", "average", "min", "dense")
ORDER_CALLS = [
    ("colMedians", (), {}), ("colMedians", (), {"na_rm": True}),
    ("rowMedians", (), {}), ("rowMedians", (), {"na_rm": True}),
    ("colQuantiles", (), {}), ("colQuantiles", ((0.1, 0.9),), {"na_rm": True}),
    ("rowQuantiles", (), {}), ("rowQuantiles", ((0.1, 0.9),), {"na_rm": True}),
    ("colIQRs", (), {"na_rm": True}), ("rowIQRs", (), {"na_rm": True}),
    ("colMads", (), {}), ("colMads", (), {"center": 1.0, "na_rm": True}),
    ("colMads", (), {"center": [1.0, 2.0, 0.0, -1.0], "constant": 1.0}),
    ("rowMads", (), {}), ("rowMads", (), {"center": [1.0, 2.0, 0.0, -1.0, 3.0], "na_rm": True}),
    *[("colRanks", (t,), {}) for t in TIES], ("colRanks", ("average",), {"preserve_shape": True}),
    *[("rowRanks", (t,), {}) for t in TIES],
    ("subset", ([3, 1, 1], [4, 2]), {}), ("subset", (), {}), ("subset", (None, [3]), {}), ("subset", ([5, 2], None), {}),
]
ENTRY_OF = {"colIQRs": "C_colQuantiles_SVT", "rowIQRs": "C_rowQuantiles_SVT", "subset": "C_subset_SVT_by_Nindex"}


def entry_of(method):
    return ENTRY_OF.get(method, f"C_{method}_SVT")


# ---- operands with a zero extent: the R-level answers, and what is still called ---------------------------------------
# A column form answers nrow == 0 itself (colRanks: either extent); a row form transposes and takes the column form.
T = "C_transpose_2D_SVT"
ZERO_EXTENT_CALLS = {
    ("colMedians", "Z04"): [], ("colMedians", "Z50"): ["C_colMedians_SVT"],
    ("colQuantiles", "Z04"): [], ("colQuantiles", "Z50"): ["C_colQuantiles_SVT"],
    ("colMads", "Z04"): [], ("colMads", "Z50"): ["C_colMads_SVT"],
    ("colRanks", "Z04"): [], ("colRanks", "Z50"): [],
    ("rowMedians", "Z04"): [T, "C_colMedians_SVT"], ("rowMedians", "Z50"): [T],
    ("rowQuantiles", "Z04"): [T, "C_colQuantiles_SVT"], ("rowQuantiles", "Z50"): [T],
    ("rowMads", "Z04"): [T, "C_colMads_SVT"], ("rowMads", "Z50"): [T],
    ("rowRanks", "Z04"): [T], ("rowRanks", "Z50"): [T],
}

# ---- the row statistics ---------------------------------------------------------------------------------------------------
ROW_METHODS = ("rowAnyNAs", "rowCountNAs", "rowAnys", "rowAlls", "rowMins", "rowMaxs", "rowRanges", "rowSums", "rowProds",
               "rowMeans", "rowVars", "rowSds")
LOGICAL_ONLY = ("rowAnys", "rowAlls")                 # (no method for a "double" operand)
# the columns of the route table: (C_rowStatsFull_SVT: "no" / "answer" / "refuse", dims == 0, NaArray)
COLUMNS = [(full, dims0, na) for na in (False, True) for full in ("no", "answer", "refuse") for dims0 in (False, True)]


def row_cases():
    """(id, method, operand, kwargs, full) of every cell of the route table, on every operand type that has the method;
    then the 3-D operand, where aperm() stands for t()."""
    out = []
    for m in ROW_METHODS:
        na_rms = (False, True) if m in ("rowMeans", "rowVars", "rowSds") else (False,)
        for full, dims0, na in COLUMNS:
            for key in (("XINA",) if na else ("XI",)) + (() if m in LOGICAL_ONLY else (("XNA",) if na else ("X",))):
                for na_rm in na_rms:
                    kw = {"dims": 0 if dims0 else 1}
                    if m not in ("rowAnyNAs", "rowCountNAs"):
                        kw["na_rm"] = na_rm
                    out.append((f"{m}|{key}|{full}|dims={kw['dims']}|na_rm={na_rm}", m, key, kw, full))
        if m in LOGICAL_ONLY:
            continue
        for full in ("no", "answer", "refuse"):
            for dims in (1, 2):
                kw = {"dims": dims} if m in ("rowAnyNAs", "rowCountNAs") else {"dims": dims, "na_rm": False}
                out.append((f"{m}|X3|{full}|dims={dims}|na_rm=False", m, "X3", kw, full))
    for m, kw in (("rowVars", {"center": [1.0, 2.0, 0.0, -1.0, 3.0]}), ("rowSds", {"center": 0.5})):
        for full in ("no", "refuse"):
            out.append((f"{m}|X|{full}|center", m, "X", kw, full))
    return out


def order_cases():
    out = []
    for key in ("X", "XI"):
        for n, (m, args, kw) in enumerate(ORDER_CALLS):
            out.append((f"{m}|{key}|{n}", m, key, args, kw))
    for (m, key) in ZERO_EXTENT_CALLS:
        args = ("average",) if m.endswith("Ranks") else ()
        out.append((f"{m}|{key}", m, key, args, {}))
    return out


def run(session_of, ops, method, key, args, kw, full=None):
    """One call on a fresh recording session: (result or the SparseArrayError it raised, the .Call names)."""
    import warnings
    rec = Recorder(session_of._call, full)
    s = type(session_of)(rec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            res = getattr(s, method)(ops[key], *args, **kw)
        except SparseArrayError as e:
            res = e
    return res, rec.calls


# ---- results as JSON ------------------------------------------------------------------------------------------------------
def _nd(a):
    a = np.asarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "f_contiguous": bool(a.flags.f_contiguous),
            "hex": a.tobytes(order="F").hex()}


def encode(res):
    if isinstance(res, SparseArrayError):
        return {"error": type(res).__name__, "text": str(res)}
    if isinstance(res, SVT_SparseArray):
        cp, ri, vv = res.to_csc()
        return {"svt": {"dim": list(res.dim), "type": res.type, "na_background": res.na_background,
                        "dimnames": res.dimnames, "col_ptr": _nd(cp), "row_idx": _nd(ri), "val": _nd(vv)}}
    return _nd(res)


def same_nd(got, want):
    """Values (any two NaNs of the same bits or not: ``equal_nan``), dtype and memory order."""
    got = np.asarray(got)
    exp = np.frombuffer(bytes.fromhex(want["hex"]), dtype=np.dtype(want["dtype"])).reshape(want["shape"], order="F")
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, got.shape, want["dtype"], want["shape"])
    assert np.array_equal(got, exp, equal_nan=got.dtype.kind == "f"), (got, exp)
    assert bool(got.flags.f_contiguous) == want["f_contiguous"], "memory order"


def assert_same(res, want, what):
    try:
        if "error" in want:
            assert isinstance(res, SparseArrayError), f"no error, want {want['text']!r}"
            assert (type(res).__name__, str(res)) == (want["error"], want["text"])
        elif "svt" in want:
            w = want["svt"]
            assert isinstance(res, SVT_SparseArray)
            assert (list(res.dim), res.type, res.na_background, res.dimnames) == \
                (w["dim"], w["type"], w["na_background"], w["dimnames"])
            for g, k in zip(res.to_csc(), ("col_ptr", "row_idx", "val")):
                same_nd(g, w[k])
        else:
            assert not isinstance(res, Exception), f"raised {res!r}"
            same_nd(res, want)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
