"""ctypes packing of the ``.Call``-level entry points onto a C ABI.

``CAbiDispatcher(lib, prefix)`` turns ``dispatcher("C_colStats_SVT", ...)``
into a call of ``<prefix>colStats_SVT`` in ``lib``.  The product instantiates
it once, for the HIP library (``libsvt_hip.so``, prefix ``svt_``;
include/svt_hip.h).  The packer is parameterised by (library, prefix) so that
the test-suite can drive its CPU checker -- which exposes the same host-level
signatures under another prefix -- with byte-identical arguments; nothing in
this package loads or names that checker.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np

from ._abi import PROTOTYPES
from .api import OPCODES, TIES_METHODS, SparseArrayError, SparseArrayUnsupported, naked_result
from .svt import INTSXP, LGLSXP, REALSXP, SVT_SparseArray, make_view, r_type_of, svt_view

_RT = {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}


def _F(a: np.ndarray) -> np.ndarray:
    return np.asfortranarray(a)


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


class CAbiDispatcher:
    def __init__(self, lib: ctypes.CDLL, prefix: str):
        self.lib = lib
        self.prefix = prefix
        self._declare()

    # -- prototypes ----------------------------------------------------------
    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def _declare(self):
        """Every row of the prototype table (svt_<name>) whose <prefix><name> the library has: the HIP library has them
        all, the checker the host-level subset."""
        for name, (res, args) in PROTOTYPES.items():
            mine = self.prefix + name[len("svt_"):]
            if name.startswith("svt_") and hasattr(self.lib, mine):
                f = getattr(self.lib, mine)
                f.restype, f.argtypes = res, args

    def _check(self, rc):
        if rc != 0:
            msg = self._fn("last_error")()
            raise (SparseArrayUnsupported if rc > 0 else SparseArrayError)(msg.decode() if msg else f"error {rc}")

    def _run(self, name, *args):
        """<prefix><name>(*args) with the status checked.  An SVT_SparseArray goes over as a pointer to its leaf table
        (which lives as long as the call), a numpy array as its address; anything else as it is."""
        args = [make_view(a) if isinstance(a, SVT_SparseArray) else a for a in args]
        self._check(self._fn(name)(*[byref(a) if isinstance(a, svt_view) else _ptr(a) if isinstance(a, np.ndarray) else a
                                     for a in args]))

    def _csc_result(self, x, new_dim, nnz, dimnames, fill):
        """The SVT_SparseArray of ``new_dim`` whose ``nnz`` nonzeros ``fill(col_ptr, row_idx, val)`` writes in the CSC
        layout (an array of no nonzeros is handed over as one unread element), its leaves rebuilt the way the glue
        rebuilds the R leaves; the type and the background are those of ``x``."""
        cp = np.zeros(int(np.prod(new_dim[1:], dtype=np.int64)) + 1, dtype=np.int64)
        ri = np.zeros(max(nnz, 1), dtype=np.int32)
        vv = np.zeros(max(nnz, 1), dtype=x.np_dtype)
        fill(cp, ri, vv)
        ans = SVT_SparseArray.from_csc(new_dim, x.type, cp, ri[:nnz], vv[:nnz], dimnames=dimnames)
        ans.na_background = x.na_background
        return ans

    # -- dispatcher ------------------------------------------------------------
    def __call__(self, name: str, *args):
        if not name.startswith("C_"):
            raise SparseArrayError(f"unknown entry point {name}")
        return getattr(self, name)(*args)

    # thread control (src/thread_control.c:47-66) -------------------------------
    def C_get_num_procs(self):
        return int(self._fn("get_num_procs")())

    def C_get_max_threads(self):
        return int(self._fn("get_max_threads")())

    def C_set_max_threads(self, nthread: int):
        """Returns the previous value (the reference returns it too, R/thread-control.R:60-66)."""
        return int(self._fn("set_max_threads")(int(nthread)))

    # crossprod / %*% / tcrossprod: a double matrix of ``shape``, column-major; the operands and flags in the C order, a
    # dense operand as (address, nrow, ncol, Rtype) --------------------------------------------------------------------
    def _product(self, name, shape, *args):
        out = np.zeros(shape, dtype=np.float64, order="F")
        flat = [b for a in args for b in ((a, a.shape[0], a.shape[1], _RT[r_type_of(a)]) if isinstance(a, np.ndarray)
                                          else (a,))]
        self._run(name, *flat, out)
        return out

    def C_crossprod2_SVT_mat(self, x: SVT_SparseArray, y: np.ndarray, tr_y: bool):
        y = _F(y)
        return self._product("crossprod2_SVT_mat", (x.dim[1], y.shape[0 if tr_y else 1]), x, y, int(tr_y))

    def C_crossprod2_mat_SVT(self, x: np.ndarray, y: SVT_SparseArray, tr_x: bool):
        x = _F(x)
        return self._product("crossprod2_mat_SVT", (x.shape[0 if tr_x else 1], y.dim[1]), x, y, int(tr_x))

    def C_crossprod2_SVT_SVT(self, x: SVT_SparseArray, y: SVT_SparseArray):
        return self._product("crossprod2_SVT_SVT", (x.dim[1], y.dim[1]), x, y)

    def C_crossprod1_SVT(self, x: SVT_SparseArray):
        return self._product("crossprod1_SVT", (x.dim[1], x.dim[1]), x)

    def C_matmul_SVT_mat(self, x: SVT_SparseArray, y: np.ndarray):
        y = _F(y)
        return self._product("matmul_SVT_mat", (x.dim[0], y.shape[1]), x, y)

    def C_matmul_SVT_SVT(self, x: SVT_SparseArray, y: SVT_SparseArray):
        return self._product("matmul_SVT_SVT", (x.dim[0], y.dim[1]), x, y)

    def C_tcrossprod1_SVT(self, x: SVT_SparseArray):
        return self._product("tcrossprod1_SVT", (x.dim[0], x.dim[0]), x)

    def C_tcrossprod2_SVT_SVT(self, x: SVT_SparseArray, y: SVT_SparseArray):
        return self._product("tcrossprod2_SVT_SVT", (x.dim[0], y.dim[0]), x, y)

    def C_matmul_SVT_SVT_sparse(self, x: SVT_SparseArray, y: SVT_SparseArray, tr_x: bool, tr_y: bool):
        """x %*% y, t(x) %*% y (``tr_x``) or x %*% t(y) (``tr_y``) with a sparse result (no counterpart in the reference;
        include/svt_hip.h, svt_matmul_SVT_SVT_sparse_begin; HIP library only): the begin / svt_Arith_SVT_end pair.
        Returns (SVT_SparseArray of type "double" without dimnames, not_finite)."""
        res, nnz, nf = c_void_p(0), ctypes.c_int64(0), c_int(0)
        self._run("matmul_SVT_SVT_sparse_begin", x, y, int(bool(tr_x)), int(bool(tr_y)), byref(res), byref(nnz), byref(nf))
        n = int(nnz.value)
        dim = (x.dim[1 if tr_x else 0], y.dim[0 if tr_y else 1])
        cp = np.zeros(dim[1] + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.float64)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        return SVT_SparseArray.from_csc(dim, "double", cp, ri[:n], vv[:n]), bool(nf.value)

    # colMedians (R/SparseArray-matrixStats.R:761-784) --------------------------------
    def C_colMedians_SVT(self, x: SVT_SparseArray, na_rm: bool):
        out = np.zeros(x.dim[1] if x.ndim == 2 else 0, dtype=np.float64)
        self._run("colMedians_SVT", x, int(bool(na_rm)), out)
        return out

    def C_rowMedians_SVT(self, x: SVT_SparseArray, na_rm: bool):
        out = np.zeros(x.dim[0] if x.ndim == 2 else 0, dtype=np.float64)
        self._run("rowMedians_SVT", x, int(bool(na_rm)), out)
        return out

    # colQuantiles / rowQuantiles, type 7 (include/svt_hip.h; HIP library only) ----
    def _quantiles(self, fname, x, probs, na_rm, nout):
        probs = np.ascontiguousarray(probs, dtype=np.float64)
        out = np.zeros((nout, probs.size), dtype=np.float64, order="F")
        self._run(fname, x, probs, int(probs.size), int(bool(na_rm)), out)
        return out

    def C_colQuantiles_SVT(self, x: SVT_SparseArray, probs, na_rm: bool):
        return self._quantiles("colQuantiles_SVT", x, probs, na_rm, x.dim[1] if x.ndim == 2 else 0)

    def C_rowQuantiles_SVT(self, x: SVT_SparseArray, probs, na_rm: bool):
        return self._quantiles("rowQuantiles_SVT", x, probs, na_rm, x.dim[0] if x.ndim == 2 else 0)

    # colMads / rowMads (include/svt_hip.h; HIP library only) ----------------------
    def _mads(self, fname, x, center, constant, na_rm, axis):
        nout = x.dim[axis] if x.ndim == 2 else 0
        if center is not None:
            center = np.ascontiguousarray(center, dtype=np.float64)
            if x.ndim == 2 and (center.ndim != 1 or center.size != nout):       # (the library sees a pointer only)
                raise SparseArrayError("'center' must be NULL, a single number, or a vector with one element per "
                                       + ("column" if axis == 1 else "row"))
        out = np.zeros(nout, dtype=np.float64)
        self._run(fname, x, center, float(constant), int(bool(na_rm)), out)
        return out

    def C_colMads_SVT(self, x: SVT_SparseArray, center, constant: float, na_rm: bool):
        return self._mads("colMads_SVT", x, center, constant, na_rm, 1)

    def C_rowMads_SVT(self, x: SVT_SparseArray, center, constant: float, na_rm: bool):
        return self._mads("rowMads_SVT", x, center, constant, na_rm, 0)

    # colRanks / rowRanks (include/svt_hip.h; HIP library only) ---------------------
    @staticmethod
    def _ranks_out(x, ties, transposed):
        """(SVT_TIES_* code, result array): ``ties`` a name or a code; an unknown one is left to the library."""
        code = TIES_METHODS.get(ties, -1) if isinstance(ties, str) else int(ties)
        nrow, ncol = (x.dim[0], x.dim[1]) if x.ndim == 2 else (0, 0)
        shape = (ncol, nrow) if transposed else (nrow, ncol)
        return code, np.zeros(shape, dtype=np.float64 if code == TIES_METHODS["average"] else np.int32, order="F")

    def C_colRanks_SVT(self, x: SVT_SparseArray, ties, preserve_shape: bool):
        code, out = self._ranks_out(x, ties, not preserve_shape)
        self._run("colRanks_SVT", x, code, int(bool(preserve_shape)), out)
        return out

    def C_rowRanks_SVT(self, x: SVT_SparseArray, ties):
        code, out = self._ranks_out(x, ties, False)
        self._run("rowRanks_SVT", x, code, out)
        return out

    # resident operands (include/svt_hip.h; HIP library only) --------------------
    def resident_set_limit(self, nbytes: int):
        self._run("resident_set_limit", int(nbytes))

    def resident_clear(self):
        self._fn("resident_clear")()

    def resident_stats(self) -> dict:
        b, e, h, m = ctypes.c_size_t(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._fn("resident_stats")(byref(b), byref(e), byref(h), byref(m))
        return {"bytes": b.value, "entries": e.value, "hits": h.value, "misses": m.value}

    @property
    def accepts_mixed_types(self) -> bool:
        """The HIP library widens an integer operand of a mixed integer/double product on the
        device (include/svt_hip.h); the oracle keeps the reference's "same type" rule."""
        return self.prefix == "svt_"

    def has_entry(self, name: str) -> bool:
        return hasattr(self.lib, self.prefix + name[2:])

    # stats -------------------------------------------------------------------
    def _opcode(self, op: str) -> int:
        if op not in OPCODES:
            raise SparseArrayError(
                "'op' must be one of: " + ", ".join(f'"{k}"' for k in OPCODES))
        return OPCODES[op]

    def C_summarize_SVT(self, x, op, na_rm, center):
        oc = self._opcode(op)
        out_d = np.zeros(2, np.float64)
        out_i = np.zeros(2, np.int32)
        out_Rtype, warn = c_int(0), c_int(0)
        self._run("summarize_SVT", x, oc, int(na_rm), float(center), out_d, out_i, byref(out_Rtype), byref(warn))
        return naked_result(op, x.type, out_d, out_i), bool(warn.value)

    def _stat_out(self, op, x, shape, per_cell=1):
        oc = self._opcode(op)
        rt = self._fn("colStats_out_Rtype")(oc, x.Rtype)
        if rt < 0:
            self._check(rt)
        dtype = np.float64 if rt == REALSXP else np.int32
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        flat = np.zeros(max(n * per_cell, 1), dtype=dtype)
        return oc, flat, n

    def C_colStats_SVT(self, x, op, na_rm, center, dims):
        shape = tuple(x.dim[dims:])
        oc, flat, n = self._stat_out(op, x, shape)
        warn = c_int(0)
        self._run("colStats_SVT", x, oc, int(na_rm), float(center), int(dims), flat, byref(warn))
        flat = flat[:n]
        ans = flat.reshape(shape, order="F") if len(shape) > 1 else flat
        return ans, bool(warn.value)

    def C_rowStats_SVT(self, x, op, na_rm, center, dims):
        return self._row_stats("rowStats_SVT", x, op, na_rm, center, dims)

    def C_rowStatsFull_SVT(self, x, op, na_rm, center, dims):
        """svt_rowStatsFull_SVT.  Returns the flat buffer (column-major prod(dim[:dims]) elements; "range": the
        minima, then as many maxima) and the warning flag: the caller shapes it."""
        return self._row_stats("rowStatsFull_SVT", x, op, na_rm, center, dims, flat_result=True)

    def _row_stats(self, fname, x, op, na_rm, center, dims, flat_result=False):
        shape = tuple(x.dim[:dims])
        per_cell = 2 if op == "range" else 1
        oc, flat, n = self._stat_out(op, x, shape, per_cell)
        nout = per_cell * n
        warn = c_int(0)
        if center is not None:
            center = np.ascontiguousarray(
                np.reshape(np.asarray(center, np.float64), -1, order="F"))
            if center.size != n:
                raise SparseArrayError("unexpected 'center' length")
        self._run(fname, x, oc, int(na_rm), center, int(dims), flat, byref(warn))
        if flat_result:
            return flat[:nout], bool(warn.value)
        flat = flat[:n]
        ans = flat.reshape(shape, order="F") if len(shape) > 1 else flat
        return ans, bool(warn.value)

    # rowsum / colsum -----------------------------------------------------------
    def _xsum(self, fname, x, group, ngroup, na_rm, shape):
        dtype = np.float64 if x.type == "double" else np.int32
        out = np.zeros(shape, dtype=dtype, order="F")
        group = np.ascontiguousarray(group, dtype=np.int32)
        ov = c_int(0)
        self._run(fname, x, group, int(ngroup), int(na_rm), out, byref(ov))
        return out, bool(ov.value)

    def C_rowsum_SVT(self, x, group, ngroup, na_rm):
        if x.ndim != 2:
            raise SparseArrayError("input object must have 2 dimensions")
        return self._xsum("rowsum_SVT", x, group, ngroup, na_rm,
                          (ngroup, x.dim[1]))

    def C_colsum_SVT(self, x, group, ngroup, na_rm):
        if x.ndim != 2:
            raise SparseArrayError("input object must have 2 dimensions")
        return self._xsum("colsum_SVT", x, group, ngroup, na_rm,
                          (x.dim[0], ngroup))

    def _dgc(self, fname, x, group, ngroup, na_rm, shape):
        (nrow, ncol), p, i, xx = x
        p = np.ascontiguousarray(p, np.int32)
        i = np.ascontiguousarray(i, np.int32)
        xx = np.ascontiguousarray(xx, np.float64)
        group = np.ascontiguousarray(group, dtype=np.int32)
        out = np.zeros(shape, dtype=np.float64, order="F")
        self._run(fname, int(nrow), int(ncol), xx, i, p, group, int(ngroup), int(na_rm), out)
        return out

    # aperm (src/SparseArray_aperm.c:935-970) ------------------------------------
    def C_aperm_SVT(self, x: SVT_SparseArray, perm):
        """Returns the permuted array as an SVT_SparseArray."""
        perm = np.asarray(perm, dtype=np.int32)
        if perm.size != x.ndim:
            raise SparseArrayError("'perm' must have one element per dimension")
        if sorted(perm.tolist()) != list(range(1, x.ndim + 1)):
            raise SparseArrayError(f"'perm' must be a permutation of 1:{x.ndim}")
        dn = None if x.dimnames is None else [x.dimnames[p - 1] for p in perm]
        return self._csc_result(x, tuple(x.dim[p - 1] for p in perm), x.nzcount(), dn,
                                lambda cp, ri, vv: self._run("aperm_SVT", x, perm, cp, ri, vv))

    # column statistics of a dgCMatrix (src/sparseMatrix_utils.c:105-223) ---------------
    def _dgc_colstat(self, fname, x, na_rm, ncols_out):
        (nrow, ncol), p, _i, xx = x
        p = np.ascontiguousarray(p, np.int32)
        xx = np.ascontiguousarray(xx, np.float64)
        out = np.zeros((ncol, ncols_out) if ncols_out > 1 else ncol, dtype=np.float64, order="F")
        self._run(fname, int(nrow), int(ncol), xx, p, int(bool(na_rm)), out)
        return out

    def C_colMins_dgCMatrix(self, x, na_rm):
        return self._dgc_colstat("colMins_dgCMatrix", x, na_rm, 1)

    def C_colMaxs_dgCMatrix(self, x, na_rm):
        return self._dgc_colstat("colMaxs_dgCMatrix", x, na_rm, 1)

    def C_colRanges_dgCMatrix(self, x, na_rm):
        return self._dgc_colstat("colRanges_dgCMatrix", x, na_rm, 2)

    def C_colVars_dgCMatrix(self, x, na_rm):
        return self._dgc_colstat("colVars_dgCMatrix", x, na_rm, 1)

    # t() (src/SparseArray_aperm.c:395-423) ----------------------------------------------
    def C_transpose_2D_SVT(self, x: SVT_SparseArray):
        """Returns t(x) as an SVT_SparseArray (the glue rebuilds the R leaves the same way)."""
        if x.ndim != 2:
            raise SparseArrayError("object to transpose must have exactly 2 dimensions")
        dn = None if x.dimnames is None else [x.dimnames[1], x.dimnames[0]]
        return self._csc_result(x, (x.dim[1], x.dim[0]), x.nzcount(), dn,
                                lambda cp, ri, vv: self._run("transpose_2D_SVT", x, cp, ri, vv))

    # x[i, j] by an N-index (src/SparseArray_subsetting.c:223-297; include/svt_hip.h; HIP library only) -------------
    def C_subset_SVT_by_Nindex(self, x: SVT_SparseArray, *index):
        """``index``: one subscript per dimension, 1-based int32 arrays, or None for the whole axis.  Returns x[i, j] as
        an SVT_SparseArray, its leaves rebuilt from the CSC layout the way t() does.  The library takes 2-D operands;
        for any other it sees the first two subscripts and answers "not supported here"."""
        if len(index) != x.ndim:
            raise SparseArrayError("incorrect number of subscripts")
        sub = [None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (index + (None,))[:2]]
        # (a pointer tells "no subscript" from an empty one: an empty array is handed over as one unread element)
        buf = [None if v is None else (v if v.size else np.zeros(1, np.int32)) for v in sub]
        res, nnz = c_void_p(0), ctypes.c_int64(0)
        self._run("subset_SVT_begin", x, *[a for v, b in zip(sub, buf) for a in ((None, 0) if v is None else (b, v.size))],
                  byref(res), byref(nnz))
        new_dim = tuple(d if v is None else int(v.size) for d, v in zip(x.dim, sub))
        dn = None
        if x.dimnames is not None:
            dn = [names if v is None or names is None else [names[k - 1] for k in v.tolist()]
                  for names, v in zip(x.dimnames, sub)]
        return self._csc_result(x, new_dim, int(nnz.value), dn,
                                lambda cp, ri, vv: self._run("subset_SVT_end", res, cp, ri, vv))

    # Arith / unary minus / Math (src/SparseArray_Arith_methods.c, src/SparseArray_Math_methods.c; include/svt_hip.h; HIP
    # library only): begin leaves the result on the device and says its type and size, end copies it out --------------
    def _arith(self, begin, x, args, dimnames, with_ovflow=True):
        """The SVT_SparseArray of x's dim that ``svt_<begin>(x, *args, &res, &Rtype, &nnz[, &ovflow])`` computes, and
        the overflow flag."""
        res, rt, nnz, ov = c_void_p(0), c_int(0), ctypes.c_int64(0), c_int(0)
        self._run(begin, x, *args, byref(res), byref(rt), byref(nnz), *([byref(ov)] if with_ovflow else []))
        n = int(nnz.value)
        type_ = "double" if rt.value == REALSXP else "integer"
        cp = np.zeros(int(np.prod(x.dim[1:], dtype=np.int64)) + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.float64 if type_ == "double" else np.int32)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        return SVT_SparseArray.from_csc(tuple(x.dim), type_, cp, ri[:n], vv[:n], dimnames=dimnames), bool(ov.value)

    def C_Arith_SVT1_SVT2(self, x: SVT_SparseArray, y: SVT_SparseArray, op: str):
        """Returns (x op y, overflow flag); the dimnames are the first non-NULL ones."""
        from .api import ARITH_OPCODES
        return self._arith("Arith_SVT_SVT_begin", x, (y, ARITH_OPCODES[op]), x.dimnames if x.dimnames is not None else y.dimnames)

    def C_Arith_SVT1_v2(self, x: SVT_SparseArray, y: float, y_type: str, op: str):
        """Returns (x op y, overflow flag) for the scalar ``y`` of R type ``y_type`` ("integer" / "double")."""
        from .api import ARITH_OPCODES
        return self._arith("Arith_SVT_scalar_begin", x, (ARITH_OPCODES[op], float(y), _RT[y_type]), x.dimnames)

    def C_unary_minus_SVT(self, x: SVT_SparseArray):
        return self._arith("unary_minus_SVT_begin", x, (), x.dimnames, with_ovflow=False)[0]

    def C_Math_SVT(self, x: SVT_SparseArray, op: str, digits: float):
        from .api import MATH_OPCODES
        return self._arith("Math_SVT_begin", x, (MATH_OPCODES.get(op, 0), float(digits)), x.dimnames, with_ovflow=False)[0]

    # Compare / Logic (src/SparseArray_Compare_methods.c, src/SparseArray_Logic_methods.c; include/svt_hip.h; HIP library
    # only): the same begin / end pair, the result "logical" with explicit values (1 or NA) ---------------------------
    def _logical_result(self, begin, x, args, dimnames):
        res, nnz = c_void_p(0), ctypes.c_int64(0)
        self._run(begin, x, *args, byref(res), byref(nnz))
        n = int(nnz.value)
        cp = np.zeros(int(np.prod(x.dim[1:], dtype=np.int64)) + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.int32)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        return SVT_SparseArray.from_csc(tuple(x.dim), "logical", cp, ri[:n], vv[:n], dimnames=dimnames)

    def C_Compare_SVT1_v2(self, x: SVT_SparseArray, y: float, y_type: str, op: str):
        """x op y for the scalar ``y`` of R type ``y_type`` ("logical" / "integer" / "double"; an integer or logical
        NA goes over as INT_MIN, like every integer scalar as its double value)."""
        from .api import COMPARE_OPCODES
        return self._logical_result("Compare_SVT_scalar_begin", x, (COMPARE_OPCODES[op], float(y), _RT[y_type]), x.dimnames)

    def C_Compare_SVT1_SVT2(self, x: SVT_SparseArray, y: SVT_SparseArray, op: str):
        """x op y, op one of != < >; the dimnames are the first non-NULL ones."""
        from .api import COMPARE_OPCODES
        return self._logical_result("Compare_SVT_SVT_begin", x, (y, COMPARE_OPCODES[op]),
                                    x.dimnames if x.dimnames is not None else y.dimnames)

    def C_Logic_SVT1_SVT2(self, x: SVT_SparseArray, y: SVT_SparseArray, op: str):
        from .api import LOGIC_OPCODES
        return self._logical_result("Logic_SVT_SVT_begin", x, (y, LOGIC_OPCODES[op]),
                                    x.dimnames if x.dimnames is not None else y.dimnames)

    # pmin / pmax and is.na / is.nan / is.infinite (.pminmax2 and C_SVT_apply_isFUN of the reference; include/svt_hip.h;
    # HIP library only): the same begin / end pair; the library says the type of a pmin / pmax result ---------------
    def C_pminmax_SVT1_SVT2(self, x: SVT_SparseArray, y: SVT_SparseArray, op: str, na_rm: bool):
        """pmin(x, y) / pmax(x, y) (``op`` "pmin" / "pmax"); the dimnames are the first non-NULL ones."""
        from .api import PMINMAX_NA_RM, PMINMAX_OPCODES
        ans = self._assigned("pminmax_SVT_SVT_begin", x, (y, PMINMAX_OPCODES[op] | (PMINMAX_NA_RM if na_rm else 0)))
        ans.dimnames = x.dimnames if x.dimnames is not None else y.dimnames
        return ans

    def C_pminmax_SVT1_v2(self, x: SVT_SparseArray, y: float, y_type: str, op: str, na_rm: bool):
        """pmin(x, y) / pmax(x, y) for the scalar ``y`` of R type ``y_type`` ("logical" / "integer" / "double")."""
        from .api import PMINMAX_NA_RM, PMINMAX_OPCODES
        return self._assigned("pminmax_SVT_scalar_begin", x,
                              (PMINMAX_OPCODES[op] | (PMINMAX_NA_RM if na_rm else 0), float(y), _RT[y_type]))

    def C_SVT_apply_isFUN(self, x: SVT_SparseArray, isFUN: str):
        """``isFUN``: "is.na", "is.nan" or "is.infinite"; returns the "logical" SVT_SparseArray."""
        from .api import ISFUN_OPCODES
        if isFUN not in ISFUN_OPCODES:
            raise SparseArrayError(f"unknown isFUN \"{isFUN}\"")
        return self._logical_result("isFUN_SVT_begin", x, (ISFUN_OPCODES[isFUN],), x.dimnames)

    # sweep(x, MARGIN, STATS, FUN) (no counterpart in the reference; include/svt_hip.h, svt_Arith_SVT_vector_begin /
    # svt_Compare_SVT_vector_begin; HIP library only): the same begin / end pairs with a host vector and the margin ------
    def C_sweep_SVT(self, x: SVT_SparseArray, stats: np.ndarray, stats_type: str, margin, op: str, na_rm: bool = False):
        """Returns (x op STATS along ``margin``, overflow flag).  ``stats``: a float64 array for ``stats_type`` "double",
        an int32 one for "integer" / "logical"; ``margin``: 1-based dimension numbers; ``na_rm``: read by "pmin" / "pmax".
        An element the library refuses is named in its message, 0-based."""
        from .api import ARITH_OPCODES, COMPARE_OPCODES, PMINMAX_NA_RM, PMINMAX_OPCODES
        stats = np.ascontiguousarray(stats, dtype=np.float64 if stats_type == "double" else np.int32).reshape(-1)
        buf = stats if stats.size else np.zeros(1, stats.dtype)     # (an empty vector is handed over as one unread element)
        m = np.ascontiguousarray(margin, dtype=np.int32).reshape(-1)
        bad = ctypes.c_int64(-1)
        if op in PMINMAX_OPCODES:
            args = (PMINMAX_OPCODES[op] | (PMINMAX_NA_RM if na_rm else 0), buf, stats.size, _RT[stats_type], m, m.size, byref(bad))
            return self._assigned("pminmax_SVT_vector_begin", x, args), False
        if op in COMPARE_OPCODES:
            args = (COMPARE_OPCODES[op], buf, stats.size, _RT[stats_type], m, m.size, byref(bad))
            return self._logical_result("Compare_SVT_vector_begin", x, args, x.dimnames), False
        args = (ARITH_OPCODES[op], buf, stats.size, _RT[stats_type], m, m.size, byref(bad))
        return self._arith("Arith_SVT_vector_begin", x, args, x.dimnames)

    # abind / cbind / rbind (src/SparseArray_abind.c; include/svt_hip.h; HIP library only): begin leaves the result on the
    # device, Arith_SVT_end copies it out ---------------------------------------------------------------------------
    def C_abind_SVT_SparseArray_objects(self, objects, along: int, ans_type: str):
        """The SVT_SparseArray (dim, type ``ans_type``, leaves; no dimnames) of ``objects`` bound along dimension
        ``along`` (1-based).  The objects go over with their own types, the library widens on the device; NaArray
        objects give an NaArray."""
        objects = list(objects)
        if not objects:
            raise SparseArrayError("'objects' cannot be an empty list")
        if ans_type not in _RT:
            raise SparseArrayError("invalid requested type")
        views = [make_view(x) for x in objects]
        table = (ctypes.POINTER(svt_view) * len(views))(*[ctypes.pointer(v) for v in views])
        res, nnz = c_void_p(0), ctypes.c_int64(0)
        self._run("abind_SVT_begin", table, len(views), int(along), _RT[ans_type], byref(res), byref(nnz))
        n, x = int(nnz.value), objects[0]
        new_dim = tuple(sum(o.dim[k] for o in objects) if k == along - 1 else d for k, d in enumerate(x.dim))
        cp = np.zeros(int(np.prod(new_dim[1:], dtype=np.int64)) + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.float64 if ans_type == "double" else np.int32)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        ans = SVT_SparseArray.from_csc(new_dim, ans_type, cp, ri[:n], vv[:n])
        ans.na_background = x.na_background
        return ans

    # x[i, j, ...] <- value by an N-index (src/SparseArray_subassignment.c:1005-1230; include/svt_hip.h; HIP library only):
    # begin leaves the result on the device, Arith_SVT_end copies it out ------------------------------------------------
    def _subassign(self, begin, x, Nindex, args):
        """``Nindex``: one subscript per dimension, 1-based int32 arrays, or None for the whole axis.  Returns the
        SVT_SparseArray of x's dim and dimnames that ``svt_<begin>(x, index, index_len, *args, &res, &Rtype, &nnz)``
        computes; its type is what the library says (the wider of x's and the value's)."""
        if len(Nindex) != x.ndim:
            raise SparseArrayError("incorrect number of subscripts")
        sub = [None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in Nindex]
        # (a pointer tells "no subscript" from an empty one: an empty array is handed over as one unread element)
        buf = [None if v is None else (v if v.size else np.zeros(1, np.int32)) for v in sub]
        index = (c_void_p * x.ndim)(*[None if b is None else b.ctypes.data for b in buf])
        index_len = np.array([-1 if v is None else v.size for v in sub], dtype=np.int64)
        return self._assigned(begin, x, (index, index_len) + tuple(args))

    def _assigned(self, begin, x, args):
        """The SVT_SparseArray of x's dim and dimnames that ``svt_<begin>(x, *args, &res, &Rtype, &nnz)`` leaves on the
        device, copied out by Arith_SVT_end."""
        res, rt, nnz = c_void_p(0), c_int(0), ctypes.c_int64(0)
        self._run(begin, x, *args, byref(res), byref(rt), byref(nnz))
        n = int(nnz.value)
        type_ = {LGLSXP: "logical", INTSXP: "integer", REALSXP: "double"}[rt.value]
        cp = np.zeros(int(np.prod(x.dim[1:], dtype=np.int64)) + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.float64 if type_ == "double" else np.int32)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        return SVT_SparseArray.from_csc(tuple(x.dim), type_, cp, ri[:n], vv[:n], dimnames=x.dimnames)

    def C_subassign_SVT_with_short_Rvector(self, x: SVT_SparseArray, Nindex, value: np.ndarray):
        """``value``: a non-empty 1-D array, bool (logical), int32 (integer) or float64 (double), recycled over the row
        subscript; NA_integer_ and NA_real_ travel as they are."""
        value = np.ascontiguousarray(value).reshape(-1)
        if value.dtype == np.bool_:
            value, v_type = value.astype(np.int32), "logical"
        else:
            v_type = r_type_of(value)
        if v_type not in _RT:
            raise SparseArrayError("the supplied value must be of type \"logical\", \"integer\" or \"double\"")
        if value.size == 0:
            raise SparseArrayError("replacement has length zero")
        return self._subassign("subassign_SVT_vector_begin", x, Nindex, (value, int(value.size), _RT[v_type]))

    def C_subassign_SVT_with_SVT(self, x: SVT_SparseArray, Nindex, v: SVT_SparseArray):
        """``v``: an SVT_SparseArray with the dims of the selection; rows strictly increasing, leaves without repeats
        (anything else in range: SparseArrayUnsupported)."""
        return self._subassign("subassign_SVT_SVT_begin", x, Nindex, (v,))

    # x[Lindex], x[Mindex] and their subassignments (src/SparseArray_subsetting.c, C_subset_SVT_by_Lindex / _by_Mindex;
    # src/SparseArray_subassignment.c, C_subassign_SVT_by_Lindex / _by_Mindex; include/svt_hip.h; HIP library only) -----
    @staticmethod
    def _index_buffer(index, dtype):
        """(the contiguous index, the buffer handed over: an empty index goes over as one unread element)"""
        index = np.ascontiguousarray(index, dtype=dtype)
        return index, (index if index.size else np.zeros(1, dtype))

    def C_subset_SVT_by_Lindex(self, x: SVT_SparseArray, Lindex: np.ndarray):
        """``Lindex``: 1-based int64, INT64_MIN for NA.  Returns the vector of x's type, one value per index."""
        L, buf = self._index_buffer(np.reshape(Lindex, -1), np.int64)
        out = np.zeros(max(L.size, 1), dtype=x.np_dtype)
        self._run("subset_SVT_by_Lindex", x, buf, int(L.size), out)
        return out[:L.size]

    def C_subset_SVT_by_Mindex(self, x: SVT_SparseArray, Mindex: np.ndarray):
        """``Mindex``: a K x ndim int32 matrix, 1-based, NA_integer_ for NA."""
        M = np.asarray(Mindex, dtype=np.int32)
        K = int(M.shape[0])
        _, buf = self._index_buffer(M.reshape(-1, order="F"), np.int32)
        out = np.zeros(max(K, 1), dtype=x.np_dtype)
        self._run("subset_SVT_by_Mindex", x, buf, K, out)
        return out[:K]

    @staticmethod
    def _assigned_value(value):
        value = np.ascontiguousarray(value).reshape(-1)
        if value.dtype == np.bool_:
            value, v_type = value.astype(np.int32), "logical"
        else:
            v_type = r_type_of(value)
        if v_type not in _RT:
            raise SparseArrayError("the supplied value must be of type \"logical\", \"integer\" or \"double\"")
        return value, int(value.size), _RT[v_type]

    def C_subassign_SVT_by_Lindex(self, x: SVT_SparseArray, Lindex: np.ndarray, value: np.ndarray):
        """``value``: a non-empty 1-D array, bool (logical), int32 (integer) or float64 (double), recycled over the
        index."""
        L, buf = self._index_buffer(np.reshape(Lindex, -1), np.int64)
        return self._assigned("subassign_SVT_by_Lindex_begin", x, (buf, int(L.size)) + self._assigned_value(value))

    def C_subassign_SVT_by_Mindex(self, x: SVT_SparseArray, Mindex: np.ndarray, value: np.ndarray):
        M = np.asarray(Mindex, dtype=np.int32)
        _, buf = self._index_buffer(M.reshape(-1, order="F"), np.int32)
        return self._assigned("subassign_SVT_by_Mindex_begin", x, (buf, int(M.shape[0])) + self._assigned_value(value))

    # poissonSparseArray() / simple_rpois() (src/randomSparseArray.c; include/svt_hip.h; HIP library only): begin leaves
    # the array on the device, Arith_SVT_end copies it out; ``seed`` in [0, 2^64) goes over as the int64 of its bits ----
    @staticmethod
    def _seed_bits(seed: int) -> int:
        return seed - 2 ** 64 if seed >= 2 ** 63 else seed

    def C_poissonSparseArray(self, dim, lambda_: float, seed: int):
        """The "integer" SVT_SparseArray of ``dim`` (a tuple of ints), no dimnames."""
        nleaves = int(np.prod(dim[1:], dtype=object)) if len(dim) > 1 else 1
        res, nnz = c_void_p(0), ctypes.c_int64(0)
        if nleaves >= 2 ** 63:
            raise SparseArrayError("the array has more than 2^63 - 1 leaves")
        self._run("poissonSparseArray_begin", int(dim[0]), nleaves, float(lambda_), self._seed_bits(seed), byref(res), byref(nnz))
        n = int(nnz.value)
        cp = np.zeros(nleaves + 1, dtype=np.int64)
        ri = np.zeros(max(n, 1), dtype=np.int32)
        vv = np.zeros(max(n, 1), dtype=np.int32)
        self._run("Arith_SVT_end", res, cp, ri, vv)
        return SVT_SparseArray.from_csc(tuple(dim), "integer", cp, ri[:n], vv[:n])

    def C_simple_rpois(self, n: int, lambda_: float, seed: int):
        out = np.zeros(max(int(n), 1), dtype=np.int32)
        self._run("simple_rpois", int(n), float(lambda_), self._seed_bits(seed), out)
        return out[:int(n)]

    def C_rowsum_dgCMatrix(self, x, group, ngroup, na_rm):
        """``x`` = ((nrow, ncol), p, i, x) -- the dgCMatrix slots."""
        return self._dgc("rowsum_dgCMatrix", x, group, ngroup, na_rm,
                         (ngroup, x[0][1]))

    def C_colsum_dgCMatrix(self, x, group, ngroup, na_rm):
        return self._dgc("colsum_dgCMatrix", x, group, ngroup, na_rm,
                         (x[0][0], ngroup))
