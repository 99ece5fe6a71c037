"""Device-resident operands (HBM) and the device-level entry points.

torch is used here as plumbing only: it owns the device allocations and the
HIP stream the kernels are launched on.  Every computation is a call into
libsvt_hip.so (include/svt_hip.h, "device level").
"""
from __future__ import annotations

import ctypes
from ctypes import c_int64, c_void_p

import numpy as np
import torch

from . import _hip
from ._abi import ALLOC_FN, FREE_FN
from .api import OPCODES, SparseArrayError, SparseArrayUnsupported, normarg_dim, poisson_lambda, seed_word
from .svt import INTSXP, LGLSXP, REALSXP


def _lib():
    return _hip.init()


def _check(rc):
    if rc != 0:
        raise (SparseArrayUnsupported if rc > 0 else SparseArrayError)(_lib().svt_last_error().decode())


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class DeviceCSC:
    """An SVT in its device layout: col_ptr int64[ncol+1], row_idx int32[nnz],
    val f64|i32[nnz] (struct svt_dev_csc).  ``ncol`` counts leaves."""

    def __init__(self, nrow: int, col_ptr: torch.Tensor, row_idx: torch.Tensor,
                 val: torch.Tensor, logical: bool = False):
        assert col_ptr.dtype == torch.int64 and row_idx.dtype == torch.int32
        assert val.dtype in (torch.float64, torch.int32)
        assert col_ptr.is_cuda and row_idx.is_cuda and val.is_cuda
        self.nrow = int(nrow)
        self.ncol = int(col_ptr.numel() - 1)
        self.nnz = int(row_idx.numel())
        self.col_ptr, self.row_idx, self.val = col_ptr.contiguous(), row_idx.contiguous(), val.contiguous()
        self.Rtype = REALSXP if val.dtype == torch.float64 else (LGLSXP if logical else INTSXP)
        self._h = _lib().svt_wrap_device_csc(self.Rtype, self.nrow, self.ncol, self.nnz,
                                             self.col_ptr.data_ptr(), self.row_idx.data_ptr(),
                                             self.val.data_ptr())

    @classmethod
    def from_host(cls, nrow, col_ptr, row_idx, val, device="cuda"):
        return cls(nrow, torch.as_tensor(np.asarray(col_ptr, np.int64), device=device),
                   torch.as_tensor(np.asarray(row_idx, np.int32), device=device),
                   torch.as_tensor(np.asarray(val), device=device))

    @classmethod
    def from_dense(cls, a: torch.Tensor, ans_type=None, na_background=False, logical=False) -> "DeviceCSC":
        """The operand of a dense array that is on the device already (include/svt_hip.h, svt_dev_from_dense): ``a`` a
        CUDA tensor of dtype float64 or int32 (integer; logical with ``logical=True``) or bool (logical, through
        ``.to(torch.int32)``) with at least one dimension; the result has nrow = a.shape[0] and ncol = prod(a.shape[1:]).
        A cell is stored when it is != 0, or, under ``na_background``, when it is not NA.  ``ans_type``: "logical",
        "integer" or "double", the array's type (the default) or a wider one; a narrower one raises
        SparseArrayUnsupported.  The memory layout decides the route and torch computes nothing: a column-major tensor
        (``a.permute(*reversed(range(a.ndim))).is_contiguous()``, every 1-D tensor) is read in place; a C-contiguous one
        is sparsified as the array of the reversed shape that it is in memory, then transposed by ``t()`` (2-D) or
        ``aperm`` with the reversing permutation; any other layout raises SparseArrayError.  Every array is a torch
        allocation on the current stream."""
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise SparseArrayError("from_dense() takes a CUDA tensor")
        if a.dtype == torch.bool:
            a, logical = a.to(torch.int32), True
        if a.dtype not in (torch.int32, torch.float64):
            raise SparseArrayError("the array must be logical (bool), integer (int32) or double (float64)")
        if a.ndim < 1:
            raise SparseArrayError("the array needs at least one dimension")
        x_Rtype = REALSXP if a.dtype == torch.float64 else LGLSXP if logical else INTSXP
        ans_Rtype = x_Rtype if ans_type is None else _rtype_of(ans_type)
        shape, nd = tuple(int(d) for d in a.shape), a.ndim
        if a.permute(*reversed(range(nd))).is_contiguous():
            return cls._sparsify(a, shape, x_Rtype, ans_Rtype, na_background)
        if not a.is_contiguous():
            raise SparseArrayError("the array must be column-major or C-contiguous")
        R = cls._sparsify(a, shape[::-1], x_Rtype, ans_Rtype, na_background)
        return R.t() if nd == 2 else R.aperm(shape[::-1], list(range(nd, 0, -1)))[0]

    @classmethod
    def _sparsify(cls, a, dim, x_Rtype, ans_Rtype, na_background):
        """svt_dev_from_dense on the memory of ``a`` read as the column-major array of extents ``dim``"""
        nrow, nleaves = dim[0], int(np.prod(dim[1:], dtype=np.int64))
        return _composed(lambda *r: _lib().svt_dev_from_dense(a.data_ptr(), x_Rtype, nrow, nleaves, ans_Rtype,
                                                              int(bool(na_background)), *r),
                         a.device, nrow, nleaves, ans_Rtype)

    def _dim(self, dim):
        dim = (self.nrow, self.ncol) if dim is None else tuple(int(d) for d in dim)
        if not dim or dim[0] != self.nrow or int(np.prod(dim[1:], dtype=np.int64)) != self.ncol:
            raise SparseArrayError("'dim' does not match the operand's rows and leaves")
        return dim

    def to_dense(self, dim=None, out_type=None, na_background=False, out=None) -> torch.Tensor:
        """The dense array of the operand, on the device (include/svt_hip.h, svt_dev_to_dense): a tensor of shape
        ``dim`` (default (nrow, ncol)) that is a zero-copy view of the column-major buffer the kernel writes -- every
        cell of it: zero, or NA under ``na_background``, where nothing is stored.  ``out_type``: the operand's type (the
        default) or a wider one.  ``out``: the caller's flat contiguous buffer of nrow * ncol elements.  The result's
        ``bad`` attribute is a device int32 word, nonzero once the kernel has run over an operand whose pointers or rows
        it refused to follow; it is left on the device so that the call stays asynchronous."""
        dim = self._dim(dim)
        out_Rtype = self.Rtype if out_type is None else _rtype_of(out_type)
        dtype = torch.float64 if out_Rtype == REALSXP else torch.int32
        n, dev = self.nrow * self.ncol, self.val.device
        if out is None:
            out = torch.empty(n, dtype=dtype, device=dev)
        if not (isinstance(out, torch.Tensor) and out.dtype == dtype and out.is_cuda and out.ndim == 1 and out.is_contiguous()
                and out.numel() == n):
            raise SparseArrayError(f"'out' must be a flat contiguous CUDA tensor of {n} elements of {dtype}")
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _check(_lib().svt_dev_to_dense(self.handle, int(bool(na_background)), out_Rtype, out.data_ptr(), bad.data_ptr(),
                                       _stream()))
        res = out.view(*reversed(dim)).permute(*reversed(range(len(dim))))
        res.bad = bad
        return res

    def nzwhich(self, dim=None, arr_ind=False) -> torch.Tensor:
        """nzwhich(x, arr.ind=) on the device (include/svt_hip.h, svt_dev_nzwhich), 0-based: an int64 tensor of nnz
        linear indices into the column-major array of extents ``dim`` (default (nrow, ncol)), in storage order, or
        (``arr_ind``) an int32 tensor of shape (nnz, ndim) of coordinates, a view of the column-major buffer.  With
        ``val`` it is the COO form of the operand."""
        dim = self._dim(dim)
        nd, dev = len(dim), self.val.device
        buf = torch.empty(self.nnz * nd if arr_ind else self.nnz, dtype=torch.int32 if arr_ind else torch.int64, device=dev)
        _check(_lib().svt_dev_nzwhich(self.handle, nd, (c_int64 * nd)(*dim), int(bool(arr_ind)), buf.data_ptr(), _stream()))
        return buf.view(nd, self.nnz).t() if arr_ind else buf

    @property
    def handle(self):
        return c_void_p(self._h)

    def _outputs(self, nleaves, out):
        """The (col_ptr, row_idx, val) triple a transposition / permutation writes: ``out`` checked, or new tensors."""
        dev = self.val.device
        if out is None:
            return (torch.empty(nleaves + 1, dtype=torch.int64, device=dev),
                    torch.empty(self.nnz, dtype=torch.int32, device=dev),
                    torch.empty(self.nnz, dtype=self.val.dtype, device=dev))
        cp, ri, vv = out
        assert cp.dtype == torch.int64 and cp.numel() == nleaves + 1 and cp.is_contiguous() and cp.is_cuda
        assert ri.dtype == torch.int32 and ri.numel() == self.nnz and ri.is_contiguous() and ri.is_cuda
        assert vv.dtype == self.val.dtype and vv.numel() == self.nnz and vv.is_contiguous() and vv.is_cuda
        return cp, ri, vv

    def t(self, ws=None, out=None) -> "DeviceCSC":
        """t(x) on the device (2-d operands).  ``ws``: a uint8 tensor of at least svt_dev_transpose_ws_bytes() bytes,
        ``out``: the (col_ptr, row_idx, val) tensors of the result; by default both are allocated here."""
        cp, ri, vv = self._outputs(self.nrow, out)
        if ws is None:
            ws = torch.empty(_lib().svt_dev_transpose_ws_bytes(self.nrow, self.nnz), dtype=torch.uint8,
                             device=self.val.device)
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.is_cuda
        _check(_lib().svt_dev_transpose(self.handle, cp.data_ptr(), ri.data_ptr(), vv.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()))
        return DeviceCSC(self.ncol, cp, ri, vv, logical=self.Rtype == LGLSXP)

    def aperm(self, dim, perm, ws=None, out=None):
        """aperm(x, perm) on the device for the N-d array of extents ``dim`` stored in
        this layout (dim[0] == nrow, prod(dim[1:]) == ncol); ``perm`` is 1-based.
        Returns (DeviceCSC of the permuted array, its dim).  The workspace is the permutation's own need
        (svt_dev_aperm_perm_ws_bytes): past the box limit a permutation that moves the rows takes the boxed
        driver, a leaf-preserving one needs the scratch of one scan.  ``ws`` (uint8) and ``out`` (the result's
        (col_ptr, row_idx, val) tensors) may be given; by default both are allocated here."""
        dim = np.asarray(dim, dtype=np.int64)
        perm = np.asarray(perm, dtype=np.int32)
        new_dim = tuple(int(dim[p - 1]) for p in perm)
        new_nl = int(np.prod(new_dim[1:], dtype=np.int64)) if len(new_dim) > 1 else 1
        cp, ri, vv = self._outputs(new_nl, out)
        if ws is None:
            nb = _lib().svt_dev_aperm_perm_ws_bytes(self.nnz, len(dim), dim.ctypes.data, perm.ctypes.data)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.val.device)
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.is_cuda
        _check(_lib().svt_dev_aperm(self.handle, len(dim), dim.ctypes.data, perm.ctypes.data,
                                    cp.data_ptr(), ri.data_ptr(), vv.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _stream()))
        return DeviceCSC(new_dim[0], cp, ri, vv, logical=self.Rtype == LGLSXP), new_dim

    def subset(self, rows=None, cols=None) -> "DeviceCSC":
        """x[rows, cols] on the device (2-d operands; include/svt_hip.h, svt_dev_subset): ``rows`` / ``cols`` are
        0-based int32 tensors or array-likes, in any order and with repeats, or None for the whole axis.  Returns a new
        DeviceCSC of len(rows) x len(cols).  An index out of range raises SparseArrayError; nothing is read through
        it.  Every array the composition needs is a torch allocation on the current stream."""
        dev = self.val.device
        sub = [None if v is None else _subscript(v, dev) for v in (rows, cols)]
        idx = [a for v in sub for a in ((None, -1) if v is None else (v.data_ptr(), v.numel()))]
        nrow = self.nrow if sub[0] is None else sub[0].numel()
        ncol = self.ncol if sub[1] is None else sub[1].numel()
        return _composed(lambda *a: _lib().svt_dev_subset(self.handle, *idx, *a), dev, nrow, ncol, self.Rtype)

    def subassign(self, rows, leaves, value, logical: bool = False) -> "DeviceCSC":
        """``x[rows, leaves] <- value`` on the device (include/svt_hip.h, svt_dev_subassign_vector / _svt): ``rows`` /
        ``leaves`` are 0-based int32 tensors or array-likes, or None for the whole axis.  ``value``: a scalar or a 1-D
        tensor / array (bool: logical, int32: integer -- logical with ``logical=True`` -- float64: double), recycled
        over the row subscript, rows and leaves in any order and with repeats, the last occurrence of a row winning; or
        a DeviceCSC of len(rows) x len(leaves), rows strictly increasing and leaves without repeats
        (SparseArrayUnsupported otherwise).  Returns a new DeviceCSC of the wider type of the two; nothing is read
        through an index out of range (SparseArrayError).  Every array is a torch allocation on the current stream."""
        dev = self.val.device
        sub = [None if v is None else _subscript(v, dev) for v in (rows, leaves)]
        idx = [a for v in sub for a in ((None, -1) if v is None else (v.data_ptr(), v.numel()))]
        if isinstance(value, DeviceCSC):
            call = lambda *a: _lib().svt_dev_subassign_svt(self.handle, *idx, value.handle, *a)          # noqa: E731
        else:
            vals, v_Rtype = _assign_values(value, dev, logical)
            call = lambda *a: _lib().svt_dev_subassign_vector(self.handle, *idx, vals.data_ptr(), vals.numel(),  # noqa: E731
                                                              v_Rtype, *a)
        return self._result(call)

    def _cell_index(self, index, dim, matrix):
        """The arguments (pointer, K[, ndim, dim]) of an L-index (int64[K], 0-based, LINDEX_NA for NA) or an M-index
        ((K, ndim) int32, 0-based; handed over column-major, which the result of ``nzwhich(arr_ind=True)`` already is)
        and the tensor that keeps them alive."""
        dev = self.val.device
        if not matrix:
            if not isinstance(index, torch.Tensor):
                a = np.asarray(index)
                if a.size and not np.issubdtype(a.dtype, np.integer):
                    raise SparseArrayError("subscripts must be integers")
                index = torch.as_tensor(a.astype(np.int64).reshape(-1), device=dev)
            if index.dtype != torch.int64 or not index.is_cuda:
                raise SparseArrayError("an L-index is an int64 CUDA tensor")
            index = index.contiguous().reshape(-1)
            return index, (index.data_ptr(), index.numel())
        dim = self._dim(dim)
        if not isinstance(index, torch.Tensor):
            a = np.asarray(index)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise SparseArrayError("subscripts must be integers")
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise SparseArrayError("subscript out of bounds")
            index = torch.as_tensor(a.astype(np.int32), device=dev)
        if index.dtype != torch.int32 or not index.is_cuda or index.ndim != 2 or index.shape[1] != len(dim):
            raise SparseArrayError("an M-index is a (K, ndim) int32 CUDA tensor")
        flat = index.t().contiguous()
        return flat, (flat.data_ptr(), int(index.shape[0]), len(dim), (c_int64 * len(dim))(*dim))

    def _gather(self, index, dim, matrix):
        keep, args = self._cell_index(index, dim, matrix)
        out = torch.empty(args[1], dtype=self.val.dtype, device=self.val.device)
        bad = torch.zeros(1, dtype=torch.int32, device=self.val.device)
        fn = _lib().svt_dev_subset_mindex if matrix else _lib().svt_dev_subset_lindex
        _check(fn(self.handle, *args, out.data_ptr(), bad.data_ptr(), _stream()))
        raised = int(bad.item()) if args[1] else 0          # (the one synchronisation: an index error is the caller's to see)
        if raised & 1:
            raise SparseArrayError(("matrix subscript (M-index)" if matrix else "linear index (L-index)") +
                                   " contains out-of-bound indices")
        if raised:
            raise SparseArrayError("the operand's column pointers descend or leave its nonzeros")
        return out

    def subset_lindex(self, L) -> torch.Tensor:
        """``x[L]`` by a linear index on the device (include/svt_hip.h, svt_dev_subset_lindex): ``L`` an int64 CUDA
        tensor -- the result of ``nzwhich()`` plugs straight in -- or an integer array-like, 0-based over the
        column-major array, LINDEX_NA for NA, in any order and with repeats.  Returns a tensor of the operand's dtype
        with one value per index: the stored value bit for bit, else 0 (NA under na_background), NA for an NA index.
        An index outside the array raises SparseArrayError and nothing was read through it."""
        return self._gather(L, None, False)

    def subset_mindex(self, M, dim=None) -> torch.Tensor:
        """``x[M]`` by a matrix subscript (svt_dev_subset_mindex): ``M`` a (K, ndim) int32 CUDA tensor -- the result of
        ``nzwhich(arr_ind=True)`` plugs straight in -- or an integer array-like of 0-based coordinates into the array
        of extents ``dim`` (default (nrow, ncol))."""
        return self._gather(M, dim, True)

    def _subassign_cells(self, index, value, dim, logical, matrix):
        keep, args = self._cell_index(index, dim, matrix)
        vals, v_Rtype = _assign_values(value, self.val.device, logical)
        fn = _lib().svt_dev_subassign_mindex if matrix else _lib().svt_dev_subassign_lindex
        return self._result(lambda *a: fn(self.handle, *args, vals.data_ptr(), vals.numel(), v_Rtype, *a))

    def subassign_lindex(self, L, value, logical: bool = False) -> "DeviceCSC":
        """``x[L] <- value`` by a linear index on the device (svt_dev_subassign_lindex): ``L`` as in subset_lindex, no
        NA; ``value`` a scalar or 1-D tensor / array as in subassign(), entry p of the index taking
        ``value[p % len(value)]``.  Positions apply in order (the last occurrence of a cell wins); a cell whose final
        value is zero has no entry afterwards; a cell no index reaches keeps its entry bit for bit, a stored zero
        included.  Returns a new DeviceCSC of the wider type of the two.  A strictly increasing index (what nzwhich()
        gives) takes the sorted route, any other the library's radix sort (lindex_route_counts())."""
        return self._subassign_cells(L, value, None, logical, False)

    def subassign_mindex(self, M, value, dim=None, logical: bool = False) -> "DeviceCSC":
        """``x[M] <- value`` by a matrix subscript (svt_dev_subassign_mindex): ``M`` as in subset_mindex, the rest as
        subassign_lindex."""
        return self._subassign_cells(M, value, dim, logical, True)

    def _result(self, call, rtype=None, ovflow=False) -> "DeviceCSC":
        """_composed() for a result of the operand's extents: ``rtype`` LGLSXP for Compare, Logic and is*(), None where
        the library reports the type; ``ovflow`` for Arith, Math and the Arith sweep."""
        return _composed(call, self.val.device, self.nrow, self.ncol, rtype, ovflow)

    def arith(self, op: str, other):
        """``self op other`` on the device (include/svt_hip.h, svt_dev_arith_merge / svt_dev_arith_map): ``other`` a
        DeviceCSC of the same nrow and ncol (op one of + - *) or a scalar (op one of * / ^ %% %/%; a Python int is an
        R integer, a float a double).  Returns a new DeviceCSC; its ``ovflow`` tensor says whether an integer result
        overflowed."""
        from .api import ARITH_OPCODES
        if op not in ARITH_OPCODES:
            raise SparseArrayError(f"unknown Arith operation {op!r}")
        if isinstance(other, DeviceCSC):
            return self._result(lambda *a: _lib().svt_dev_arith_merge(self.handle, other.handle, ARITH_OPCODES[op], *a),
                                ovflow=True)
        s_Rtype = INTSXP if isinstance(other, (int, np.integer)) and not isinstance(other, (bool, np.bool_)) else REALSXP
        return self._result(lambda *a: _lib().svt_dev_arith_map(self.handle, ARITH_SCALAR, ARITH_OPCODES[op], float(other),
                                                                s_Rtype, *a), ovflow=True)

    def neg(self) -> "DeviceCSC":
        """``-self`` on the device; the type is kept."""
        return self._result(lambda *a: _lib().svt_dev_arith_map(self.handle, ARITH_NEG, 0, 0.0, 0, *a), ovflow=True)

    def math(self, op: str) -> "DeviceCSC":
        """One of abs sign sqrt floor ceiling trunc log1p expm1 on a double operand; the other zero-preserving members
        of the Math group raise SparseArrayUnsupported."""
        from .api import MATH_OPCODES
        if op not in MATH_OPCODES:
            raise SparseArrayError(f"unknown Math operation {op!r}")
        return self._result(lambda *a: _lib().svt_dev_arith_map(self.handle, ARITH_MATH, MATH_OPCODES[op], 0.0, 0, *a),
                            ovflow=True)

    def compare(self, op: str, other) -> "DeviceCSC":
        """``self op other`` on the device (include/svt_hip.h, svt_dev_compare_merge / svt_dev_compare_map): ``other`` a
        DeviceCSC of the same nrow and ncol (op one of != < >) or a scalar against which zero compares FALSE (any of
        == != <= >= < >; a Python bool is an R logical, an int an integer, a float a double).  Returns a logical
        DeviceCSC whose values are 1 or NA_integer."""
        from .api import COMPARE_OPCODES
        if op not in COMPARE_OPCODES:
            raise SparseArrayError(f"unknown Compare operation {op!r}")
        if isinstance(other, DeviceCSC):
            return self._result(lambda *a: _lib().svt_dev_compare_merge(self.handle, other.handle, COMPARE_OPCODES[op], *a),
                                LGLSXP)
        s_Rtype = (LGLSXP if isinstance(other, (bool, np.bool_)) else
                   INTSXP if isinstance(other, (int, np.integer)) else REALSXP)
        return self._result(lambda *a: _lib().svt_dev_compare_map(self.handle, COMPARE_OPCODES[op], float(other), s_Rtype, *a),
                            LGLSXP)

    def _pminmax(self, name: str, other, na_rm) -> "DeviceCSC":
        from .api import PMINMAX_NA_RM, PMINMAX_OPCODES
        op = PMINMAX_OPCODES[name] | (PMINMAX_NA_RM if na_rm else 0)
        if isinstance(other, DeviceCSC):
            return self._result(lambda *a: _lib().svt_dev_pminmax_merge(self.handle, other.handle, op, *a))
        s_Rtype = (LGLSXP if isinstance(other, (bool, np.bool_)) else
                   INTSXP if isinstance(other, (int, np.integer)) else REALSXP)
        try:
            return self._result(lambda *a: _lib().svt_dev_pminmax_map(self.handle, op, float(other), s_Rtype, *a))
        except SparseArrayError as e:
            if "result wouldn't be sparse" not in str(e):
                raise
            raise SparseArrayError(f"{name}(x, {other!r}): {name}(0, {other!r}) is not 0 (result wouldn't be sparse)") from e

    def pmin(self, other, na_rm: bool = False) -> "DeviceCSC":
        """``pmin(self, other)`` on the device (include/svt_hip.h, svt_dev_pminmax_merge / svt_dev_pminmax_map): ``other``
        a DeviceCSC of the same nrow and ncol, or a scalar that is not NA / NaN and ``>= 0`` (a Python bool is an R
        logical, an int an integer, a float a double) -- ``x.pmin(s)`` caps the outliers in one pass.  The result has the
        wider of the two types; an NA on either side gives NA unless ``na_rm``, which then gives the other side."""
        return self._pminmax("pmin", other, na_rm)

    def pmax(self, other, na_rm: bool = False) -> "DeviceCSC":
        """``pmax(self, other)``; as pmin, the scalar ``<= 0``."""
        return self._pminmax("pmax", other, na_rm)

    def _isfun(self, name: str) -> "DeviceCSC":
        from .api import ISFUN_OPCODES
        return self._result(lambda *a: _lib().svt_dev_isfun_map(self.handle, ISFUN_OPCODES[name], *a), LGLSXP)

    def is_na(self) -> "DeviceCSC":
        """``is.na(self)`` on the device (svt_dev_isfun_map): a logical DeviceCSC that stores 1 where an entry is NA or
        NaN (NA_integer_ for an integer or logical operand)."""
        return self._isfun("is.na")

    def is_nan(self) -> "DeviceCSC":
        """``is.nan(self)``: 1 where an entry is a NaN that is not NA_real_; empty for an integer or logical operand."""
        return self._isfun("is.nan")

    def is_infinite(self) -> "DeviceCSC":
        """``is.infinite(self)``: 1 where an entry is +-Inf; empty for an integer or logical operand."""
        return self._isfun("is.infinite")

    def sweep(self, op: str, stats, margin=2, dim=None, logical: bool = False, na_rm: bool = False) -> "DeviceCSC":
        """``sweep(x, margin, stats, op)`` on the device (include/svt_hip.h, svt_dev_arith_sweep / svt_dev_compare_sweep):
        every stored value meets the element of ``stats`` that belongs to its position along ``margin`` -- 1-based, an
        int or a strictly increasing run of consecutive dimensions of the array of extents ``dim`` (default
        (nrow, ncol): 1 the rows, 2 the columns).  ``t(t(x) / colSums(x))`` is ``x.sweep("/", colstats(x, "sum")[0])``,
        R's ``x * w`` with ``len(w) == nrow`` is ``x.sweep("*", w, 1)``.  ``op``: one of ``* / ^ %% %/%`` or of the six
        comparison operators, or ``"pmin"`` / ``"pmax"`` (a cap or a floor per row or per leaf, with ``na_rm`` as in
        pmin(); svt_dev_pminmax_sweep; the result has the wider of the two types).  ``stats``: a float64 or int32 tensor
        on the operand's device (bool, or int32 with ``logical=True``: logical, for Compare and pmin / pmax, not for
        Arith), or an array-like; prod(dim[margin]) elements, an N-d one read column-major.  Returns a new DeviceCSC,
        with ``ovflow`` for Arith, logical for Compare, of the wider type for pmin / pmax.  An element that would
        not keep the result sparse (NA, zero under ``/``, ...) raises SparseArrayError naming its 0-based index and
        value; the library finds it on the device and nothing was written."""
        from .api import ARITH_OPCODES, COMPARE_OPCODES, PMINMAX_NA_RM, PMINMAX_OPCODES
        compare, pminmax = op in COMPARE_OPCODES, op in PMINMAX_OPCODES
        if not compare and not pminmax and op not in ARITH_OPCODES:
            raise SparseArrayError(f"unknown Arith or Compare operation {op!r}")
        if op in ("+", "-"):
            raise SparseArrayError(f"\"{op}\" is not supported between a SparseArray object and a vector "
                                   "(result wouldn't be sparse in general)")
        with_rows, stride, length = sweep_form(self._dim(dim), margin)
        if isinstance(stats, torch.Tensor):
            if stats.device != self.val.device:
                raise SparseArrayError("'stats' must be on the operand's device")
            if stats.ndim > 1:
                stats = stats.permute(*reversed(range(stats.ndim)))
        else:
            stats = np.asarray(stats).reshape(-1, order="F")
        vals, s_Rtype = _assign_values(stats, self.val.device, logical)
        bad = c_int64(-1)
        geometry = (vals.data_ptr(), s_Rtype, vals.numel(), with_rows, stride, length)
        try:
            if pminmax:
                return self._result(lambda *a: _lib().svt_dev_pminmax_sweep(
                    self.handle, PMINMAX_OPCODES[op] | (PMINMAX_NA_RM if na_rm else 0), *geometry, *a[:-1],
                    ctypes.byref(bad), a[-1]))
            if compare:
                return self._result(lambda *a: _lib().svt_dev_compare_sweep(
                    self.handle, COMPARE_OPCODES[op], *geometry, *a[:-1], ctypes.byref(bad), a[-1]), LGLSXP)
            return self._result(lambda *a: _lib().svt_dev_arith_sweep(
                self.handle, ARITH_OPCODES[op], *geometry, *a[:-1], ctypes.byref(bad), a[-1]), ovflow=True)
        except SparseArrayError as e:
            if bad.value < 0:
                raise
            value = vals[bad.value].item()                      # (the error path's one read of an element)
            raise SparseArrayError(f"sweep(\"{op}\"): stats[{bad.value}] = {value!r} does not keep the result sparse "
                                   "(result wouldn't be sparse)") from e

    def logic(self, op: str, other: "DeviceCSC") -> "DeviceCSC":
        """``self & other`` / ``self | other`` on the device for two logical operands (svt_dev_logic_merge)."""
        from .api import LOGIC_OPCODES
        if op not in LOGIC_OPCODES:
            raise SparseArrayError(f"unknown Logic operation {op!r}")
        if not isinstance(other, DeviceCSC):
            raise SparseArrayError("logic() takes two DeviceCSC operands")
        return self._result(lambda *a: _lib().svt_dev_logic_merge(self.handle, other.handle, LOGIC_OPCODES[op], *a), LGLSXP)

    def matmul_sparse(self, other: "DeviceCSC"):
        """``self %*% other`` with a resident sparse result: (DeviceCSC of type double, not_finite), see
        matmul_csc_csc_sparse()."""
        return matmul_csc_csc_sparse(self, other)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib().svt_release(self._h)
                self._h = None
        except Exception:
            pass


class _TorchBlocks:
    """svt_dev_alloc_fn / svt_dev_free_fn over torch allocations on the current stream (include/svt_hip.h,
    svt_dev_subset): a block lives until the library releases it, or, for the result arrays it hands back, as the
    tensors ``csc()`` returns."""

    def __init__(self, device):
        self.device, self.live = device, {}
        self.alloc_fn, self.free_fn = ALLOC_FN(self._alloc), FREE_FN(self._release)

    def _alloc(self, nbytes, _ctx):
        try:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        except RuntimeError:
            return None
        self.live[t.data_ptr()] = t
        return t.data_ptr()

    def _release(self, p, _ctx):
        self.live.pop(p, None)

    def csc(self, out, ncol, nnz, dtype):
        """the (col_ptr, row_idx, val) tensors behind the three result pointers ``out``; nothing else is kept"""
        live, self.live = self.live, {}
        return (live[out[0].value].view(torch.int64)[:ncol + 1], live[out[1].value].view(torch.int32)[:nnz],
                live[out[2].value].view(dtype)[:nnz])


def _composed(call, device, nrow, ncol=None, rtype=None, ovflow=False) -> DeviceCSC:
    """The new DeviceCSC that a composition of the library -- count, allocate, fill over the caller's allocator
    (include/svt_hip.h, svt_dev_subset) -- leaves in torch allocations on the current stream.  ``call`` is given the
    arguments from ``alloc`` on, in the header's order: alloc, release, ctx, [out_nrow, out_nleaves: ``ncol`` None, the
    library reports the extents (abind),] [out_Rtype: ``rtype`` None, the library reports the type,] out_nnz,
    out_col_ptr, out_row_idx, out_val, [the overflow word: ``ovflow``,] stream.  With ``ovflow`` the result's ``ovflow``
    attribute is that device word (int32 tensor; nonzero once the fill has run: "NAs produced by integer overflow"),
    left on the device so that the call stays asynchronous after its count."""
    mem = _TorchBlocks(device)
    dims = [] if ncol is not None else [c_int64(0), c_int64(0)]
    rt = [] if rtype is not None else [ctypes.c_int(0)]
    nnz, out = c_int64(0), [c_void_p(0), c_void_p(0), c_void_p(0)]
    word = [torch.zeros(1, dtype=torch.int32, device=device)] if ovflow else []
    _check(call(mem.alloc_fn, mem.free_fn, None, *[ctypes.byref(c) for c in dims + rt + [nnz] + out],
                *[w.data_ptr() for w in word], _stream()))
    if dims:
        nrow, ncol = int(dims[0].value), int(dims[1].value)
    if rt:
        rtype = rt[0].value
    dtype = torch.float64 if rtype == REALSXP else torch.int32
    R = DeviceCSC(nrow, *mem.csc(out, ncol, int(nnz.value), dtype), logical=rtype == LGLSXP)
    if word:
        R.ovflow = word[0]
    return R


def _two_calls(device, nrow, ncol, dtype, logical, count, fill, need=0, ws=None, col_ptr=None) -> DeviceCSC:
    """The two-call form of the same protocol, every array a tensor made here: the workspace (``ws``, or ``need`` bytes)
    and col_ptr (``col_ptr``, or int64[ncol + 1]), ``count(col_ptr, out_nnz, ws, ws_bytes, stream)``, row_idx and val for
    the nonzeros it found, ``fill(col_ptr, nnz, row_idx, val, ws, ws_bytes, stream)``."""
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.is_cuda
    cp = torch.empty(ncol + 1, dtype=torch.int64, device=device) if col_ptr is None else col_ptr
    nnz = c_int64(0)
    _check(count(cp.data_ptr(), ctypes.byref(nnz), ws.data_ptr(), ws.numel(), _stream()))
    ri = torch.empty(nnz.value, dtype=torch.int32, device=device)
    vv = torch.empty(nnz.value, dtype=dtype, device=device)
    _check(fill(cp.data_ptr(), nnz.value, ri.data_ptr(), vv.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return DeviceCSC(nrow, cp, ri, vv, logical=logical)


def _subscript(v, device) -> torch.Tensor:
    """A subscript as a contiguous int32 device tensor (the values are checked on the device)."""
    if not isinstance(v, torch.Tensor):
        a = np.asarray(v)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise SparseArrayError("subscripts must be integers")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise SparseArrayError("subscript out of bounds")
        v = torch.as_tensor(a.astype(np.int32).reshape(-1), device=device)
    assert v.dtype == torch.int32 and v.is_cuda
    return v.contiguous().reshape(-1)


def _assign_values(value, device, logical=False):
    """(contiguous 1-D device tensor, its R type) of the new values of a vector subassignment."""
    if isinstance(value, torch.Tensor):
        v = value.reshape(-1)
    else:
        a = np.asarray(value)
        if a.dtype != np.bool_ and np.issubdtype(a.dtype, np.integer):
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise SparseArrayError("integer values must fit in 32 bits")
            a = a.astype(np.int32)
        elif np.issubdtype(a.dtype, np.floating):
            a = a.astype(np.float64)
        v = torch.as_tensor(a.reshape(-1), device=device)
    if v.dtype == torch.bool:
        v, logical = v.to(torch.int32), True
    if v.dtype not in (torch.int32, torch.float64):
        raise SparseArrayError("the value must be logical, integer (int32) or double (float64)")
    assert v.is_cuda
    return v.contiguous(), (REALSXP if v.dtype == torch.float64 else LGLSXP if logical else INTSXP)


def subassign_tile() -> int:
    """Entries of the placed operand per workgroup tile of the placement's fill (svt_dev_subassign_tile).  Needs no GPU."""
    return int(_hip.load_library().svt_dev_subassign_tile())


def subassign_place(nrow, ncol, rows, leaves, value, logical=False, ws=None, tables=None, col_ptr=None):
    """The placement alone (svt_dev_subassign_place_*_count, then _fill): returns (Y, cover_row, cover_leaf) -- the
    placed operand of ``x[rows, leaves] <- value`` for an x of nrow x ncol and the two uint8 cover tables (None for a
    whole axis).  ``ws`` (uint8), ``tables`` (the two uint8 tensors) and ``col_ptr`` (int64[ncol + 1]) may be given."""
    lib = _lib()
    dev = value.val.device if isinstance(value, DeviceCSC) else torch.device("cuda")
    sub = [None if v is None else _subscript(v, dev) for v in (rows, leaves)]
    idx = [a for v in sub for a in ((None, -1) if v is None else (v.data_ptr(), v.numel()))]
    if tables is None:
        tables = [None if s is None else torch.empty(n, dtype=torch.uint8, device=dev) for s, n in zip(sub, (nrow, ncol))]
    tab = [None if t is None else t.data_ptr() for t in tables]
    if isinstance(value, DeviceCSC):
        what, dtype, is_lgl = (value.handle,), value.val.dtype, value.Rtype == LGLSXP
        count, fill = lib.svt_dev_subassign_place_svt_count, lib.svt_dev_subassign_place_svt_fill
    else:
        vals, v_Rtype = _assign_values(value, dev, logical)
        what, dtype, is_lgl = (vals.data_ptr(), vals.numel(), v_Rtype), vals.dtype, v_Rtype == LGLSXP
        count, fill = lib.svt_dev_subassign_place_vector_count, lib.svt_dev_subassign_place_vector_fill
    Y = _two_calls(dev, nrow, ncol, dtype, is_lgl,
                   lambda cp, nnz, *w: count(nrow, ncol, *idx, *what, cp, *tab, nnz, *w),
                   lambda cp, *a: fill(nrow, ncol, *idx, *what, cp, *a),
                   lib.svt_dev_subassign_place_ws_bytes(nrow, ncol), ws, col_ptr)
    return Y, tables[0], tables[1]


def assign_merge(x: DeviceCSC, y: DeviceCSC, cover_row=None, cover_leaf=None, ws=None, col_ptr=None) -> DeviceCSC:
    """The assign merge alone (svt_dev_assign_merge_count, then _fill): x with the placed operand ``y`` written over
    it under the two cover tables (uint8 tensors; None: the whole axis)."""
    tab = [None if t is None else t.data_ptr() for t in (cover_row, cover_leaf)]
    return _merge_two_calls(x, y, _lib().svt_dev_assign_merge_count, _lib().svt_dev_assign_merge_fill, tab, ws, col_ptr)


def _merge_two_calls(x, y, count, fill, tab, ws, col_ptr) -> DeviceCSC:
    """_two_calls() for a merge of the placed operand ``y`` over ``x``: the result has the wider type of the two"""
    return _two_calls(x.val.device, x.nrow, x.ncol, torch.float64 if REALSXP in (x.Rtype, y.Rtype) else torch.int32,
                      x.Rtype == LGLSXP and y.Rtype == LGLSXP,
                      lambda *a: count(x.handle, y.handle, *tab, *a),
                      lambda cp, nnz, *a: fill(x.handle, y.handle, *tab, cp, *a),
                      _lib().svt_dev_arith_merge_ws_bytes(x.ncol, x.nnz, y.nnz), ws, col_ptr)


# the NA of an L-index (include/svt_hip.h, svt_dev_subset_lindex)
LINDEX_NA = -2 ** 63


def lindex_route_counts(reset=False) -> dict:
    """Sorted and unsorted placements of this process so far (svt_dev_lindex_route_counts)."""
    buf = (c_int64 * 2)()
    _lib().svt_dev_lindex_route_counts(buf, int(bool(reset)))
    return {"sorted": int(buf[0]), "unsorted": int(buf[1])}


def lindex_sort_passes(nrow: int, ncol: int) -> int:
    """8-bit passes of the unsorted route's sort for an array of nrow x ncol cells (svt_dev_lindex_sort_passes).  Needs
    no GPU."""
    return int(_hip.load_library().svt_dev_lindex_sort_passes(nrow, ncol))


def lindex_place(x: DeviceCSC, index, value, dim=None, matrix=False, logical=False, ws=None, col_ptr=None) -> DeviceCSC:
    """The placement alone (svt_dev_subassign_place_lindex_count, then _fill): the placed operand Y of ``x[index] <-
    value`` -- one entry per distinct assigned cell, zeros included.  ``ws`` (uint8) and ``col_ptr`` (int64[ncol + 1]) may
    be given."""
    lib, dev = _lib(), x.val.device
    keep, args = x._cell_index(index, dim, matrix)
    args = args if matrix else args + (0, None)
    vals, v_Rtype = _assign_values(value, dev, logical)
    what = (x.nrow, x.ncol, *args, vals.data_ptr(), vals.numel(), v_Rtype)
    return _two_calls(dev, x.nrow, x.ncol, vals.dtype, v_Rtype == LGLSXP,
                      lambda *a: lib.svt_dev_subassign_place_lindex_count(*what, *a),
                      lambda *a: lib.svt_dev_subassign_place_lindex_fill(*what, *a),
                      lib.svt_dev_subassign_place_lindex_ws_bytes(args[1], x.ncol), ws, col_ptr)


def assign_cells_merge(x: DeviceCSC, y: DeviceCSC, ws=None, col_ptr=None) -> DeviceCSC:
    """The merge under the rule of the subassignment by cells alone (svt_dev_assign_cells_merge_count, then _fill): x
    with the placed operand ``y`` written over it, a zero of ``y`` deleting."""
    lib = _lib()
    return _merge_two_calls(x, y, lib.svt_dev_assign_cells_merge_count, lib.svt_dev_assign_cells_merge_fill, (), ws, col_ptr)


# kinds of svt_dev_arith_map / svt_dev_arith_out_Rtype (include/svt_hip.h)
ARITH_MERGE, ARITH_SCALAR, ARITH_NEG, ARITH_MATH = 0, 1, 2, 3


def arith_tile() -> int:
    """Entries per workgroup tile of the Arith / Math kernels (svt_dev_arith_tile).  Needs no GPU."""
    return int(_hip.load_library().svt_dev_arith_tile())


def sweep_form(dim, margin):
    """(with_rows, stride, len) of ``sweep(x, margin, ...)`` for the array of extents ``dim`` (include/svt_hip.h,
    svt_dev_arith_sweep): the entry of row r in leaf q meets element
    ``(r if with_rows else 0) + (nrow if with_rows else 1) * ((q // stride) % len)`` of the column-major array of the
    margin's extents.  ``margin``: 1-based, an int or a strictly increasing run of consecutive dimensions; any other
    raises SparseArrayError.  Needs no GPU."""
    dim = tuple(int(d) for d in dim)
    m = (margin,) if isinstance(margin, (int, np.integer)) else tuple(margin)
    if (not m or any(isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) for k in m)
            or any(k < 1 or k > len(dim) for k in m)):
        raise SparseArrayError(f"'margin' must name dimensions between 1 and {len(dim)}")
    if any(b != a + 1 for a, b in zip(m, m[1:])):
        raise SparseArrayError("'margin' must be a strictly increasing run of consecutive dimensions (e.g. 2 or (2, 3)); "
                               f"{tuple(int(k) for k in m)} is not supported")
    stride = int(np.prod(dim[1:max(m[0] - 1, 1)], dtype=np.int64))
    length = int(np.prod([dim[k - 1] for k in m if k > 1], dtype=np.int64))
    return int(m[0] == 1), stride, length


def subset_tile() -> int:
    """Nonzeros per workgroup tile of the column gather and the row filter (svt_dev_subset_tile).  Needs no GPU."""
    lib = _hip.load_library()
    return int(lib.svt_dev_subset_tile())


def subset_route_counts(reset=False) -> dict:
    """Column gathers, row filters and general-row compositions of this process so far (svt_dev_subset_route_counts)."""
    buf = (c_int64 * 3)()
    _lib().svt_dev_subset_route_counts(buf, int(bool(reset)))
    return dict(zip(("column_gather", "row_filter", "general_rows"), (int(x) for x in buf)))


def _subset_two_calls(A: DeviceCSC, idx, ws, rows: bool) -> DeviceCSC:
    lib, dev = _lib(), A.val.device
    idx = _subscript(idx, dev)
    n = idx.numel()
    if rows:
        return _two_calls(dev, n, A.ncol, A.val.dtype, A.Rtype == LGLSXP,
                          lambda *a: lib.svt_dev_subset_rows_count(A.handle, idx.data_ptr(), n, *a),
                          lambda cp, nnz, *a: lib.svt_dev_subset_rows_fill(A.handle, cp, *a),
                          lib.svt_dev_subset_rows_ws_bytes(A.nrow, A.ncol, A.nnz), ws)
    return _two_calls(dev, A.nrow, n, A.val.dtype, A.Rtype == LGLSXP,
                      lambda *a: lib.svt_dev_subset_cols_count(A.handle, idx.data_ptr(), n, *a),
                      lambda cp, nnz, ri, vv, *w: lib.svt_dev_subset_cols_fill(A.handle, idx.data_ptr(), n, cp, ri, vv, w[-1]),
                      lib.svt_dev_subset_cols_ws_bytes(n), ws)


def subset_cols(A: DeviceCSC, cols, ws=None) -> DeviceCSC:
    """The column gather alone (svt_dev_subset_cols_count, then _fill): x[, cols], ``cols`` 0-based, any order, repeats."""
    return _subset_two_calls(A, cols, ws, rows=False)


def subset_rows(A: DeviceCSC, rows, ws=None) -> DeviceCSC:
    """The row filter alone (svt_dev_subset_rows_count, then _fill): x[rows, ] for a strictly increasing 0-based
    ``rows``; any other subscript in range raises SparseArrayUnsupported (take ``A.subset(rows=...)``)."""
    return _subset_two_calls(A, rows, ws, rows=True)


def _rtype_of(type_name) -> int:
    try:
        return {"logical": LGLSXP, "integer": INTSXP, "double": REALSXP}[type_name]
    except (KeyError, TypeError):
        raise SparseArrayError("invalid requested type") from None


def coerce_tile() -> int:
    """Cells (dense <-> sparse) or entries (nzwhich) per workgroup tile of the coercion kernels (svt_dev_coerce_tile).
    Needs no GPU."""
    return int(_hip.load_library().svt_dev_coerce_tile())


def _seed_bits(seed) -> int:
    """``seed`` in [0, 2^64) as the int64 of the same bits, which is how the C ABI takes it"""
    seed = seed_word(seed)
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def poisson_ticks(lambda_: float):
    """The table of cumulated Poisson probabilities behind poisson() and rpois() (svt_poisson_ticks): a float64 array of at
    most 32 ticks, empty when every cell is 0; "'lambda' too big?" when 32 are not enough.  Needs no GPU."""
    buf = (ctypes.c_double * 32)()
    n = _hip.load_library().svt_poisson_ticks(float(lambda_), buf)
    if n < 0:
        raise SparseArrayError("'lambda' too big?" if lambda_ >= 0 else "'lambda' must be a non-negative number")
    return np.array(buf[:n], dtype=np.float64)


def poisson(dim, lambda_=None, density=None, seed=0, first_leaf=0, nleaves=None, device="cuda") -> DeviceCSC:
    """poissonSparseArray(dim, lambda, density) made on the device (include/svt_hip.h, svt_dev_poisson): the integer
    operand with nrow = dim[0] whose leaves are the prod(dim[1:]) leaves of the array, every cell drawn from
    Poisson(lambda) and the nonzeros kept.  A cell is a function of (seed, its flat index in the whole array), so
    ``first_leaf`` / ``nleaves`` give the window of leaves [first_leaf, first_leaf + nleaves) of the same array (default:
    from first_leaf to the end): the windows, bound by cbind(), are the array.  ``seed``: an integer in [0, 2^64).  Every
    array is a torch allocation on the current stream."""
    dim = normarg_dim(dim)
    lam = poisson_lambda(lambda_, density)
    bits = _seed_bits(seed)
    total = int(np.prod(dim[1:], dtype=object)) if len(dim) > 1 else 1
    first_leaf = int(first_leaf)
    nleaves = total - first_leaf if nleaves is None else int(nleaves)
    if first_leaf < 0 or nleaves < 0 or first_leaf + nleaves > total:
        raise SparseArrayError("the window of leaves is not inside the array")
    return _composed(lambda *r: _lib().svt_dev_poisson(lam, bits, dim[0], first_leaf, nleaves, *r), torch.device(device), dim[0],
                     nleaves, INTSXP)


def rpois(n, lambda_, seed=0, first=0, device="cuda") -> torch.Tensor:
    """simple_rpois(n, lambda) on the device (svt_dev_rpois): the int32 tensor of the cells [first, first + n) of the
    stream of ``seed`` -- the dense form of poisson(): rpois(nrow * ncol) read column-major is the array."""
    n = int(n)
    if n < 0:
        raise SparseArrayError("'n' cannot be negative")
    lam = poisson_lambda(lambda_, None)
    out = torch.empty(n, dtype=torch.int32, device=device)
    _check(_lib().svt_dev_rpois(lam, _seed_bits(seed), int(first), n, out.data_ptr(), _stream()))
    return out


def abind_tile() -> int:
    """Result entries per workgroup tile of the copy of abind (svt_dev_abind_tile).  Needs no GPU."""
    return int(_hip.load_library().svt_dev_abind_tile())


def _abind_operands(objects, along, dim):
    """(handle array, inner, ext array or None, ans_Rtype, result dim) of abind(objects, along, dim): the dims are
    checked here, the way svt_abind_SVT_begin checks those of host operands."""
    objects = list(objects)
    if not objects or not all(isinstance(o, DeviceCSC) for o in objects):
        raise SparseArrayError("abind() takes one or more DeviceCSC operands")
    dims = [(o.nrow, o.ncol) for o in objects] if dim is None else [tuple(int(d) for d in dd) for dd in dim]
    if len(dims) != len(objects):
        raise SparseArrayError("'dim' must hold the dim of every object")
    nd = len(dims[0])
    if not 1 <= along <= nd:
        raise SparseArrayError("'along' must be >= 1 and <= the number of dimensions of the objects to bind")
    for o, dd in zip(objects, dims):
        if len(dd) != nd:
            raise SparseArrayError("all the objects to bind must have the same number of dimensions")
        if dd[0] != o.nrow or int(np.prod(dd[1:], dtype=np.int64)) != o.ncol:
            raise SparseArrayError("'dim' does not match the operand's rows and leaves")
        for k in range(nd):
            if k != along - 1 and dd[k] != dims[0][k]:
                raise SparseArrayError(f"all the objects to bind must have the same extent along dimension {k + 1} (they "
                                       f"are bound along dimension {along})")
    new_dim = tuple(sum(dd[k] for dd in dims) if k == along - 1 else d for k, d in enumerate(dims[0]))
    handles = (c_void_p * len(objects))(*[o._h for o in objects])
    ext = None if along == 1 else (c_int64 * len(objects))(*[dd[along - 1] for dd in dims])
    inner = int(np.prod(dims[0][1:along - 1], dtype=np.int64)) if along > 2 else 1
    ans_Rtype = max((o.Rtype for o in objects), key=(LGLSXP, INTSXP, REALSXP).index)
    return objects, handles, inner, ext, ans_Rtype, new_dim


def abind(objects, along=1, dim=None):
    """abind() of resident operands along dimension ``along`` (1-based; include/svt_hip.h, svt_dev_abind).  ``dim``:
    the dim of every object, one tuple each, for N-d operands (dim[0] == nrow, prod(dim[1:]) == ncol); None: every
    object is the 2-D (nrow, ncol).  The result's type is the widest of logical < integer < double over the objects
    (logical only when every object is logical) and the values widen on the device.  Returns (DeviceCSC, its dim); every
    array is a torch allocation on the current stream."""
    objects, handles, inner, ext, ans_Rtype, new_dim = _abind_operands(objects, int(along), dim)
    R = _composed(lambda *a: _lib().svt_dev_abind(handles, len(objects), inner, ext, ans_Rtype, *a), objects[0].val.device,
                  None, None, ans_Rtype)
    return R, new_dim


def cbind(*objects) -> DeviceCSC:
    """cbind() of resident 2-D operands of the same nrow: their columns one object after the other."""
    return abind(objects, along=2)[0]


def rbind(*objects) -> DeviceCSC:
    """rbind() of resident 2-D operands of the same ncol: in every column their rows one object after the other."""
    return abind(objects, along=1)[0]


class CrossprodPlan:
    """Reusable workspace for crossprod(A, Y) with K dense columns."""

    def __init__(self, A: DeviceCSC, K: int):
        self.A, self.K = A, int(K)
        n = _lib().svt_dev_crossprod_ws_bytes(A.nrow, A.ncol, self.K)
        self.ws = torch.empty(n, dtype=torch.uint8, device=A.val.device)

    def prepare(self, Y: torch.Tensor, ldY: int, tr_y: bool = False):
        """Y: device buffer holding the dense operand in R (column-major) layout."""
        _check(_lib().svt_dev_dense_prepare(Y.data_ptr(), ldY, self.A.nrow, self.K,
                                            int(tr_y), self.A.Rtype, self.ws.data_ptr(),
                                            self.ws.numel(), _stream()))

    def multiply(self, out: torch.Tensor, stride_c: int, stride_k: int):
        _check(_lib().svt_dev_crossprod_prepared(self.A.handle, self.ws.data_ptr(), self.K,
                                                 out.data_ptr(), stride_c, stride_k, _stream()))

    def run(self, Y, ldY, out, stride_c=1, stride_k=None, tr_y=False):
        if stride_k is None:
            stride_k = self.A.ncol
        self.prepare(Y, ldY, tr_y)
        self.multiply(out, stride_c, stride_k)


class PbcPlan:
    """Fast path of crossprod(A, Y) for f64: panel-blocked copy of A (built
    once, here) + workspace for K dense columns.

    Layouts (CBW, WPB, logR), 1 <= CBW <= 40: (CBW, 16, 7) for the LDS-DMA kernel,
    (CBW, 4, 9..15) for the gather kernels, (0, 0, 0) to let the library pick one
    by density.  Any other layout raises SparseArrayError.  Below 256 rows an
    LDS-DMA layout holds no records and the general kernels answer the product."""

    def __init__(self, A: DeviceCSC, K: int, CBW: int = 40, WPB: int = 16, logR: int = 7):
        assert A.Rtype == REALSXP
        self.A, self.K = A, int(K)
        self._p = _lib().svt_dev_pbc_build(A.handle, CBW, WPB, logR)
        if not self._p:
            raise SparseArrayError(_lib().svt_last_error().decode())
        n = _lib().svt_dev_crossprod_pbc_ws_bytes(self._p, self.K)
        self.ws = torch.empty(n, dtype=torch.uint8, device=A.val.device)

    def run(self, Y, ldY, out, stride_c=1, stride_k=None, tr_y=False):
        if stride_k is None:
            stride_k = self.A.ncol
        _check(_lib().svt_dev_crossprod_pbc(self._p, self.A.handle, Y.data_ptr(), ldY, self.K,
                                            int(tr_y), out.data_ptr(), stride_c, stride_k,
                                            self.ws.data_ptr(), self.ws.numel(), _stream()))

    def run_from(self, first_col, Y, ldY, out, stride_c=1, stride_k=None, tr_y=False):
        """The product restricted to the leaves from ``first_col`` on (svt_dev_crossprod_pbc_from)."""
        if stride_k is None:
            stride_k = self.A.ncol
        _check(_lib().svt_dev_crossprod_pbc_from(self._p, self.A.handle, Y.data_ptr(), ldY, self.K,
                                                 int(tr_y), out.data_ptr(), stride_c, stride_k,
                                                 self.ws.data_ptr(), self.ws.numel(), _stream(), int(first_col)))

    def plan(self, stride_c=1, stride_k=None, tr_y=False, first_col=0) -> dict:
        """What run() / run_from() with these arguments launches under the present knobs: kind, kernel, NV, nsplit,
        panels_per_split, direct, launches, tail_splits, tail_blocks (svt_dev_crossprod_pbc_plan).  Launches nothing."""
        if stride_k is None:
            stride_k = self.A.ncol
        return _hip.pbc_plan(self._p, self.K, tr_y, stride_c, stride_k, first_col)

    def run_phase(self, phase, Y, ldY, out, stride_c=1, stride_k=None, tr_y=False):
        if stride_k is None:
            stride_k = self.A.ncol
        _check(_lib().svt_dev_crossprod_pbc_phase(self._p, self.A.handle, Y.data_ptr(), ldY,
                                                  self.K, int(tr_y), out.data_ptr(), stride_c,
                                                  stride_k, self.ws.data_ptr(), self.ws.numel(),
                                                  _stream(), phase))

    def __del__(self):
        try:
            if getattr(self, "_p", None):
                _lib().svt_dev_pbc_release(self._p)
                self._p = None
        except Exception:
            pass


def transpose_plan(nrow: int, ncol: int, nnz: int, nslab: int = 1) -> dict:
    """Which form ``DeviceCSC.t()`` takes for such an operand, or (``nslab`` > 1) the batched transposition of aperm's
    "first two axes change places" (svt_dev_transpose_plan; _hip.transpose_plan).  Launches nothing, needs no GPU."""
    return _hip.transpose_plan(nrow, ncol, nnz, nslab)


def aperm_route_counts(reset=False) -> dict:
    """Which route the transpositions / permutations of this process took so far (svt_dev_aperm_route_counts)."""
    names = ("t_bucketed", "t_key_sort", "leaf_preserving", "first_two_axes_swapped", "slab", "via_intermediate_3d",
             "general_composed", "key_sort_32", "key_sort_64", "slab_refused_at_run_time")
    buf = (c_int64 * 10)()
    _lib().svt_dev_aperm_route_counts(buf, int(bool(reset)))
    return dict(zip(names, (int(x) for x in buf)))


def set_box_nnz(n: int = 0) -> None:
    """Box limit of the device transposition and of the aperm that moves the rows (svt_dev_set_box_nnz): n > 0
    sends every such operand of more than n nonzeros through the boxed driver with boxes of at most n (or one
    column / one index of the axis that becomes the rows); n <= 0 restores the default (from 2^31 nonzeros on,
    boxes of 2^30 for t(), 2^28 for aperm).  Leaf-preserving permutations are never boxed."""
    _lib().svt_dev_set_box_nnz(int(n))


def boxed_calls(reset=False) -> int:
    """Transpositions and row-moving permutations of this process that took a boxed driver, one per call
    (svt_dev_boxed_calls)."""
    return int(_lib().svt_dev_boxed_calls(int(bool(reset))))


def trim_layout_pool() -> None:
    """Returns the memory the layout pools keep for the next build to the driver (svt_dev_pbc_trim)."""
    _lib().svt_dev_pbc_trim()


def set_spare_cus(n: int) -> None:
    """CUs the LDS-DMA product kernel leaves idle from now on (0 = none; include/svt_hip.h:
    svt_dev_pbc_set_spare_cus) -- room for a collective's kernels beside the product."""
    _lib().svt_dev_pbc_set_spare_cus(int(n))


def spare_cus() -> int:
    return int(_lib().svt_dev_pbc_spare_cus())


def set_gather_pacing(dsync: int = 1, spin: int = 256) -> None:
    """Pacing of the gather product of very sparse operands (include/svt_hip.h:
    svt_dev_pbc_set_gather_pacing); dsync < 0 selects the unpaced kernels."""
    _lib().svt_dev_pbc_set_gather_pacing(int(dsync), int(spin))


def set_round_launches(on=True) -> None:
    """One launch per round of workgroups for products with many column blocks (svt_dev_pbc_set_round_launches):
    False / 0 = one launch, True / 1 = per round with the partly filled last round cut by rows (default), 2 = per
    round with the last round whole."""
    _lib().svt_dev_pbc_set_round_launches(int(on))


def crossprod_csc_dense(A: DeviceCSC, Y: torch.Tensor) -> torch.Tensor:
    """crossprod(A, Y) for a dense Y given as a (K, nrow) C-contiguous tensor,
    i.e. the column-major nrow x K matrix R would hand over.  Returns the
    (K, ncol) C-contiguous tensor that is the column-major ncol x K result."""
    K, nrow = Y.shape
    assert nrow == A.nrow and Y.is_contiguous()
    out = torch.zeros((K, A.ncol), dtype=torch.float64, device=Y.device)
    CrossprodPlan(A, K).run(Y, nrow, out)
    return out


def colstats_form(A: DeviceCSC, inner=1):
    """(form, nchunk) of colstats(A, ..., inner=inner) (svt_dev_colstats_form)."""
    return _hip.colstats_form(A.ncol // inner, A.nnz)


def rowstats_form(A: DeviceCSC, op: str, inner=1, na_background=False):
    """(form, panel_shift, nsplit) of one pass of rowstats(A, op, inner=inner) (svt_dev_rowstats_form)."""
    return _hip.rowstats_form(A.nrow, A.ncol, A.nnz, op, inner, na_background)


def colstats(A: DeviceCSC, op: str, na_rm=False, center=float("nan"), inner=1):
    oc = OPCODES[op]
    rt = _lib().svt_colStats_out_Rtype(oc, A.Rtype)
    nseg = A.ncol // inner
    out = torch.empty(nseg, dtype=torch.float64 if rt == REALSXP else torch.int32,
                      device=A.val.device)
    warn = torch.zeros(4, dtype=torch.int32, device=A.val.device)
    _check(_lib().svt_dev_colstats(A.handle, oc, int(na_rm), float(center), inner,
                                   out.data_ptr(), warn.data_ptr(), _stream()))
    return out, warn


def colmedians(A: DeviceCSC, na_rm=False, out=None, ws=None):
    """colMedians() of a resident 2-D operand (include/svt_hip.h, svt_dev_colmedians)."""
    if out is None:
        out = torch.empty(A.ncol, dtype=torch.float64, device=A.val.device)
    if ws is None:
        ws = torch.empty(_lib().svt_dev_colmedians_ws_bytes(A.nnz, A.ncol), dtype=torch.uint8,
                         device=A.val.device)
    _check(_lib().svt_dev_colmedians(A.handle, int(na_rm), out.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _stream()))
    return out


def colquantiles(A: DeviceCSC, probs, na_rm=False, out=None, ws=None):
    """colQuantiles(type = 7) of a resident 2-D operand (include/svt_hip.h, svt_dev_colquantiles).  ``probs``: a
    sequence, or a float64 tensor already on the device (every entry finite and in [0, 1]: checked here for a
    sequence, the caller's promise for a tensor).  Returns the (P, ncol) C-contiguous tensor that is the
    column-major ncol x P result."""
    dev = A.val.device
    if not isinstance(probs, torch.Tensor):
        p = np.asarray(probs, dtype=np.float64).reshape(-1)
        if not np.all((p >= 0.0) & (p <= 1.0)):
            raise SparseArrayError("'probs' outside [0,1]")
        probs = torch.as_tensor(p, device=dev)
    assert probs.dtype == torch.float64 and probs.is_cuda and probs.is_contiguous()
    P = int(probs.numel())
    if out is None:
        out = torch.empty((P, A.ncol), dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == P * A.ncol
    if ws is None:
        ws = torch.empty(_lib().svt_dev_colquantiles_ws_bytes(A.nnz, A.ncol, P), dtype=torch.uint8, device=dev)
    _check(_lib().svt_dev_colquantiles(A.handle, probs.data_ptr(), P, int(na_rm), out.data_ptr(), ws.data_ptr(),
                                       ws.numel(), _stream()))
    return out


def colmads(A: DeviceCSC, center=None, constant=1.4826, na_rm=False, out=None, ws=None):
    """colMads() of a resident 2-D operand (include/svt_hip.h, svt_dev_colmads).  ``center``: None for the column
    medians, or a float64 tensor of ncol entries already on the device."""
    dev = A.val.device
    if center is not None:
        assert center.dtype == torch.float64 and center.is_cuda and center.is_contiguous()
        if center.numel() != A.ncol:
            raise SparseArrayError("'center' must be NULL, a single number, or a vector with one element per column")
    if out is None:
        out = torch.empty(A.ncol, dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == A.ncol
    if ws is None:
        ws = torch.empty(_lib().svt_dev_colmads_ws_bytes(A.nnz, A.ncol), dtype=torch.uint8, device=dev)
    _check(_lib().svt_dev_colmads(A.handle, None if center is None else center.data_ptr(), float(constant), int(na_rm),
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return out


def colranks_form_limits():
    """(last stored length of form 0, last stored length of form 1) of svt_dev_colranks_form, found by bisection.
    Needs no GPU."""
    form = _hip.load_library().svt_dev_colranks_form

    def last(f):
        lo, hi = 0, 1 << 40                             # form(lo) <= f < form(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if form(mid) <= f else (lo, mid)
        return lo
    return last(0), last(1)


def colranks_long_nnz(A: DeviceCSC) -> int:
    """The stored values in the columns that svt_dev_colranks sorts in its workspace (form 2)."""
    lens = A.col_ptr[1:] - A.col_ptr[:-1]
    return int(lens[lens > colranks_form_limits()[1]].sum().item())


def colranks(A: DeviceCSC, ties_method="max", rank_nz=None, zero_rank=None, ws=None, flag=None):
    """colRanks() of a resident 2-D operand in the compact form (include/svt_hip.h, svt_dev_colranks): returns
    (rank_nz, zero_rank), one rank per stored value and one per column for its zeros, int32 tensors, or float64 ones
    for "average".  Without ``ws`` the workspace is sized from the column lengths (one read-back); a given one that was
    made for fewer long nonzeros than the operand holds raises.  ``flag``: a caller's int32 device word for that
    condition; it is then left to the caller to read, and the call stays asynchronous."""
    from .api import TIES_METHODS
    if ties_method not in TIES_METHODS:
        raise SparseArrayError("'ties.method' must be \"max\", \"average\", \"min\" or \"dense\"")
    dev = A.val.device
    dtype = torch.float64 if ties_method == "average" else torch.int32
    if rank_nz is None:
        rank_nz = torch.empty(A.nnz, dtype=dtype, device=dev)
    if zero_rank is None:
        zero_rank = torch.empty(A.ncol, dtype=dtype, device=dev)
    assert rank_nz.dtype == dtype and rank_nz.is_contiguous() and rank_nz.numel() == A.nnz
    assert zero_rank.dtype == dtype and zero_rank.is_contiguous() and zero_rank.numel() == A.ncol
    if ws is None:
        ws = torch.empty(_lib().svt_dev_colranks_ws_bytes(A.ncol, colranks_long_nnz(A)), dtype=torch.uint8, device=dev)
    own_flag = flag is None
    if own_flag:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    assert flag.dtype == torch.int32 and flag.is_cuda and flag.numel() == 1
    _check(_lib().svt_dev_colranks(A.handle, TIES_METHODS[ties_method], rank_nz.data_ptr(), zero_rank.data_ptr(),
                                   flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    if own_flag and int(flag.item()):
        raise SparseArrayError("svt_dev_colranks: the workspace was made for fewer long nonzeros than the operand holds")
    return rank_nz, zero_rank


def matmul_csc_csc(A: DeviceCSC, B: DeviceCSC, out=None, ws=None):
    """A %*% B for two resident sparse operands, B much sparser than a dense matrix (include/svt_hip.h,
    svt_dev_matmul_csc_csc).  Returns (out, not_finite): out is the (B.ncol, A.nrow) C-contiguous tensor that is
    the column-major A.nrow x B.ncol matrix; not_finite is a device int32 tensor, nonzero when a non-finite value
    or an NA took part -- the result then has to come from the dense route."""
    assert A.ncol == B.nrow
    dev = A.val.device
    if out is None:
        out = torch.empty((B.ncol, A.nrow), dtype=torch.float64, device=dev)
    if ws is None:
        ws = torch.empty(_lib().svt_dev_matmul_csc_csc_ws_bytes(A.handle), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(_lib().svt_dev_matmul_csc_csc(A.handle, B.handle, out.data_ptr(), A.nrow, ws.data_ptr(), ws.numel(),
                                         flag.data_ptr(), _stream()))
    return out, flag


def spgemm_panel(nrow: int) -> int:
    """Rows per panel of the sparse-result product for an operand of ``nrow`` rows (svt_dev_spgemm_panel).  Needs no
    GPU."""
    return int(_hip.load_library().svt_dev_spgemm_panel(int(nrow)))


def matmul_csc_csc_sparse(A: DeviceCSC, B: DeviceCSC, ws=None):
    """A %*% B for two resident sparse operands with a resident SPARSE result (include/svt_hip.h, svt_dev_spgemm; with
    ``ws``, a uint8 tensor of at least svt_dev_spgemm_ws_bytes() bytes, svt_dev_spgemm_count then _fill).  Every cell
    is the sum of its products in ascending order of the inner index, stored unless the sum == 0.  Returns
    (DeviceCSC of type double, not_finite): not_finite is a device int32 tensor, nonzero when a stored value of A or
    of B is not finite or an NA -- the result is complete under the rule, but its dense form may then differ from the
    reference's ``%*%``."""
    if not isinstance(A, DeviceCSC) or not isinstance(B, DeviceCSC):
        raise SparseArrayError("matmul_csc_csc_sparse() takes two DeviceCSC operands")
    lib, dev = _lib(), A.val.device
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if ws is None:
        return _composed(lambda *a: lib.svt_dev_spgemm(A.handle, B.handle, *a[:-1], flag.data_ptr(), a[-1]), dev, A.nrow, B.ncol,
                         REALSXP), flag
    return _two_calls(dev, A.nrow, B.ncol, torch.float64, False,
                      lambda *a: lib.svt_dev_spgemm_count(A.handle, B.handle, *a[:-1], flag.data_ptr(), a[-1]),
                      lambda cp, nnz, *a: lib.svt_dev_spgemm_fill(A.handle, B.handle, cp, *a), ws=ws), flag


def crossprod_csc_csc_sparse(X: DeviceCSC, Y: DeviceCSC = None):
    """crossprod(X, Y) = t(X) %*% Y with a resident sparse result (``Y`` None: the unary form, Y = X): ``X.t()`` on the
    device, then matmul_csc_csc_sparse.  Returns (DeviceCSC, not_finite)."""
    return matmul_csc_csc_sparse(X.t(), X if Y is None else Y)


def tcrossprod_csc_csc_sparse(X: DeviceCSC, Y: DeviceCSC = None):
    """tcrossprod(X, Y) = X %*% t(Y) with a resident sparse result (``Y`` None: Y = X).  Returns (DeviceCSC,
    not_finite)."""
    return matmul_csc_csc_sparse(X, (X if Y is None else Y).t())


def crossprod_csc_csc(Xt: DeviceCSC, Y: DeviceCSC, sym=False, out=None, ws=None):
    """crossprod(X, Y) of two resident sparse operands without a dense buffer (include/svt_hip.h,
    svt_dev_crossprod_csc_csc): ``Xt`` is t(X) (``X.t()``), ``sym`` says Y is X.  Returns (out, not_finite): out is the
    (ncol(Y), ncol(X)) C-contiguous tensor that is the column-major ncol(X) x ncol(Y) matrix; not_finite a device
    int32 tensor, nonzero when a non-finite value or an NA took part -- the result then has to come from the
    dense-buffer route."""
    assert Xt.ncol == Y.nrow
    dev = Y.val.device
    if out is None:
        out = torch.empty((Y.ncol, Xt.nrow), dtype=torch.float64, device=dev)
    if ws is None:
        ws = torch.empty(_lib().svt_dev_crossprod_csc_csc_ws_bytes(Xt.handle), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(_lib().svt_dev_crossprod_csc_csc(Xt.handle, Y.handle, int(bool(sym)), out.data_ptr(), Xt.nrow,
                                            ws.data_ptr(), ws.numel(), flag.data_ptr(), _stream()))
    return out, flag


def crossprod_csc_csc_dense_buffer(X: DeviceCSC, Y: DeviceCSC, out=None):
    """The dense-buffer route of crossprod(X, Y) on resident operands (svt_dev_crossprod_csc_csc_dense_buffer;
    ``Y is X``: the unary form).  Allocates and synchronises inside.  Returns the (ncol(Y), ncol(X)) C-contiguous
    tensor that is the column-major result."""
    if out is None:
        out = torch.empty((Y.ncol, X.ncol), dtype=torch.float64, device=Y.val.device)
    torch.cuda.synchronize()
    _check(_lib().svt_dev_crossprod_csc_csc_dense_buffer(X.handle, X.handle if Y is X else Y.handle, out.data_ptr()))
    return out


def set_sparse_crossprod_cost(factor=1.0) -> None:
    """Route choice of the host entry points crossprod(x) / crossprod(x, y) (svt_sparse_crossprod_set_cost):
    < 0 never the sparse-aware kernel, 0 always, 1 the measured model."""
    _lib().svt_sparse_crossprod_set_cost(float(factor))


def set_sparse_crossprod_panel(one_block_max=-1, log2_panel=-1) -> None:
    """Cell-panel shape of crossprod_csc_csc() (svt_dev_crossprod_csc_csc_set_panel); defaults restored by -1."""
    _lib().svt_dev_crossprod_csc_csc_set_panel(int(one_block_max), int(log2_panel))


class SpmmPlan:
    """What `A %*% B` (both sparse) needs from A alone -- the table of run bounds per row panel and the scan of
    its values -- done once (svt_dev_matmul_csc_csc_prepare), as `PbcPlan` does for crossprod(A, Y)."""

    def __init__(self, A: DeviceCSC):
        self.A = A
        self.ws = torch.empty(_lib().svt_dev_matmul_csc_csc_ws_bytes(A.handle), dtype=torch.uint8, device=A.val.device)
        _check(_lib().svt_dev_matmul_csc_csc_prepare(A.handle, self.ws.data_ptr(), self.ws.numel(), _stream()))

    def run(self, B: DeviceCSC, out=None):
        """Returns (out, not_finite) like matmul_csc_csc(); the flag tensor is this call's own."""
        A = self.A
        assert A.ncol == B.nrow
        if out is None:
            out = torch.empty((B.ncol, A.nrow), dtype=torch.float64, device=A.val.device)
        # (products are asynchronous: a flag tensor shared between runs would show a later product's verdict to
        # whoever reads an earlier one late)
        flag = torch.zeros(1, dtype=torch.int32, device=A.val.device)
        _check(_lib().svt_dev_matmul_csc_csc_prepared(A.handle, B.handle, out.data_ptr(), A.nrow, self.ws.data_ptr(),
                                                      self.ws.numel(), flag.data_ptr(), _stream()))
        return out, flag


def rowsums(A: DeviceCSC, na_rm=False, inner=1, out=None, ws=None):
    if out is None:
        out = torch.empty(inner * A.nrow, dtype=torch.float64, device=A.val.device)
    if ws is None:
        ws = torch.empty(_lib().svt_dev_rowstats_ws_bytes(A.nrow, A.ncol), dtype=torch.uint8,
                         device=A.val.device)
    _check(_lib().svt_dev_rowsums(A.handle, int(na_rm), inner, out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream()))
    return out


def rowstats(A: DeviceCSC, op: str, na_rm=False, center=None, inner=1, out=None, ws=None):
    """Any row statistic of a resident operand in one asynchronous call (include/svt_hip.h, svt_dev_rowstats): the
    six operations of C_rowStats_SVT plus "any", "all", "prod", "range", "mean", "var1" and "sd1".  ``center``: a
    float64 device tensor of inner * nrow elements ("centered_X2_sum", "var1", "sd1").  Returns (out, warn): ``out``
    has inner * nrow elements, float64 or int32 by the operation and the operand's type -- "range": 2 x (inner *
    nrow), the minima, then the maxima; ``warn`` is a device int32 tensor, nonzero when an integer min / max / range
    cell had no value."""
    oc = OPCODES[op]
    dev = A.val.device
    n = inner * A.nrow
    rt = _lib().svt_colStats_out_Rtype(oc, A.Rtype)
    dtype = torch.float64 if rt == REALSXP else torch.int32
    if out is None:
        out = torch.empty((2, n) if op == "range" else n, dtype=dtype, device=dev)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() == (2 * n if op == "range" else n)
    if ws is None:
        ws = torch.empty(_lib().svt_dev_rowstats_ws_bytes_op(A.handle, oc, inner), dtype=torch.uint8, device=dev)
    cptr = None
    if center is not None:
        assert center.dtype == torch.float64 and center.is_cuda and center.is_contiguous() and center.numel() == n
        cptr = center.data_ptr()
    warn = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(_lib().svt_dev_rowstats(A.handle, oc, int(na_rm), cptr, inner, out.data_ptr(), warn.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream()))
    return out, warn


class RowSumsPlan:
    """rowSums() of a resident operand with the table of run bounds built once (svt_dev_rowsums_prepare)."""

    def __init__(self, A: DeviceCSC, inner=1):
        self.A, self.inner = A, int(inner)
        self.ws = torch.empty(_lib().svt_dev_rowstats_ws_bytes(A.nrow, A.ncol), dtype=torch.uint8, device=A.val.device)
        _check(_lib().svt_dev_rowsums_prepare(A.handle, self.inner, self.ws.data_ptr(), self.ws.numel(), _stream()))

    def run(self, na_rm=False, out=None):
        A = self.A
        if out is None:
            out = torch.empty(self.inner * A.nrow, dtype=torch.float64, device=A.val.device)
        _check(_lib().svt_dev_rowsums_prepared(A.handle, int(na_rm), self.inner, out.data_ptr(), self.ws.data_ptr(),
                                               self.ws.numel(), _stream()))
        return out


def rowsum_form(A: DeviceCSC, ngroup: int):
    """(form, cols_per_wg, window_rows) of rowsum(A, group, ngroup) (svt_dev_rowsum_form)."""
    return _hip.rowsum_form(A.nrow, A.ncol, A.nnz, ngroup, "double" if A.Rtype == REALSXP else "integer")


def rowsum_prepare_form(A: DeviceCSC, ngroup: int):
    """(form, cols_per_wg) of the ids RowsumPlan(A, group, ngroup) prepares (svt_dev_rowsum_prepare_form)."""
    return _hip.rowsum_prepare_form(A.nrow, A.ncol, A.nnz, ngroup)


def rowsum_prepared_form(A: DeviceCSC, ngroup: int):
    """(supported, cols_per_wg) of RowsumPlan(A, group, ngroup).run() (svt_dev_rowsum_prepared_form)."""
    return _hip.rowsum_prepared_form(A.ncol, ngroup)


def rowsum(A: DeviceCSC, group: torch.Tensor, ngroup: int, na_rm=False, out=None):
    assert group.dtype == torch.int32 and group.numel() == A.nrow
    if out is None:
        out = torch.empty((A.ncol, ngroup), dtype=torch.float64, device=A.val.device)
    _check(_lib().svt_dev_rowsum(A.handle, group.data_ptr(), int(ngroup), int(na_rm),
                                 out.data_ptr(), _stream()))
    return out


class RowsumPlan:
    """rowsum(A, group) for a pair used more than once: the 16-bit group id of every nonzero is computed once
    (svt_dev_rowsum_prepare), a call then streams 10 bytes per nonzero and looks nothing up
    (svt_dev_rowsum_prepared; src/rowsum_methods.c:44-64 for the rules)."""

    def __init__(self, A: DeviceCSC, group: torch.Tensor, ngroup: int, gid=None):
        """``gid``: the caller's uint8 device buffer of at least svt_dev_rowsum_gid_bytes() bytes for the ids."""
        assert group.dtype == torch.int32 and group.numel() == A.nrow
        self.A, self.ngroup = A, int(ngroup)
        if gid is None:
            gid = torch.empty(_lib().svt_dev_rowsum_gid_bytes(A.handle), dtype=torch.uint8, device=A.val.device)
        assert gid.dtype == torch.uint8 and gid.is_contiguous() and gid.is_cuda
        self.gid = gid
        _check(_lib().svt_dev_rowsum_prepare(A.handle, group.data_ptr(), self.ngroup, self.gid.data_ptr(),
                                             self.gid.numel(), _stream()))

    def run(self, na_rm=False, out=None):
        """(ncol, ngroup) C-contiguous = the column-major ngroup x ncol result, like rowsum()."""
        A = self.A
        if out is None:
            out = torch.empty((A.ncol, self.ngroup), dtype=torch.float64, device=A.val.device)
        _check(_lib().svt_dev_rowsum_prepared(A.handle, self.gid.data_ptr(), self.ngroup, int(na_rm),
                                              out.data_ptr(), _stream()))
        return out
