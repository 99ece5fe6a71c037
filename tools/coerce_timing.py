"""Device-level timing of the coercions dense array <-> resident operand and of nzwhich against their nearest references,
in one process.

Workloads (doubles; the dense array is made on the device from a seed: a cell is kept with probability `density`):

    1e6 x 128 at 1 %, 10 % and 50 %   the size of the headline Y, in both directions
    1e6 x 1000 at 1 %                 8 GB of cells
    nzwhich of the 1e6 x 1e4 operand at 1 % (1e8 entries), linear indices and coordinates

Calls, per array:

    from_dense count     svt_dev_from_dense_count: the keep test over the cells, the scan, col_ptr; it synchronises the
                         stream once and is timed by the host clock around it (the stream is idle before)
    from_dense fill      svt_dev_from_dense_fill: ranks from the masks, rows and values of the kept cells
    to_dense             svt_dev_to_dense: every output cell written once from a tile built in LDS
    fill + scatter       the obvious alternative to it: a background fill of the whole array (Tensor.zero_) followed by a
                         scatter over the entries (Tensor.index_copy_ with the linear indices svt_dev_nzwhich made
                         beforehand, outside the timed region -- which favours the alternative)
    torch to_sparse_csc  torch's own sparsification of the same tensor (it synchronises; host clock)
    torch to_dense       torch's own densification of that sparse tensor
    torch.clone          a plain copy of the dense array: the floor for reading and writing it once

Asynchronous calls are timed by device events around CALLS calls.  Every workload is warmed and checked (the round trip
gives the array back, bit for bit; both densifications agree), then the calls are timed in turn, round after round
(interleaved, so that drift hits all of them alike).  Reported: median / min / max over the rounds, the spread (max - min)
/ median and GB/s from the ALGORITHMIC bytes, stated per call in the report:

    count            8 per cell read, 1 bit per cell written and read again, 8 per leaf written
    fill             1 bit per cell and 8 per kept cell read, 12 per kept cell written
    to_dense         8 per cell written, 12 per entry and 8 per leaf read
    fill + scatter   8 per cell written, then 16 per entry read and 8 per entry written
    to_sparse_csc    8 per cell read, 12 per kept cell and 8 per column written (whatever torch moves in between)
    torch to_dense   as to_dense
    clone            8 per cell read and 8 written
    nzwhich          4 per entry and 8 per leaf read; 8 per entry written (linear), 4 * ndim per entry written (coordinates)

    python tools/coerce_timing.py [--out FILE] [--rounds 15] [--calls 10] [--small]

profiles/coerce_timing.txt holds one output of it.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsearray_amd import _hip, synth                                    # noqa: E402
from sparsearray_amd.device import DeviceCSC, _lib, _stream                # noqa: E402
from sparsearray_amd.svt import REALSXP                                    # noqa: E402


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def dense_array(nrow, ncol, density, seed, dev):
    """flat float64[nrow * ncol], column-major: uniform values in (0, density) where kept, 0 elsewhere"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    d = torch.rand(nrow * ncol, dtype=torch.float64, device=dev, generator=g)
    d.mul_(d < density)
    return d


class Array:
    """One dense array and the preallocated outputs of every call on it"""

    def __init__(self, nrow, ncol, density, seed, dev, with_torch=True):
        self.nrow, self.ncol, self.n, self.density = nrow, ncol, nrow * ncol, density
        self.flat = dense_array(nrow, ncol, density, seed, dev)
        self.ws = torch.empty(_lib().svt_dev_from_dense_ws_bytes(self.n), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(ncol + 1, dtype=torch.int64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.count()
        nnz = self.nnz.value
        self.ri = torch.empty(nnz, dtype=torch.int32, device=dev)
        self.vv = torch.empty(nnz, dtype=torch.float64, device=dev)
        self.fill()
        self.X = DeviceCSC(nrow, self.cp, self.ri, self.vv)
        self.lin = self.X.nzwhich()
        self.out = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.out2 = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.view = self.flat.view(ncol, nrow).t()      # the nrow x ncol tensor torch sees
        self.sparse, self.torch_error = None, None
        if with_torch:
            try:
                self.sparse = self.view.to_sparse_csc()
            except Exception as e:                      # noqa: BLE001 (reported in the table)
                self.torch_error = f"{type(e).__name__}: {str(e).splitlines()[0][:90]}"

    def _args(self):
        return (self.flat.data_ptr(), REALSXP, self.nrow, self.ncol, REALSXP, 0)

    def count(self):
        rc = _lib().svt_dev_from_dense_count(*self._args(), self.cp.data_ptr(), ctypes.byref(self.nnz), self.ws.data_ptr(),
                                             self.ws.numel(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill(self):
        rc = _lib().svt_dev_from_dense_fill(*self._args(), self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(),
                                            self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def to_dense(self):
        rc = _lib().svt_dev_to_dense(self.X.handle, 0, REALSXP, self.out.data_ptr(), self.bad.data_ptr(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill_scatter(self):
        self.out2.zero_()
        self.out2.index_copy_(0, self.lin, self.vv)

    def to_sparse_csc(self):
        self.view.to_sparse_csc()

    def torch_to_dense(self):
        self.sparse.to_dense()

    def clone(self):
        self.flat.clone()

    def calls(self):
        n, nnz, nl = self.n, self.nnz.value, self.ncol
        rows = [("from_dense count", self.count, "host", 8 * n + 2 * (n // 8) + 8 * nl),
                ("from_dense fill", self.fill, "dev", n // 8 + 8 * nnz + 12 * nnz),
                ("to_dense", self.to_dense, "dev", 8 * n + 12 * nnz + 8 * nl),
                ("fill + scatter", self.fill_scatter, "dev", 8 * n + 24 * nnz)]
        if self.sparse is not None:
            rows += [("torch to_sparse_csc", self.to_sparse_csc, "host", 8 * n + 12 * nnz + 8 * nl),
                     ("torch to_dense", self.torch_to_dense, "dev", 8 * n + 12 * nnz + 8 * nl)]
        rows.append(("torch.clone", self.clone, "dev", 16 * n))
        return rows

    def check(self):
        self.count()
        self.fill()
        self.to_dense()
        self.fill_scatter()
        torch.cuda.synchronize()
        assert int(self.bad.item()) == 0
        assert torch.equal(self.out.view(torch.int64), self.flat.view(torch.int64)), "round trip"
        assert torch.equal(self.out2, self.out), "fill + scatter"
        if self.sparse is not None:
            assert self.sparse.values().numel() == self.nnz.value
            assert torch.equal(self.sparse.to_dense().t().contiguous().view(-1), self.flat), "torch round trip"


class Nzwhich:
    def __init__(self, nrow, ncol, density, dev):
        cp, ri, v = synth.random_device_csc(nrow, ncol, density, seed=7, device=dev)
        self.X = DeviceCSC(nrow, cp, ri, v)
        self.dim = (ctypes.c_int64 * 2)(nrow, ncol)
        self.lin = torch.empty(self.X.nnz, dtype=torch.int64, device=dev)
        self.coo = torch.empty(2 * self.X.nnz, dtype=torch.int32, device=dev)

    def linear(self):
        rc = _lib().svt_dev_nzwhich(self.X.handle, 2, self.dim, 0, self.lin.data_ptr(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def coordinates(self):
        rc = _lib().svt_dev_nzwhich(self.X.handle, 2, self.dim, 1, self.coo.data_ptr(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def calls(self):
        nnz, nl = self.X.nnz, self.X.ncol
        return [("nzwhich, linear", self.linear, "dev", 4 * nnz + 8 * nl + 8 * nnz),
                ("nzwhich, coordinates", self.coordinates, "dev", 4 * nnz + 8 * nl + 8 * nnz)]

    def check(self):
        self.linear()
        self.coordinates()
        torch.cuda.synchronize()
        X, nnz = self.X, self.X.nnz
        leaf = torch.repeat_interleave(torch.arange(X.ncol, device=X.val.device), X.col_ptr[1:] - X.col_ptr[:-1])
        assert torch.equal(self.lin, leaf * X.nrow + X.row_idx), "linear"
        assert torch.equal(self.coo[:nnz], X.row_idx) and torch.equal(self.coo[nnz:].to(torch.int64), leaf), "coordinates"


def measure(work, rounds, calls):
    """{label: [ms per round]} for the (label, fn, clock, bytes) rows of ``work``, interleaved"""
    for _, fn, _, _ in work:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _, _, _ in work}
    for _ in range(rounds):
        for label, fn, clock, _ in work:
            times[label].append(host_ms(fn) if clock == "host" else device_ms(fn, calls))
    return times


def table(title, work, times):
    lines = [title, f"  {'call':<22} {'clock':<5} {'median':>10} {'min':>10} {'max':>10} {'spread':>7} {'MB':>10} {'GB/s':>8}"]
    for label, _, clock, nbytes in work:
        t = times[label]
        med = statistics.median(t)
        lines.append(f"  {label:<22} {clock:<5} {med:10.4f} {min(t):10.4f} {max(t):10.4f} {(max(t) - min(t)) / med:7.2f} "
                     f"{nbytes / 1e6:10.1f} {nbytes / med / 1e6:8.1f}")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="a hundredth of every size: a rehearsal, not a measurement")
    args = ap.parse_args()
    _hip.init()
    dev = torch.device("cuda", 0)
    k = 100 if args.small else 1
    lines = [f"Coercions dense array <-> resident operand and nzwhich against torch and a plain copy, device level, ms "
             f"({torch.cuda.get_device_name(0)}).",
             f"{args.rounds} interleaved rounds; clock host: one call by the host clock around a stream that is idle before and "
             f"synchronised after; clock dev: {args.calls} calls between two device events;",
             "spread = (max - min) / median; MB = the algorithmic bytes of the call (tools/coerce_timing.py states them per "
             "call); GB/s = those bytes / median.", ""]
    for nrow, ncol, density in ((1_000_000 // k, 128, 0.01), (1_000_000 // k, 128, 0.10), (1_000_000 // k, 128, 0.50),
                                (1_000_000 // k, 1000, 0.01)):
        A = Array(nrow, ncol, density, seed=int(density * 100) + ncol, dev=dev)
        A.check()
        work = A.calls()
        times = measure(work, args.rounds, args.calls if ncol == 128 else max(1, args.calls // 3))
        title = f"{nrow} x {ncol} doubles at {density:g}: {A.n} cells, {A.nnz.value} kept"
        if A.torch_error:
            title += f" (torch to_sparse_csc failed: {A.torch_error})"
        lines += table(title, work, times)
        del A, work
        torch.cuda.empty_cache()
    N = Nzwhich(1_000_000 // k, 10_000, 0.01, dev)
    N.check()
    work = N.calls()
    lines += table(f"nzwhich of the {N.X.nrow} x {N.X.ncol} operand at 0.01: {N.X.nnz} entries, ndim = 2", work,
                   measure(work, args.rounds, args.calls))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
