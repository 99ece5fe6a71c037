"""Device-level timing of cbind() / rbind() of two resident halves against the two nearest references, in one process.

Operand: BASELINE config 2, 1e6 x 1e4 at 1 % (1e8 nonzeros, doubles), split on the device into two column halves and into
two row halves (DeviceCSC.subset).  Workloads, all producing the bytes of the whole operand again:

    cbind          svt_dev_abind_count + svt_dev_abind_fill on the two column halves
    rbind          the same on the two row halves
    cbind / rbind, mixed   the first half with int32 values (its values * 100, truncated), the second half doubles: the
                   copy widens; the result has the bytes of a double operand
    gather         the column gather that produces the same operand, svt_dev_subset_cols_count + _fill with
                   cols = 0 .. ncol-1 (what DeviceCSC.subset(cols=arange(ncol)) runs): the nearest code of this library
    torch.cat      torch.cat of the halves' row_idx and of their val tensors into preallocated outputs: the floor for
                   moving those bytes (for the mixed pairs the int32 half is converted by a .to(float64) first, which
                   writes and reads one more array)

A count call synchronises its stream once and is timed by the host clock around it (the stream is idle before); a fill
call is asynchronous and is timed by device events around CALLS calls; torch.cat likewise.  Every workload is warmed,
then the workloads are timed in turn, round after round (interleaved, so that drift hits all of them alike).  Reported:
median / min / max over the rounds, the spread (max - min) / median, the ratio of the fill's median to the gather fill's
median, and the achieved bytes per second of the fills -- algorithmic bytes: (4 + element size) per nonzero read and (4 +
8) written, plus the column pointers read (8 per leaf of every source, of the result too for the fills that search it).
The results of the abind calls are compared with the operand's own arrays, bit for bit, before anything is timed.

    python tools/abind_timing.py [--out FILE] [--rounds 15] [--calls 10] [--nrow 1000000 --ncol 10000 --density 0.01]

profiles/abind_timing.txt holds one output of it.
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


class Abind:
    """svt_dev_abind_count / _fill of ``objs`` into preallocated arrays"""

    def __init__(self, objs, along, nnz, nleaves):
        dev = objs[0].val.device
        self.objs, self.n = objs, len(objs)
        self.handles = (ctypes.c_void_p * self.n)(*[o._h for o in objs])
        self.ext = None if along == 1 else (ctypes.c_int64 * self.n)(*[o.ncol for o in objs])
        self.ws = torch.empty(_lib().svt_dev_abind_ws_bytes(self.n, nleaves, int(along == 1)), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(nleaves + 1, dtype=torch.int64, device=dev)
        self.ri = torch.empty(nnz, dtype=torch.int32, device=dev)
        self.vv = torch.empty(nnz, dtype=torch.float64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.read = sum(o.nnz * (4 + o.val.element_size()) + 8 * (o.ncol + 1) for o in objs)

    def count(self):
        rc = _lib().svt_dev_abind_count(self.handles, self.n, 1, self.ext, REALSXP, self.cp.data_ptr(), ctypes.byref(self.nnz),
                                        self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill(self):
        rc = _lib().svt_dev_abind_fill(self.handles, self.n, 1, self.ext, REALSXP, self.cp.data_ptr(), self.ri.data_ptr(),
                                       self.vv.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill_bytes(self):
        return self.read + self.ri.numel() * 12 + 8 * self.cp.numel()


class Gather:
    """svt_dev_subset_cols_count / _fill of the whole operand with cols = 0 .. ncol-1"""

    def __init__(self, A):
        dev = A.val.device
        self.A = A
        self.cols = torch.arange(A.ncol, dtype=torch.int32, device=dev)
        self.ws = torch.empty(_lib().svt_dev_subset_cols_ws_bytes(A.ncol), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(A.ncol + 1, dtype=torch.int64, device=dev)
        self.ri = torch.empty(A.nnz, dtype=torch.int32, device=dev)
        self.vv = torch.empty(A.nnz, dtype=torch.float64, device=dev)
        self.nnz = ctypes.c_int64(0)

    def count(self):
        rc = _lib().svt_dev_subset_cols_count(self.A.handle, self.cols.data_ptr(), self.A.ncol, self.cp.data_ptr(),
                                              ctypes.byref(self.nnz), self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill(self):
        rc = _lib().svt_dev_subset_cols_fill(self.A.handle, self.cols.data_ptr(), self.A.ncol, self.cp.data_ptr(),
                                             self.ri.data_ptr(), self.vv.data_ptr(), _stream())
        assert rc == 0, _lib().svt_last_error()

    def fill_bytes(self):
        A = self.A
        return A.nnz * 12 + 8 * (A.ncol + 1) + 4 * A.ncol + A.nnz * 12 + 8 * (A.ncol + 1)


class Cat:
    def __init__(self, objs, nnz):
        dev = objs[0].val.device
        self.objs = objs
        self.ri = torch.empty(nnz, dtype=torch.int32, device=dev)
        self.vv = torch.empty(nnz, dtype=torch.float64, device=dev)
        self.extra = sum(o.nnz * 16 for o in objs if o.val.dtype != torch.float64)     # the converted copy: written, read
        self.read = sum(o.nnz * (4 + o.val.element_size()) for o in objs)

    def fill(self):
        torch.cat([o.row_idx for o in self.objs], out=self.ri)
        torch.cat([o.val if o.val.dtype == torch.float64 else o.val.to(torch.float64) for o in self.objs], out=self.vv)

    def fill_bytes(self):
        return self.read + self.extra + self.ri.numel() * 12


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                                # ends in the call's own stream synchronisation
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def as_int(A):
    return DeviceCSC(A.nrow, A.col_ptr, A.row_idx, (A.val * 100.0).to(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nrow", type=int, default=1_000_000)
    ap.add_argument("--ncol", type=int, default=10_000)
    ap.add_argument("--density", type=float, default=0.01)
    args = ap.parse_args()
    _hip.init()
    dev = torch.device("cuda", 0)
    nrow, ncol = args.nrow, args.ncol
    cp, ri, v = synth.random_device_csc(nrow, ncol, args.density, seed=7, device=dev)
    X = DeviceCSC(nrow, cp, ri, v)
    ar = lambda a, b: torch.arange(a, b, dtype=torch.int32, device=dev)       # noqa: E731
    left, right = X.subset(cols=ar(0, ncol // 2)), X.subset(cols=ar(ncol // 2, ncol))
    top, bottom = X.subset(rows=ar(0, nrow // 2)), X.subset(rows=ar(nrow // 2, nrow))
    work = [("cbind", Abind([left, right], 2, X.nnz, ncol)), ("rbind", Abind([top, bottom], 1, X.nnz, ncol)),
            ("cbind, int + double", Abind([as_int(left), right], 2, X.nnz, ncol)),
            ("rbind, int + double", Abind([as_int(top), bottom], 1, X.nnz, ncol)),
            ("gather", Gather(X)),
            ("torch.cat, column halves", Cat([left, right], X.nnz)), ("torch.cat, row halves", Cat([top, bottom], X.nnz)),
            ("torch.cat, int + double", Cat([as_int(left), right], X.nnz))]
    for label, w in work:                               # warm-up, and the results against the operand itself
        for _ in range(3):
            if hasattr(w, "count"):
                w.count()
            w.fill()
        torch.cuda.synchronize()
        if hasattr(w, "count"):
            assert w.nnz.value == X.nnz and torch.equal(w.cp, X.col_ptr) and torch.equal(w.ri, X.row_idx), label
        if label in ("cbind", "rbind", "gather"):
            assert torch.equal(w.vv.view(torch.int64), X.val.view(torch.int64)), label
    mixed = work[2][1].vv
    assert torch.equal(mixed[left.nnz:], X.val[left.nnz:]) and torch.equal(mixed[:left.nnz], (left.val * 100.0).to(torch.int32).to(torch.float64))
    counts = {label: [] for label, w in work if hasattr(w, "count")}
    fills = {label: [] for label, _ in work}
    for _ in range(args.rounds):
        for label, w in work:
            if hasattr(w, "count"):
                counts[label].append(host_ms(w.count))
            fills[label].append(device_ms(w.fill, args.calls))
    base = statistics.median(fills["gather"])
    lines = [f"cbind / rbind of two resident halves against the column gather and torch.cat, device level, ms "
             f"({torch.cuda.get_device_name(0)}).",
             f"operand {nrow} x {ncol} at {args.density:g}: {X.nnz} nonzeros, doubles; halves of {left.nnz} + {right.nnz} (columns) and "
             f"{top.nnz} + {bottom.nnz} (rows) nonzeros.",
             f"{args.rounds} interleaved rounds; count: one call by the host clock (it synchronises the stream once); fill: "
             f"{args.calls} calls between two device events;",
             "spread = (max - min) / median; ratio = median fill / median fill of the gather; GB/s = algorithmic bytes of the "
             "fill / median.",
             "",
             f"  {'workload':<26} {'call':<6} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'ratio':>7} {'GB/s':>8}"]
    for label, w in work:
        if label in counts:
            t = counts[label]
            med = statistics.median(t)
            lines.append(f"  {label:<26} {'count':<6} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {(max(t) - min(t)) / med:7.2f}")
        t = fills[label]
        med = statistics.median(t)
        lines.append(f"  {label:<26} {'fill':<6} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {(max(t) - min(t)) / med:7.2f} "
                     f"{med / base:7.2f} {w.fill_bytes() / med / 1e6:8.1f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
