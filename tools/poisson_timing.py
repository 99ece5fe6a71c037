"""Device-level timing of poissonSparseArray() on the device, in one process.

    1  svt_dev_poisson_count and svt_dev_poisson_fill, separately, for the 1e6 x 1e4 operand (1e10 cells) at density 0.01
       and 0.05, with the peak device memory of count + allocate + fill (workspace, col_ptr, row_idx, val).
    2  sparsearray_amd.synth.random_device_csc building an operand of the same size -- what the generator replaces in
       practice -- with its time and peak device memory.
    3  the two ways of sharing a Philox block between the two cells it serves, on the count pass of 999999 x 1e4 cells:
       first_leaf = 0 (an even first cell: a lane makes the block of two neighbouring cells, the ballots are dealt back
       into the mask words) against first_leaf = 1 (an odd first cell: every lane makes the block of its own cell).
    4  svt_dev_from_dense_count + _fill on the 1e6 x 128 array at 1 % of profiles/coerce_timing.txt, this library against
       another build of it (--parent-lib: the parent commit's libsvt_hip.so), interleaved round by round.

The count calls synchronise the stream once and are timed by the host clock around them (the stream is idle before); the
fill calls by device events.  Reported: median / min / max over the rounds and the spread (max - min) / median.

    python tools/poisson_timing.py [--out FILE] [--rounds 11] [--small] [--parent-lib PATH] [--synth-rounds 3]

profiles/poisson_timing.txt holds one output of it.
"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsearray_amd import synth                                          # noqa: E402
from sparsearray_amd._abi import PROTOTYPES                                # noqa: E402
from sparsearray_amd.device import _lib, _stream                           # noqa: E402
from sparsearray_amd.svt import REALSXP                                    # noqa: E402


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def row(name, ms, extra=""):
    med = statistics.median(ms)
    return f"    {name:<44s} {med:10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}   spread {(max(ms) - min(ms)) / med * 100:5.1f} %   {extra}"


class Poisson:
    """One window of a Poisson array and the preallocated outputs of its two calls"""

    def __init__(self, lib, nrow, total, lam, seed, first_leaf, nleaves, dev):
        self.lib, self.args = lib, (float(lam), seed, nrow, first_leaf, nleaves)
        self.ncells = nrow * nleaves
        self.ws = torch.empty(lib.svt_dev_poisson_ws_bytes(self.ncells), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(nleaves + 1, dtype=torch.int64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.count()
        self.ri = torch.empty(self.nnz.value, dtype=torch.int32, device=dev)
        self.vv = torch.empty(self.nnz.value, dtype=torch.int32, device=dev)
        self.fill()

    def count(self):
        rc = self.lib.svt_dev_poisson_count(*self.args, self.cp.data_ptr(), ctypes.byref(self.nnz), self.ws.data_ptr(),
                                            self.ws.numel(), _stream())
        assert rc == 0, self.lib.svt_last_error()

    def fill(self):
        rc = self.lib.svt_dev_poisson_fill(*self.args, self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, self.lib.svt_last_error()


class FromDense:
    """svt_dev_from_dense_count / _fill of one library on a dense array of doubles"""

    def __init__(self, lib, flat, nrow, ncol, dev):
        self.lib, self.args = lib, (flat.data_ptr(), REALSXP, nrow, ncol, REALSXP, 0)
        self.ws = torch.empty(lib.svt_dev_from_dense_ws_bytes(nrow * ncol), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(ncol + 1, dtype=torch.int64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.count()
        self.ri = torch.empty(self.nnz.value, dtype=torch.int32, device=dev)
        self.vv = torch.empty(self.nnz.value, dtype=torch.float64, device=dev)
        self.fill()

    def count(self):
        rc = self.lib.svt_dev_from_dense_count(*self.args, self.cp.data_ptr(), ctypes.byref(self.nnz), self.ws.data_ptr(),
                                               self.ws.numel(), _stream())
        assert rc == 0, self.lib.svt_last_error()

    def fill(self):
        rc = self.lib.svt_dev_from_dense_fill(*self.args, self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(),
                                              self.ws.data_ptr(), self.ws.numel(), _stream())
        assert rc == 0, self.lib.svt_last_error()


def other_library(path):
    lib = ctypes.CDLL(path)
    for name in ("svt_init", "svt_last_error", "svt_dev_from_dense_ws_bytes", "svt_dev_from_dense_count", "svt_dev_from_dense_fill"):
        f = getattr(lib, name)
        f.restype, f.argtypes = PROTOTYPES[name]
    assert lib.svt_init(0) == 0, lib.svt_last_error()
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--synth-rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="1e5 x 1e3 in place of 1e6 x 1e4: a check of the tool")
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    lib, dev = _lib(), torch.device("cuda")
    nrow, ncol = (100000, 1000) if a.small else (1000000, 10000)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"poissonSparseArray() on {lib.svt_device_arch().decode()}, {a.rounds} rounds")
    emit()

    emit(f"1  {nrow} x {ncol} ({nrow * ncol:.3g} cells), count and fill")
    for density in (0.01, 0.05):
        lam = -math.log(1.0 - density)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        P = Poisson(lib, nrow, ncol, lam, 1, 0, ncol, dev)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        tc, tf = [], []
        for _ in range(a.rounds):
            tc.append(host_ms(P.count))
            tf.append(device_ms(P.fill))
        nnz = P.nnz.value
        emit(f"  density {density}: lambda {lam:.6g}, {nnz} nonzeros ({nnz / P.ncells:.5f}), peak device memory {peak / 2 ** 30:.2f} GiB "
             f"(workspace {P.ws.numel() / 2 ** 30:.2f}, result {(P.cp.numel() * 8 + nnz * 8) / 2 ** 30:.2f})")
        emit(row("svt_dev_poisson_count", tc, f"{P.ncells / statistics.median(tc) / 1e6:.1f} Gcell/s"))
        emit(row("svt_dev_poisson_fill", tf, f"{P.ncells / statistics.median(tf) / 1e6:.1f} Gcell/s"))
        del P

    emit()
    emit(f"2  synth.random_device_csc({nrow}, {ncol}, density, seed), {a.synth_rounds} rounds")
    for density in (0.01, 0.05):
        ts, peak, nnz = [], 0, 0
        for r in range(a.synth_rounds):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            out = []
            ts.append(host_ms(lambda: out.append(synth.random_device_csc(nrow, ncol, density, seed=r + 1))))
            peak = max(peak, torch.cuda.max_memory_allocated())
            nnz = int(out[0][1].numel())
            del out
        emit(row(f"density {density}: {nnz} nonzeros", ts, f"peak device memory {peak / 2 ** 30:.2f} GiB"))

    emit()
    n2 = nrow - 1
    emit(f"3  the count pass of {n2} x {ncol} cells at density 0.05: one block per pair of cells against one per cell")
    lam = -math.log(0.95)
    even = Poisson(lib, n2, ncol + 1, lam, 1, 0, ncol, dev)
    odd = Poisson(lib, n2, ncol + 1, lam, 1, 1, ncol, dev)
    assert n2 % 2 == 1
    te, to = [], []
    for _ in range(a.rounds):
        te.append(host_ms(even.count))
        to.append(host_ms(odd.count))
    emit(row("first cell even: a block per pair, 4 ballots", te))
    emit(row("first cell odd: a block per cell, 1 ballot", to))
    del even, odd

    emit()
    emit("4  svt_dev_from_dense_count + _fill, 1000000 x 128 doubles at 1 %")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    fn, fc = (100000, 128) if a.small else (1000000, 128)
    flat = torch.rand(fn * fc, dtype=torch.float64, device=dev, generator=g)
    flat.mul_(flat < 0.01)
    libs = [("this library", FromDense(lib, flat, fn, fc, dev))]
    if a.parent_lib:
        libs.append(("the other build", FromDense(other_library(a.parent_lib), flat, fn, fc, dev)))
        assert torch.equal(libs[0][1].ri, libs[1][1].ri) and torch.equal(libs[0][1].vv, libs[1][1].vv)
    t = {(name, call): [] for name, _ in libs for call in ("count", "fill")}
    for _ in range(a.rounds):
        for name, F in libs:
            t[name, "count"].append(host_ms(F.count))
            t[name, "fill"].append(device_ms(F.fill))
    for name, _ in libs:
        emit(row(f"{name}: count", t[name, "count"]))
        emit(row(f"{name}: fill", t[name, "fill"]))
        emit(row(f"{name}: count + fill", [x + y for x, y in zip(t[name, "count"], t[name, "fill"])]))

    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
