"""Arith and Math on resident operands (DeviceCSC.arith / .math; kernels_arith.hip): x + y, x * y, x * s and log1p(x) on
the config-2 operand (1e6 x 1e4 at 1 %) and on the config-3 sparse operand (1e4 x 128 at 1 %); y is a second operand of
the same shape from another seed.

ms: a host clock around the whole call -- the count pass, its one synchronisation, the allocations from torch's
allocator, the fill pass -- ending in a device synchronise; median / min / max over the rounds after warm-up.
GB/s: ALGORITHMIC bytes, what the two passes must move, computed here from the shapes, over the median:
  merge  count pass: 12 bytes (row index, value) per operand entry and 16 per pair of column pointers; fill pass: the
         same 12 per operand entry again and 12 written per result entry; 8 per result column pointer
  map    count pass: 8 bytes (value) per operand entry and 8 per column pointer; fill pass: 12 per operand entry and 12
         written per result entry; 8 per result column pointer
The config-3 operand is 12 800 entries, 7 tiles: its rows measure the launches and the synchronisation, not bandwidth.
No threshold is attached to any of these numbers."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sparsearray_amd import synth                                   # noqa: E402
from sparsearray_amd.device import DeviceCSC, arith_tile            # noqa: E402

ROUNDS, WARM = 10, 3


def clock(f, rounds, warm):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    return float(np.median(ts)), min(ts), max(ts)


def main():
    dev = torch.device("cuda", 0)
    shapes = [("config-2", 1_000_000, 10_000, 0.01), ("config-3", 10_000, 128, 0.01)]
    if len(sys.argv) > 3:
        shapes = [("argv", int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]))]
    print(f"Arith / Math on resident operands, tiles of {arith_tile()} entries; {ROUNDS} rounds after {WARM} warm-up calls, "
          "one MI355X")
    print(f"  {'operand':9s} {'call':10s} {'operand nnz':>12s} {'result nnz':>11s} {'median ms':>10s} {'min':>9s} {'max':>9s} "
          f"{'alg. GB':>8s} {'GB/s':>8s}")
    for name, nrow, ncol, dens in shapes:
        x = DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, dens, seed=1, device=dev))
        y = DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, dens, seed=2, device=dev))
        calls = [("x + y", lambda: x.arith("+", y), True), ("x * y", lambda: x.arith("*", y), True),
                 ("x * s", lambda: x.arith("*", 2.0), False), ("log1p(x)", lambda: x.math("log1p"), False)]
        for what, f, merge in calls:
            R = f()
            torch.cuda.synchronize()
            if merge:
                entries = x.nnz + y.nnz
                alg = 24 * entries + 16 * ncol + 12 * R.nnz + 8 * ncol
            else:
                entries = x.nnz
                alg = 20 * entries + 8 * ncol + 12 * R.nnz + 8 * ncol
            rnnz = R.nnz
            del R
            med, lo, hi = clock(f, ROUNDS, WARM)
            print(f"  {name:9s} {what:10s} {entries:12d} {rnnz:11d} {med:10.3f} {lo:9.3f} {hi:9.3f} {alg / 1e9:8.3f} "
                  f"{alg / med / 1e6:8.1f}")
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
