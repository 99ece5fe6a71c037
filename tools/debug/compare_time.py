"""Compare and Logic on resident operands (DeviceCSC.compare / .logic; the Compare and Logic rules of kernels_arith.hip):
x > 0, x != y and a & b with a = x > 0, b = y > 0, on the config-2 operand (1e6 x 1e4 at 1 %) and on the config-3 sparse
operand (1e4 x 128 at 1 %); y is a second operand of the same shape from another seed.  The operands and the clock are
those of tools/debug/arith_time.py.

ms: a host clock around the whole call -- the count pass, its one synchronisation, the allocations from torch's
allocator, the fill pass -- ending in a device synchronise; median / min / max over the rounds after warm-up.
GB/s: ALGORITHMIC bytes, what the two passes must move, computed here from the shapes, over the median.  An operand
value is 8 bytes for x and y (doubles) and 4 for a and b (logicals), `v` below; a result value is 4 bytes:
  merge  count pass: 4 + v bytes (row index, value) per operand entry and 16 per pair of column pointers; fill pass: the
         same 4 + v per operand entry again and 8 written per result entry; 8 per result column pointer
  map    count pass: v bytes (value) per operand entry and 8 per column pointer; fill pass: 4 + v per operand entry and 8
         written per result entry; 8 per result column pointer
The config-3 operand is 12 800 entries, 7 tiles: its rows measure the launches and the synchronisation, not bandwidth.
No threshold is attached to any of these numbers."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from arith_time import ROUNDS, WARM, clock                          # noqa: E402
from sparsearray_amd import synth                                   # noqa: E402
from sparsearray_amd.device import DeviceCSC, arith_tile            # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    shapes = [("config-2", 1_000_000, 10_000, 0.01), ("config-3", 10_000, 128, 0.01)]
    if len(sys.argv) > 3:
        shapes = [("argv", int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]))]
    print(f"Compare / Logic on resident operands, tiles of {arith_tile()} entries; {ROUNDS} rounds after {WARM} warm-up calls, "
          "one MI355X")
    print(f"  {'operand':9s} {'call':10s} {'operand nnz':>12s} {'result nnz':>11s} {'median ms':>10s} {'min':>9s} {'max':>9s} "
          f"{'alg. GB':>8s} {'GB/s':>8s}")
    for name, nrow, ncol, dens in shapes:
        x = DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, dens, seed=1, device=dev))
        y = DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, dens, seed=2, device=dev))
        a, b = x.compare(">", 0), y.compare(">", 0)
        calls = [("x > 0", lambda: x.compare(">", 0), x.nnz, 8, False), ("x != y", lambda: x.compare("!=", y), x.nnz + y.nnz, 8, True),
                 ("a & b", lambda: a.logic("&", b), a.nnz + b.nnz, 4, True)]
        for what, f, entries, v, merge in calls:
            R = f()
            torch.cuda.synchronize()
            if merge:
                alg = 2 * (4 + v) * entries + 16 * ncol + 8 * R.nnz + 8 * ncol
            else:
                alg = (v + 4 + v) * entries + 8 * ncol + 8 * R.nnz + 8 * ncol
            rnnz = R.nnz
            del R
            med, lo, hi = clock(f, ROUNDS, WARM)
            print(f"  {name:9s} {what:10s} {entries:12d} {rnnz:11d} {med:10.3f} {lo:9.3f} {hi:9.3f} {alg / 1e9:8.3f} "
                  f"{alg / med / 1e6:8.1f}")
        del x, y, a, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
