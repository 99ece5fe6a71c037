"""x[i, j] on the resident config-2 operand (1e6 x 1e4 at 1 %): the three routes of DeviceCSC.subset, and what the same
subset costs without them (download the three arrays, numpy, upload).

  columns   a random half of the columns, in random order            -> column gather
  rows      a random half of the rows, increasing                    -> row filter
  permute   a random permutation of the rows                         -> t(), column gather, t()

ms: a host clock around the whole call (allocations and its synchronisations included) ending in a device synchronise,
median / min / max over the rounds after warm-up.  GB/s: ALGORITHMIC bytes -- what any method must move, computed here
from the shapes -- over the median:
  columns   12 bytes read + 12 written per result entry, 12 bytes of subscript and pointers per result column
  rows      4 bytes (row index) read per operand entry, 8 read + 12 written per kept entry, 16 per column pointer pair
  permute   12 read + 12 written per entry
The host route is timed once per case (it takes seconds) and its result is compared with the device's, array for array.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sparsearray_amd import synth                                   # noqa: E402
from sparsearray_amd.device import DeviceCSC, subset_route_counts   # noqa: E402

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


def host_route(A, rows, cols):
    """D2H, numpy, H2D: (seconds, result arrays on the host)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cp, ri, v = A.col_ptr.cpu().numpy(), A.row_idx.cpu().numpy(), A.val.cpu().numpy()
    t1 = time.perf_counter()
    if cols is not None:
        lens = (cp[1:] - cp[:-1])[cols]
        ncp = np.zeros(cols.size + 1, dtype=np.int64)
        np.cumsum(lens, out=ncp[1:])
        src = np.repeat(cp[:-1][cols] - ncp[:-1], lens) + np.arange(ncp[-1])
        cp, ri, v = ncp, ri[src], v[src]
    if rows is not None:
        new = np.full(A.nrow, -1, dtype=np.int64)
        new[rows] = np.arange(rows.size)                         # (no repeats in these cases)
        nr = new[ri]
        keep = nr >= 0
        col = np.repeat(np.arange(cp.size - 1), cp[1:] - cp[:-1])[keep]
        nr, v = nr[keep], v[keep]
        if not np.all(np.diff(rows) > 0):
            order = np.argsort(col * rows.size + nr, kind="stable")
            nr, v = nr[order], v[order]
        ncp = np.zeros(cp.size, dtype=np.int64)
        np.cumsum(np.bincount(col, minlength=cp.size - 1), out=ncp[1:])
        cp, ri = ncp, nr.astype(np.int32)
    t2 = time.perf_counter()
    dev = A.val.device
    up = [torch.as_tensor(a, device=dev) for a in (cp, ri, v)]
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del up
    return (t1 - t0, t2 - t1, t3 - t2), (cp, ri, v)


def main():
    dev = torch.device("cuda", 0)
    nrow, ncol, dens = 1_000_000, 10_000, 0.01
    if len(sys.argv) > 3:
        nrow, ncol, dens = int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3])
    cp, ri, v = synth.random_device_csc(nrow, ncol, dens, seed=1, device=dev)
    A = DeviceCSC(nrow, cp, ri, v)
    rng = np.random.default_rng(2)
    cases = [
        ("columns", None, rng.permutation(ncol)[:ncol // 2].astype(np.int32)),
        ("rows", np.sort(rng.permutation(nrow)[:nrow // 2]).astype(np.int32), None),
        ("permute", rng.permutation(nrow).astype(np.int32), None),
    ]
    print(f"x[i, j] of a resident {nrow} x {ncol} operand at {dens}: {A.nnz} nonzeros, "
          f"{12 * A.nnz / 1e9:.2f} GB of entries; {ROUNDS} rounds after {WARM} warm-up calls, one MI355X")
    print(f"  {'case':8s} {'route counts (gather, filter, general)':40s} {'result nnz':>11s} {'median ms':>10s} {'min':>9s} "
          f"{'max':>9s} {'alg. GB':>8s} {'GB/s':>8s}   host route: D2H + numpy + H2D = s   same arrays")
    for name, rows, cols in cases:
        dr = None if rows is None else torch.as_tensor(rows, device=dev)
        dc = None if cols is None else torch.as_tensor(cols, device=dev)
        subset_route_counts(reset=True)
        R = A.subset(rows=dr, cols=dc)
        torch.cuda.synchronize()
        routes = tuple(subset_route_counts().values())
        if name == "columns":
            alg = 24 * R.nnz + 12 * R.ncol
        elif name == "rows":
            alg = 4 * A.nnz + 20 * R.nnz + 16 * A.ncol
        else:
            alg = 24 * A.nnz
        med, lo, hi = clock(lambda: A.subset(rows=dr, cols=dc), ROUNDS, WARM)
        (d2h, npy, h2d), want = host_route(A, rows, cols)
        got = (R.col_ptr.cpu().numpy(), R.row_idx.cpu().numpy(), R.val.cpu().numpy())
        same = all(np.array_equal(g, w) for g, w in zip(got, want))
        print(f"  {name:8s} {str(routes):40s} {R.nnz:11d} {med:10.3f} {lo:9.3f} {hi:9.3f} {alg / 1e9:8.3f} "
              f"{alg / med / 1e6:8.1f}   {d2h:.2f} + {npy:.2f} + {h2d:.2f} = {d2h + npy + h2d:.2f}   {same}")
        del R, got, want


if __name__ == "__main__":
    main()
