"""Device-level timing of colquantiles against colmedians on the same resident operand, in one process.

Two operands: (a) BASELINE config 2, 1e6 x 1e4 at 1 % (every (column, prob) pair is decided by the counting pass),
(b) 5e4 x 2000 at 60 % fill, positive values (the median and the upper quantiles are order statistics of the stored
values: the per-column radix select runs).  Four workloads on each: colmedians, colquantiles with probs = (0.5),
with the default five probs, and with (0.25, 0.75).  Every workload is warmed, then the workloads are timed in turn,
round after round (interleaved, so that drift hits all of them alike): per round CALLS calls between two device
events.  Reported per workload: median / min / max of the per-call time over the rounds, and the ratio of its median
to the colmedians median; "spread" is (max - min) / median of colmedians, the run-to-run noise the ratios are read
against.  The colmedians result and the probs = (0.5) column are compared bit for bit before anything is timed.

    python tools/quantiles_timing.py [--out profiles/quantiles_timing.txt] [--rounds 15] [--calls 50]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsearray_amd import _hip, synth                                    # noqa: E402
from sparsearray_amd.device import DeviceCSC, _lib, colmedians, colquantiles    # noqa: E402

OPERANDS = (
    ("a: 1e6 x 1e4 @ 1 % (config 2)", 1_000_000, 10_000, 0.01, False),
    ("b: 5e4 x 2000 @ 60 %, positive", 50_000, 2_000, 0.6, True),
)
PROBS = (("colquantiles (0.5)", (0.5,)),
         ("colquantiles (0, .25, .5, .75, 1)", (0.0, 0.25, 0.5, 0.75, 1.0)),
         ("colquantiles (.25, .75)", (0.25, 0.75)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "quantiles_timing.txt"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    _hip.init()
    dev = torch.device("cuda", 0)
    lines = [f"colquantiles against colmedians, device level, ms per call ({torch.cuda.get_device_name(0)}).",
             f"{args.rounds} interleaved rounds of {args.calls} calls per workload between two device events, "
             "every workload warmed first;",
             "ratio = median / median of colmedians on the same operand; spread = (max - min) / median of colmedians.",
             ""]
    for name, nrow, ncol, dens, positive in OPERANDS:
        cp, ri, v = synth.random_device_csc(nrow, ncol, dens, seed=7, device=dev)
        if positive:
            v = v.abs()
        A = DeviceCSC(nrow, cp, ri, v)
        med_out = torch.empty(ncol, dtype=torch.float64, device=dev)
        med_ws = torch.empty(_lib().svt_dev_colmedians_ws_bytes(A.nnz, ncol), dtype=torch.uint8, device=dev)
        work = [("colmedians", lambda: colmedians(A, out=med_out, ws=med_ws))]
        for label, probs in PROBS:
            p = torch.tensor(probs, dtype=torch.float64, device=dev)
            out = torch.empty((len(probs), ncol), dtype=torch.float64, device=dev)
            ws = torch.empty(_lib().svt_dev_colquantiles_ws_bytes(A.nnz, ncol, len(probs)), dtype=torch.uint8,
                             device=dev)
            work.append((label, lambda p=p, out=out, ws=ws: colquantiles(A, p, out=out, ws=ws)))
        for _, fn in work:                              # warm-up; and the shared helpers give the same bits
            for _ in range(3):
                res = fn()
        torch.cuda.synchronize()
        half = work[1][1]()[0]
        same = bool(torch.equal(work[0][1]().view(torch.int64), half.view(torch.int64)))
        nonzero = int((half != 0).sum())
        times = {label: [] for label, _ in work}
        for _ in range(args.rounds):
            for label, fn in work:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[label].append(e0.elapsed_time(e1) / args.calls)
        base = statistics.median(times["colmedians"])
        spread = (max(times["colmedians"]) - min(times["colmedians"])) / base
        lines.append(f"operand {name}: {A.nnz} nonzeros, {nonzero} of {ncol} medians nonzero, "
                     f"colmedians == colquantiles(0.5) bit for bit: {same}; colmedians spread {spread:.3f}")
        lines.append(f"  {'workload':<36} {'median':>8} {'min':>8} {'max':>8} {'ratio':>7} {'GNZ/s':>7}")
        for label, _ in work:
            t = times[label]
            med = statistics.median(t)
            lines.append(f"  {label:<36} {med:8.4f} {min(t):8.4f} {max(t):8.4f} {med / base:7.3f} "
                         f"{A.nnz / med / 1e6:7.0f}")
        lines.append("")
        del A, cp, ri, v, work, res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
