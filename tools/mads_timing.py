"""Device-level timing of colmads against colmedians on the same resident operand, in one process.

The two operands of tools/quantiles_timing.py: (a) BASELINE config 2, 1e6 x 1e4 at 1 % (every median is a zero and more
than half of every column is zeros: colmads answers every column from the median's counts, one walk of the values),
(b) 5e4 x 2000 at 60 % fill, positive values (every median is an order statistic of the stored values, and so is the
median of the deviations: both selects run on every column).  Workloads on each: colmedians, colmads, colmads with a
given center (the medians, computed beforehand: the deviations' two launches alone).  On operand b the median of the
deviations falls on the zeros' deviation |0 - c| (40 % of each column), which the counting pass knows; so a fourth
workload there: colmads on a variant with the values moved away from zero, |v| + 3, whose median is near 3.2 and whose
zeros have the largest deviation of all -- the median of the deviations is an order statistic of the stored values and
the second select runs on every column too.  Every workload is warmed, then the workloads are timed in turn, round after
round (interleaved, so that drift hits all of them alike): per round CALLS calls between two device events.  Reported
per workload: median / min / max of the per-call time over the rounds, the ratio of its median to the colmedians median
on the same operand, and the number of columns each select stage was left with (read from the per-column flags in the
workspace after a call; layout in include/svt_hip.h, svt_dev_colmads).  colmads with the medians given is compared
with colmads bit for bit before anything is timed.

    python tools/mads_timing.py [--out FILE] [--rounds 15] [--calls 50]

profiles/mads_timing.txt holds one output of it, next to the compiler's resource report of the kernels.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsearray_amd import _hip, synth                                    # noqa: E402
from sparsearray_amd.device import DeviceCSC, _lib, colmads, colmedians    # noqa: E402

OPERANDS = (
    ("a: 1e6 x 1e4 @ 1 % (config 2)", 1_000_000, 10_000, 0.01, False),
    ("b: 5e4 x 2000 @ 60 %, positive", 50_000, 2_000, 0.6, True),
)


def _undecided(ws, ncol, carve):
    """Columns left to the select launch by the counting launch number ``carve`` (0: the median's, 1: the
    deviations') of the last colmads call on ``ws``: three int64 arrays, then the int32 flags, 256-byte aligned."""
    p = ws.data_ptr()
    for _ in range(carve + 1):
        p = (p + 255) & ~255
        flags = p + 24 * ncol
        p = flags + 4 * ncol
    off = flags - ws.data_ptr()
    return int(ws[off:off + 4 * ncol].view(torch.int32).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    _hip.init()
    dev = torch.device("cuda", 0)
    lines = [f"colmads against colmedians, device level, ms per call ({torch.cuda.get_device_name(0)}).",
             f"{args.rounds} interleaved rounds of {args.calls} calls per workload between two device events, "
             "every workload warmed first;",
             "ratio = median / median of colmedians on the same operand; spread = (max - min) / median of colmedians;",
             "selected = columns left to the median's select / to the deviations' select.",
             ""]
    for name, nrow, ncol, dens, positive in OPERANDS:
        cp, ri, v = synth.random_device_csc(nrow, ncol, dens, seed=7, device=dev)
        operands = [("", DeviceCSC(nrow, cp, ri, v.abs() if positive else v))]
        if positive:
            operands.append((", values |v| + 3", DeviceCSC(nrow, cp, ri, v.abs() + 3.0)))
        A = operands[0][1]
        med_out = torch.empty(ncol, dtype=torch.float64, device=dev)
        med_ws = torch.empty(_lib().svt_dev_colmedians_ws_bytes(A.nnz, ncol), dtype=torch.uint8, device=dev)
        work = [("colmedians", lambda: colmedians(A, out=med_out, ws=med_ws), None)]
        same = []
        for suffix, B in operands:
            out = torch.empty(ncol, dtype=torch.float64, device=dev)
            ws = torch.zeros(_lib().svt_dev_colmads_ws_bytes(B.nnz, ncol), dtype=torch.uint8, device=dev)
            work.append(("colmads" + suffix, lambda B=B, out=out, ws=ws: colmads(B, out=out, ws=ws), ws))
            if not suffix:
                cen = colmedians(B).clone()
                out2 = torch.empty(ncol, dtype=torch.float64, device=dev)
                ws2 = torch.zeros(_lib().svt_dev_colmads_ws_bytes(B.nnz, ncol), dtype=torch.uint8, device=dev)
                work.append(("colmads, medians given", lambda B=B, cen=cen, out2=out2, ws2=ws2:
                             colmads(B, center=cen, out=out2, ws=ws2), ws2))
                same = [out, out2]
        for _, fn, _ in work:                           # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        identical = bool(torch.equal(same[0].view(torch.int64), same[1].view(torch.int64)))
        nonzero = int((med_out != 0).sum())
        selected = {}
        for label, fn, ws in work:
            if ws is not None:
                given = "given" in label
                selected[label] = ("-" if given else str(_undecided(ws, ncol, 0))) + " / " + str(_undecided(ws, ncol, 1))
        times = {label: [] for label, _, _ in work}
        for _ in range(args.rounds):
            for label, fn, _ in work:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[label].append(e0.elapsed_time(e1) / args.calls)
        base = statistics.median(times["colmedians"])
        spread = (max(times["colmedians"]) - min(times["colmedians"])) / base
        lines.append(f"operand {name}: {A.nnz} nonzeros, {nonzero} of {ncol} medians nonzero, colmads == colmads with "
                     f"the medians given, bit for bit: {identical}; colmedians spread {spread:.3f}")
        lines.append(f"  {'workload':<36} {'median':>8} {'min':>8} {'max':>8} {'ratio':>7} {'GNZ/s':>7}  selected")
        for label, _, _ in work:
            t = times[label]
            med = statistics.median(t)
            lines.append(f"  {label:<36} {med:8.4f} {min(t):8.4f} {max(t):8.4f} {med / base:7.3f} "
                         f"{A.nnz / med / 1e6:7.0f}  {selected.get(label, '')}")
        lines.append("")
        del A, operands, cp, ri, v, work, same
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
