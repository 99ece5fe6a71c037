"""Device-level timing of colranks (the compact form: a rank per stored value, a rank per column for its zeros) against
colmedians on the same resident operand, in one process.

Three operands, one per form of svt_dev_colranks_form: (a) BASELINE config 2, 1e6 x 1e4 at 1 % -- about 1e4 stored
values per column, every column sorted in LDS by one workgroup (form 1); (b) 1e4 x 2e5 at 1 % -- about 100 stored values
per column, a wavefront per column (form 0); (c) 5e4 x 2000 at 60 % fill -- 3e4 stored values per column, gathered and
sorted in the workspace (form 2).  Workloads on each: colmedians, colranks "max" (int32 ranks) and colranks "average"
(doubles).  Every workload is warmed, then the workloads are timed in turn, round after round (interleaved, so that
drift hits all of them alike): per round CALLS calls between two device events (an operand whose single call takes more
than 100 ms is timed with CALLS / 5 calls per round, and the report says so).  Reported per workload: median / min / max
of the per-call time over the rounds, the ratio of its median to the colmedians median on the same operand, and the
achieved bytes per second against the algorithmic bytes -- the value read and the rank written, 8 + 4 per nonzero for
"max" and 8 + 8 for "average" (4-byte values: 4 + 4 and 4 + 8).  The columns of each form are counted on the host from
col_ptr.

    python tools/ranks_timing.py [--out FILE] [--rounds 15] [--calls 50]

profiles/ranks_timing.txt holds one output of it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsearray_amd import _hip, synth                                    # noqa: E402
from sparsearray_amd.device import (DeviceCSC, _lib, colmedians, colranks, colranks_form_limits,   # noqa: E402
                                    colranks_long_nnz)

OPERANDS = (
    ("a: 1e6 x 1e4 @ 1 % (config 2)", 1_000_000, 10_000, 0.01),
    ("b: 1e4 x 2e5 @ 1 % (100 per column)", 10_000, 200_000, 0.01),
    ("c: 5e4 x 2000 @ 60 %", 50_000, 2_000, 0.6),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    _hip.init()
    dev = torch.device("cuda", 0)
    f0, f1 = colranks_form_limits()
    lines = [f"colranks against colmedians, device level, ms per call ({torch.cuda.get_device_name(0)}).",
             f"{args.rounds} interleaved rounds of {args.calls} calls per workload between two device events, "
             "every workload warmed first;",
             "ratio = median / median of colmedians on the same operand; GB/s = algorithmic bytes (value read + rank "
             "written per nonzero) / median;",
             f"forms: stored length <= {f0} form 0, <= {f1} form 1, longer form 2.",
             ""]
    for name, nrow, ncol, dens in OPERANDS:
        cp, ri, v = synth.random_device_csc(nrow, ncol, dens, seed=7, device=dev)
        A = DeviceCSC(nrow, cp, ri, v)
        lens = (cp[1:] - cp[:-1]).cpu()
        forms = [int((lens <= f0).sum()), int(((lens > f0) & (lens <= f1)).sum()), int((lens > f1).sum())]
        long_nnz = colranks_long_nnz(A)
        med_out = torch.empty(ncol, dtype=torch.float64, device=dev)
        med_ws = torch.empty(_lib().svt_dev_colmedians_ws_bytes(A.nnz, ncol), dtype=torch.uint8, device=dev)
        ws = torch.empty(_lib().svt_dev_colranks_ws_bytes(ncol, long_nnz), dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        work = [("colmedians", lambda: colmedians(A, out=med_out, ws=med_ws), 0)]
        for ties, dt, rb in (("max", torch.int32, 4), ("average", torch.float64, 8)):
            rn = torch.empty(A.nnz, dtype=dt, device=dev)
            rz = torch.empty(ncol, dtype=dt, device=dev)
            work.append((f"colranks {ties}", lambda ties=ties, rn=rn, rz=rz: colranks(A, ties, rank_nz=rn, zero_rank=rz, ws=ws,
                                                                                  flag=flag),
                         v.element_size() + rb))
        for _, fn, _ in work:                           # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert int(flag.item()) == 0                    # the workspace held the long columns
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work[1][1]()
        e1.record()
        e1.synchronize()
        calls = args.calls if e0.elapsed_time(e1) <= 100.0 else max(1, args.calls // 5)
        times = {label: [] for label, _, _ in work}
        for _ in range(args.rounds):
            for label, fn, _ in work:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[label].append(e0.elapsed_time(e1) / calls)
        base = statistics.median(times["colmedians"])
        lines.append(f"operand {name}: {A.nnz} nonzeros; columns of form 0 / 1 / 2: {forms[0]} / {forms[1]} / {forms[2]}; "
                     f"{long_nnz} long nonzeros, workspace {ws.numel()} bytes; {calls} calls per round")
        lines.append(f"  {'workload':<20} {'median':>9} {'min':>9} {'max':>9} {'ratio':>8} {'GB/s':>8}")
        for label, _, nbytes in work:
            t = times[label]
            med = statistics.median(t)
            rate = f"{A.nnz * nbytes / med / 1e6:8.1f}" if nbytes else f"{'':>8}"
            lines.append(f"  {label:<20} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {med / base:8.2f} {rate}")
        lines.append("")
        del A, cp, ri, v, work, ws, rn, rz
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
