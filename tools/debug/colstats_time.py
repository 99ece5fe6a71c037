"""Device-level colSums / colVars / colMins per launch form of launch_colstats (kernels_colstats.hip), for comparing two
builds of the library (same ABI) under this tree's Python.  Run on the GPU box, the two libraries in alternation.
  run   [--lib PATH] --label NAME --out FILE.json [--repeats 7] [--window 0.3]
        per (form, op): REPEATS windows of about WINDOW seconds of back-to-back calls between two device events, after
        a warm-up; milliseconds per call of each window
  table BASE_LABEL FILE.json ...
        per figure the base label's lowest .. highest window and the other labels' medians; "outside" marks a median
        that is not inside the base's range
Shapes: ~100 nonzeros per column (config 1 / config 5 leaves: 16 lanes), 400 (wavefront), 1e4 (config 2: workgroup,
register-cached), 3e4 (workgroup, streaming), 2 (a shattered operand: thread), and config 2's 1e8 nonzeros as one
segment (whole-array sum() / var(): split)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# form: (nrow, ncol, density, whole array as one segment)
SHAPES = [("lanes16", 20_000, 400_000, 0.005, False), ("wavefront", 100_000, 100_000, 0.004, False),
          ("workgroup_cached", 1_000_000, 10_000, 0.01, False), ("split", 1_000_000, 10_000, 0.01, True),
          ("workgroup_streaming", 1_000_000, 1_000, 0.03, False), ("thread", 8, 20_000_000, 0.25, False)]


def run(args):
    import torch
    from sparsearray_amd import _hip, synth
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    from sparsearray_amd import device
    dev = torch.device("cuda", 0)
    rows, A, built = [], None, None
    for form, nrow, ncol, density, whole in SHAPES:
        if built != (nrow, ncol, density):
            del A
            torch.cuda.empty_cache()
            A = device.DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, density, seed=11, device=dev))
            built = (nrow, ncol, density)
        inner = ncol if whole else 1
        assert device.colstats_form(A, inner)[0] == form, (form, device.colstats_form(A, inner))
        for op in ("sum", "var1") + (() if whole else ("min",)):
            call = lambda: device.colstats(A, op, inner=inner)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def window(n):
                e0.record()
                for _ in range(n):
                    call()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / n
            window(3)
            n = max(3, int(args.window * 1e3 / window(10)))
            ms = [window(n) for _ in range(args.repeats)]
            rows.append({"label": args.label, "form": form, "op": op, "nnz": A.nnz, "calls": n, "ms": ms})
            print(f"[{args.label}] {form:20s} {op:5s} {n:6d} calls/window  median {statistics.median(ms):9.4f} ms  "
                  f"{min(ms):9.4f} .. {max(ms):9.4f}", flush=True)
    with open(args.out, "w") as f:
        json.dump(rows, f)


def table(args):
    fig, labels = {}, [args.base]
    for p in args.files:
        for r in json.load(open(p)):
            fig.setdefault((r["form"], r["op"]), {}).setdefault(r["label"], []).extend(r["ms"])
            if r["label"] not in labels:
                labels.append(r["label"])
    print(f"{'form':20s} {'op':5s} {args.base + ' median':>16s} {'lowest .. highest':>24s} " +
          " ".join(f"{lb + ' median':>16s}" for lb in labels[1:]) + "   (ms per call)")
    for (form, op), by in fig.items():
        lo, hi = min(by[args.base]), max(by[args.base])
        cols = []
        for lb in labels[1:]:
            m = statistics.median(by[lb])
            cols.append(f"{m:16.4f}" + ("" if lo <= m <= hi else " outside, " + ("slower" if m > hi else "faster")))
        print(f"{form:20s} {op:5s} {statistics.median(by[args.base]):16.4f} {lo:11.4f} .. {hi:9.4f} " + " ".join(cols))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", default=None)
    r.add_argument("--label", default="this")
    r.add_argument("--out", required=True)
    r.add_argument("--repeats", type=int, default=7)
    r.add_argument("--window", type=float, default=0.3)
    t = sub.add_parser("table")
    t.add_argument("base")
    t.add_argument("files", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else table)(a)


if __name__ == "__main__":
    main()
