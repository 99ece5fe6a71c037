"""Row statistics in one call (svt_rowStatsFull_SVT / svt_dev_rowstats) at BASELINE config 2 (1e6 x 1e4 @ 1 %) and
config 5 (2e4 x 2e4 x 64 @ 0.5 %, dims = 2).  Run on the GPU box.

  run   --lib PATH --label NAME --out FILE.json [--configs 25] [--levels host,device] [--reps N]
        Host level: wall time of rowAnys (int operand), rowProds, rowVars(na_rm=True) and rowRanges through the Session
        of this tree over the library at PATH.  A library without svt_rowStatsFull_SVT (the parent commit's, built in
        a scratch checkout) takes the composed route of the R methods, which is what the parent's Session did.
        Device level: each added operation of svt_dev_rowstats next to svt_dev_rowsums on the same resident operand.
  table FILE.json ...     the rows of several runs side by side (profiles/rowstats_native_timing.txt)

A call whose composed route would rebuild more than 1e7 leaves on the host (aperm() of config 5: 4e8 leaves) is
not run on a library without the entry point; the table says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HOST_CALLS = [("rowAnys(int)", "rowAnys", "integer", {}), ("rowProds", "rowProds", "double", {}),
              ("rowVars(na_rm=TRUE)", "rowVars", "double", {"na_rm": True}), ("rowRanges", "rowRanges", "double", {})]
DEV_OPS = [("any", "integer"), ("all", "integer"), ("prod", "double"), ("range", "double"), ("mean", "double"),
           ("var1", "double"), ("sd1", "double")]
CONFIGS = {"2": ((1_000_000, 10_000), 0.01, 1, 7), "5": ((20_000, 20_000, 64), 0.005, 2, 5)}


def run(args):
    import numpy as np
    import torch
    from sparsearray_amd import SVT_SparseArray, _hip, synth
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    import sparsearray_amd
    from sparsearray_amd import device
    hip = sparsearray_amd.hip_session()
    native = hip._call.has_entry("C_rowStatsFull_SVT")
    dev = torch.device("cuda", 0)
    rows = []

    def note(config, level, call, ms, remark=""):
        rows.append({"label": args.label, "config": config, "level": level, "call": call, "ms": ms, "remark": remark})
        print(f"[{args.label}] config {config} {level:6s} {call:24s} "
              f"{'%10.3f ms' % ms if ms is not None else '   not run'} {remark}", flush=True)

    for c in args.configs:
        dim, density, dims, seed = CONFIGS[c]
        nleaves = int(np.prod(dim[1:]))
        cp, ri, v = synth.random_device_csc(dim[0], nleaves, density, seed=seed, device=dev)
        vi = (torch.arange(v.numel(), device=dev, dtype=torch.int32) % 19) + 1
        if "device" in args.levels and native:
            inner = int(np.prod(dim[1:dims]))
            for kind, val in (("integer", vi), ("double", v)):
                A = device.DeviceCSC(dim[0], cp, ri, val)
                n = inner * dim[0]
                sums = torch.empty(n, dtype=torch.float64, device=dev)
                ws0 = torch.empty(device._lib().svt_dev_rowstats_ws_bytes(A.nrow, A.ncol), dtype=torch.uint8, device=dev)

                def timed(f, reps):
                    for _ in range(2):
                        f()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        f()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / reps * 1e3
                reps = 20 if c == "2" else 5
                base = timed(lambda: device.rowsums(A, inner=inner, out=sums, ws=ws0), reps)
                note(c, "device", f"rowsums [{kind}]", base)
                for op, k in DEV_OPS:
                    if k != kind:
                        continue
                    oc = sparsearray_amd.api.OPCODES[op]
                    ws = torch.empty(device._lib().svt_dev_rowstats_ws_bytes_op(A.handle, oc, inner), dtype=torch.uint8,
                                     device=dev)
                    out, _ = device.rowstats(A, op, inner=inner, ws=ws)
                    for na_rm in ((False, True) if op == "var1" else (False,)):
                        ms = timed(lambda: device.rowstats(A, op, na_rm=na_rm, inner=inner, out=out, ws=ws), reps)
                        note(c, "device", f"{op}{' na_rm' if na_rm else ''}", ms, f"{ms / base:.2f} x rowsums")
                    del out, ws
                del A, sums, ws0
        if "host" in args.levels:
            hcp, hri = cp.cpu().numpy(), ri.cpu().numpy()
            xs = {"double": SVT_SparseArray.from_csc(dim, "double", hcp, hri, v.cpu().numpy()),
                  "integer": SVT_SparseArray.from_csc(dim, "integer", hcp, hri, vi.cpu().numpy())}
            for name, fn, kind, kw in HOST_CALLS:
                # leaves the composed route rebuilds on the host: those of aperm(x) / t(x)
                rebuilt = int(np.prod(dim[:-1])) if fn in ("rowAnys", "rowProds") else 0
                if not native and rebuilt > 10_000_000:
                    note(c, "host", name, None, f"composed route rebuilds {rebuilt:.1e} leaves of aperm(x) on the host")
                    continue
                best = None
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    getattr(hip, fn)(xs[kind], dims=dims, **kw)
                    ms = (time.perf_counter() - t0) * 1e3
                    best = ms if best is None else min(best, ms)
                note(c, "host", name, best, f"best of {args.reps}")
            del xs
        del cp, ri, v, vi
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)


def table(args):
    runs = [json.load(open(p)) for p in args.files]
    labels = []
    for r in runs:
        for row in r:
            if row["label"] not in labels:
                labels.append(row["label"])
    keys = []
    cell = {}
    for r in runs:
        for row in r:
            k = (row["config"], row["level"], row["call"])
            if k not in keys:
                keys.append(k)
            cell.setdefault(k, {})[row["label"]] = row
    print(f"{'config':6s} {'level':6s} {'call':24s} " + " ".join(f"{lb:>14s}" for lb in labels) + "  remarks")
    for k in keys:
        cols, remarks = [], []
        for lb in labels:
            row = cell[k].get(lb)
            cols.append(f"{'-':>14s}" if row is None else f"{'not run':>14s}" if row["ms"] is None else f"{row['ms']:11.3f} ms")
            if row is not None and row["remark"]:
                remarks.append(f"{lb}: {row['remark']}")
        print(f"{k[0]:6s} {k[1]:6s} {k[2]:24s} " + " ".join(cols) + "  " + "; ".join(remarks))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", default=None)
    r.add_argument("--label", default="this")
    r.add_argument("--out", required=True)
    r.add_argument("--configs", default="25", type=lambda s: [c for c in s if c in CONFIGS])
    r.add_argument("--levels", default="host,device", type=lambda s: s.split(","))
    r.add_argument("--reps", type=int, default=2)
    t = sub.add_parser("table")
    t.add_argument("files", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else table)(a)


if __name__ == "__main__":
    main()
