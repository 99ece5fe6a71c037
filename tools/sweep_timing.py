"""Device-level timing of sweep(x, MARGIN, STATS, FUN) against its yardstick, in one run on one GPU.

Operand: BASELINE config 2, 1e6 x 1e4 at 1 % (1e8 nonzeros, doubles).  Four workloads, each a count call and a fill call:

    sweep(2, "/")    x / colSums(x) per column, the vector being the resident result of colstats(x, "sum")
    sweep(1, "*")    x * w with one weight per row (1e6 doubles: the gather is a random read into 8 MB)
    sweep(1, ">")    x > q with one threshold per row, a logical result
    scalar map       x / s, svt_dev_arith_map_count / _fill: the yardstick.  It moves the same bytes but for the row_idx
                     read of the count pass and the gather of the vector.  With --parent-lib it is also run on the library
                     of the parent commit, a child process per run, alternated with this build's.

A count call synchronises its stream once and is timed by the host clock around it (the stream is idle before); a fill
call is asynchronous and is timed by device events around CALLS calls.  Everything is warmed, then timed in turn, round
after round.  Reported: median / min / max over the rounds, the spread (max - min) / median and the ratio to the scalar
map's median.  Results are checked before anything is timed: the division against torch's own on the stored values, the
other two by their nonzero counts.

    python tools/sweep_timing.py [--out FILE] [--rounds 11] [--calls 5] [--parent-lib PATH]
                                 [--nrow 1000000 --ncol 10000 --density 0.01]

profiles/sweep_timing.txt holds one output of it.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsearray_amd import synth                                           # noqa: E402
from sparsearray_amd._abi import PROTOTYPES                                 # noqa: E402
from sparsearray_amd.svt import REALSXP                                     # noqa: E402

ARITH_SCALAR, MULT, DIV, GT = 1, 3, 4, 6
SCALAR = 3.0


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


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def row(label, call, t, ref=None):
    med = statistics.median(t)
    s = f"  {label:<34} {call:<6} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {(max(t) - min(t)) / med:7.2f}"
    return s + (f" {med / statistics.median(ref):7.2f}" if ref else "")


class Call:
    """one count / fill pair on its own buffers; ``count(*head, out_col_ptr, &nnz, *mid, ws, ws_bytes, stream)``"""

    def __init__(self, lib, X, label, count, fill, head, count_mid, fill_mid, need, out_dtype):
        dev = X.val.device
        self.lib, self.label, self.count_fn, self.fill_fn, self.head = lib, label, count, fill, head
        self.count_mid, self.fill_mid = count_mid, fill_mid
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.cp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.count()
        self.ri = torch.empty(self.nnz.value, dtype=torch.int32, device=dev)
        self.vv = torch.empty(self.nnz.value, dtype=out_dtype, device=dev)

    def count(self):
        rc = self.count_fn(*self.head, self.cp.data_ptr(), ctypes.byref(self.nnz), *self.count_mid, self.ws.data_ptr(),
                           self.ws.numel(), stream())
        assert rc == 0, self.lib.svt_last_error()

    def fill(self):
        rc = self.fill_fn(*self.head, self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(), *self.fill_mid,
                          self.ws.data_ptr(), self.ws.numel(), stream())
        assert rc == 0, self.lib.svt_last_error()


def scalar_map(lib, X, handle):
    return Call(lib, X, "scalar map x / s (yardstick)", lib.svt_dev_arith_map_count, lib.svt_dev_arith_map_fill,
                (handle, ARITH_SCALAR, DIV, SCALAR, REALSXP), (), (None,), lib.svt_dev_arith_map_ws_bytes(X.ncol, X.nnz), torch.float64)


class Operand:
    def __init__(self, nrow, cp, ri, v):
        self.nrow, self.ncol, self.nnz, self.col_ptr, self.row_idx, self.val = nrow, cp.numel() - 1, ri.numel(), cp, ri, v


# ---------------------------------------------------------------------------
# the child: the scalar map on the library at `path`, through ctypes alone (the parent's library lacks the new symbols)
# ---------------------------------------------------------------------------
def map_child(path, nrow, ncol, density, rounds, calls):
    lib = ctypes.CDLL(path)
    for name in ("svt_init", "svt_last_error", "svt_wrap_device_csc", "svt_dev_arith_map_ws_bytes", "svt_dev_arith_map_count",
                 "svt_dev_arith_map_fill"):
        f = getattr(lib, name)
        f.restype, f.argtypes = PROTOTYPES[name]
    assert lib.svt_init(0) == 0, lib.svt_last_error()
    dev = torch.device("cuda", 0)
    cp, ri, v = synth.random_device_csc(nrow, ncol, density, seed=7, device=dev)
    X = Operand(nrow, cp, ri, v)
    h = lib.svt_wrap_device_csc(REALSXP, nrow, ncol, X.nnz, cp.data_ptr(), ri.data_ptr(), v.data_ptr())
    m = scalar_map(lib, X, h)
    for _ in range(3):
        m.count()
        m.fill()
    torch.cuda.synchronize()
    check = [int(m.nnz.value), int(m.ri.to(torch.int64).sum().item()), int(m.vv.view(torch.int64).sum().item())]
    tc, tf = [], []
    for _ in range(rounds):
        tc.append(host_ms(m.count))
        tf.append(device_ms(m.fill, calls))
    print(json.dumps({"count": tc, "fill": tf, "check": check}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=1_000_000)
    ap.add_argument("--ncol", type=int, default=10_000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None, help="libsvt_hip.so of the parent commit, for the scalar map on both builds")
    ap.add_argument("--map-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.map_child:
        map_child(args.map_child, args.nrow, args.ncol, args.density, args.rounds, args.calls)
        return
    import sparsearray_amd.device as D
    from sparsearray_amd import _hip
    lib = _hip.init()
    dev = torch.device("cuda", 0)
    nrow, ncol = args.nrow, args.ncol
    cp, ri, v = synth.random_device_csc(nrow, ncol, args.density, seed=7, device=dev)
    X = D.DeviceCSC(nrow, cp, ri, v)
    sums, _ = D.colstats(X, "sum")                       # resident: it never leaves the device
    g = torch.Generator(device="cpu").manual_seed(11)
    weights = (torch.rand(nrow, generator=g, dtype=torch.float64) + 0.5).to(dev)
    q = torch.quantile(X.val[:1_000_000].abs(), 0.5).item()
    thresholds = (torch.rand(nrow, generator=g, dtype=torch.float64) * 2.0 * q).to(dev)
    need = lib.svt_dev_sweep_ws_bytes(ncol, X.nnz)

    def sweep(label, code, stats, form, compare):
        head = (X.handle, code, stats.data_ptr(), REALSXP, stats.numel(), *form)
        bad = ctypes.c_int64(-1)
        if compare:
            return Call(lib, X, label, lib.svt_dev_compare_sweep_count, lib.svt_dev_compare_sweep_fill, head, (ctypes.byref(bad),), (),
                        need, torch.int32)
        return Call(lib, X, label, lib.svt_dev_arith_sweep_count, lib.svt_dev_arith_sweep_fill, head, (ctypes.byref(bad),), (None,),
                    need, torch.float64)

    work = [sweep('sweep(2, "/") by resident colSums', DIV, sums, D.sweep_form((nrow, ncol), 2), False),
            sweep('sweep(1, "*") by row weights', MULT, weights, D.sweep_form((nrow, ncol), 1), False),
            sweep('sweep(1, ">") by row thresholds', GT, thresholds, D.sweep_form((nrow, ncol), 1), True),
            scalar_map(lib, X, X.handle)]
    for w in work:
        for _ in range(2):
            w.count(), w.fill()
    torch.cuda.synchronize()
    # the results, before anything is timed
    col_of = torch.repeat_interleave(torch.arange(ncol, device=dev), X.col_ptr[1:] - X.col_ptr[:-1])
    assert work[0].nnz.value == X.nnz and torch.equal(work[0].vv.view(torch.int64), (X.val / sums[col_of]).view(torch.int64))
    del col_of
    assert work[1].nnz.value == X.nnz and torch.equal(work[1].vv.view(torch.int64), (X.val * weights[X.row_idx.long()]).view(torch.int64))
    assert work[2].nnz.value == int((X.val > thresholds[X.row_idx.long()]).sum().item()) and bool((work[2].vv == 1).all())
    assert work[3].nnz.value == X.nnz
    T = {(w.label, k): [] for w in work for k in ("count", "fill")}
    for _ in range(args.rounds):
        for w in work:
            T[(w.label, "count")].append(host_ms(w.count))
            T[(w.label, "fill")].append(device_ms(w.fill, args.calls))
    ref = work[3].label
    lines = [f"sweep(x, MARGIN, STATS, FUN) against the scalar map, device level, ms ({torch.cuda.get_device_name(0)}).",
             f"operand {nrow} x {ncol} at {args.density:g}: {X.nnz} nonzeros, doubles.  {args.rounds} interleaved rounds; count: one "
             f"call by the host clock (it synchronises the stream once); fill: {args.calls} calls between two device events.",
             "spread = (max - min) / median; ratio = median / median of the scalar map on this build.", "",
             f"  {'workload':<34} {'call':<6} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'ratio':>7}"]
    for w in work:
        lines.append(f"{w.label}: result {w.nnz.value} nonzeros")
        lines.append(row("", "count", T[(w.label, "count")], T[(ref, "count")]))
        lines.append(row("", "fill", T[(w.label, "fill")], T[(ref, "fill")]))
        both = [a + b for a, b in zip(T[(w.label, "count")], T[(w.label, "fill")])]
        lines.append(row("", "both", both, [a + b for a, b in zip(T[(ref, "count")], T[(ref, "fill")])]))
    if args.parent_lib:
        from sparsearray_amd._hip import LIB_PATH
        del work, X, sums, weights, thresholds
        torch.cuda.empty_cache()
        runs = []
        for label, path in (("this build", LIB_PATH), ("parent", args.parent_lib), ("this build", LIB_PATH), ("parent", args.parent_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--map-child", os.path.abspath(path), "--nrow", str(nrow),
                                  "--ncol", str(ncol), "--density", str(args.density), "--rounds", str(args.rounds), "--calls",
                                  str(args.calls)], capture_output=True, text=True, check=True, timeout=300)
            runs.append((label, json.loads(out.stdout.strip().split("\n")[-1])))
        assert all(r["check"] == runs[0][1]["check"] for _, r in runs), "the two builds computed different results"
        lines.append("scalar map x / s on this build and on the parent commit's library, a process per run, alternated; the same "
                     "checksum of the result from all four:")
        for k, (label, r) in enumerate(runs):
            lines.append(row(f"  {label}, run {k // 2 + 1}", "count", r["count"]))
            lines.append(row(f"  {label}, run {k // 2 + 1}", "fill", r["fill"]))
        med = lambda k, key: statistics.median(runs[k][1][key])       # noqa: E731
        for key in ("count", "fill"):
            new, par = (med(0, key) + med(2, key)) / 2, (med(1, key) + med(3, key)) / 2
            lines.append(f"  {key}: this build / parent = {new / par:.3f}; parent run 2 / parent run 1 = {med(3, key) / med(1, key):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
