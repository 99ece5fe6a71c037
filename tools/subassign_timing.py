"""Device-level timing of subassignment x[i, j] <- value against its yardsticks, in one run on one GPU.

Operand: BASELINE config 2, 1e6 x 1e4 at 1 % (1e8 nonzeros, doubles).  Workloads:

    cols <- 0      x[, j] <- 0 for 1000 columns               (the filter: the placed operand Y is empty)
    rows <- 0      x[i, ] <- 0 for a 10 % sample of the rows  (the filter)
    block <- 1.5   x[i, j] <- 1.5 on a 1000 x 1000 block      (Y: 1e6 entries)
    put-back       x[, 1:5000] <- x[, 1:5000], the SVT form   (Y: half of x)

Per workload: the placement (svt_dev_subassign_place_*_count, _fill), the assign merge (svt_dev_assign_merge_count,
_fill) and the whole composition (DeviceCSC.subassign, its allocations and two synchronisations inside).  Yardsticks,
timed in the same rounds:

    Arith merge    svt_dev_arith_merge_count / _fill of x + Y for the SAME x and placed Y: the same kernel family on
                   the same merged length nnz(x) + nnz(Y).  ratio = assign merge / Arith merge; the assign rule adds two
                   byte loads per x entry and, for an x entry whose row is covered, a search for its column.
    row filter     svt_dev_subset_rows_count / _fill keeping the rows that `rows <- 0` leaves: it also streams nnz(x)
                   once per pass.
    parent         Arith x + y of two operands of the config (seeds 7 and 8) on this build and on the library of the
                   parent commit (--parent-lib), each run a child process of its own, alternated this build / parent /
                   this build / parent: two runs of each give the noise band.

A count call synchronises its stream once and is timed by the host clock around it (the stream is idle before); a fill
call is asynchronous and is timed by device events around CALLS calls.  Everything is warmed, then timed in turn, round
after round.  Reported: median / min / max over the rounds and the spread (max - min) / median.  Results are checked
before anything is timed: the cleared cells are gone and nothing else changed, the put-back gives x again bit for bit.

    python tools/subassign_timing.py [--out FILE] [--rounds 11] [--calls 5] [--parent-lib PATH]
                                     [--nrow 1000000 --ncol 10000 --density 0.01]

profiles/subassign_timing.txt holds one output of it.
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

ARITH_ADD = 1


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
    s = f"  {label:<30} {call:<6} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {(max(t) - min(t)) / med:7.2f}"
    return s + (f" {med / statistics.median(ref):7.2f}" if ref else "")


# ---------------------------------------------------------------------------
# the child: Arith x + y on the library at `path`, through ctypes alone (the parent's library lacks the new symbols)
# ---------------------------------------------------------------------------
def arith_child(path, nrow, ncol, density, rounds, calls):
    lib = ctypes.CDLL(path)
    for name in ("svt_init", "svt_last_error", "svt_wrap_device_csc", "svt_release", "svt_dev_arith_merge_ws_bytes",
                 "svt_dev_arith_merge_count", "svt_dev_arith_merge_fill"):
        f = getattr(lib, name)
        f.restype, f.argtypes = PROTOTYPES[name]
    assert lib.svt_init(0) == 0, lib.svt_last_error()
    dev = torch.device("cuda", 0)
    cp, ri, v = synth.random_device_csc(nrow, ncol, density, seed=7, device=dev)
    cp2, ri2, v2 = synth.random_device_csc(nrow, ncol, density, seed=8, device=dev)
    nnz, nnz2 = ri.numel(), ri2.numel()
    X = lib.svt_wrap_device_csc(REALSXP, nrow, ncol, nnz, cp.data_ptr(), ri.data_ptr(), v.data_ptr())
    Y = lib.svt_wrap_device_csc(REALSXP, nrow, ncol, nnz2, cp2.data_ptr(), ri2.data_ptr(), v2.data_ptr())
    need = lib.svt_dev_arith_merge_ws_bytes(ncol, nnz, nnz2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ocp = torch.empty(ncol + 1, dtype=torch.int64, device=dev)
    got = ctypes.c_int64(0)

    def count():
        assert lib.svt_dev_arith_merge_count(X, Y, ARITH_ADD, ocp.data_ptr(), ctypes.byref(got), ws.data_ptr(), need, stream()) == 0
    count()
    ori = torch.empty(got.value, dtype=torch.int32, device=dev)
    ov = torch.empty(got.value, dtype=torch.float64, device=dev)

    def fill():
        assert lib.svt_dev_arith_merge_fill(X, Y, ARITH_ADD, ocp.data_ptr(), ori.data_ptr(), ov.data_ptr(), None, ws.data_ptr(),
                                            need, stream()) == 0
    for _ in range(3):
        count()
        fill()
    torch.cuda.synchronize()
    # a checksum of the result, so that the two builds can be compared: they must compute the same
    check = [int(got.value), int(ocp[-1].item()), int(ori.to(torch.int64).sum().item()), int(ov.view(torch.int64).sum().item())]
    tc, tf = [], []
    for _ in range(rounds):
        tc.append(host_ms(count))
        tf.append(device_ms(fill, calls))
    print(json.dumps({"count": tc, "fill": tf, "check": check, "merged": nnz + nnz2}))


# ---------------------------------------------------------------------------
# the workloads
# ---------------------------------------------------------------------------
class Work:
    """one subassignment: its placement, its merge, the Arith merge of the same operands, the composition"""

    def __init__(self, D, X, label, rows, leaves, value):
        lib, dev = D._lib(), X.val.device
        self.D, self.X, self.label, self.rows, self.leaves, self.value = D, X, label, rows, leaves, value
        self.sub = [None if s is None else D._subscript(s, dev) for s in (rows, leaves)]
        self.idx = [a for s in self.sub for a in ((None, -1) if s is None else (s.data_ptr(), s.numel()))]
        if isinstance(value, D.DeviceCSC):
            self.what, self.pc, self.pf = (value.handle,), lib.svt_dev_subassign_place_svt_count, lib.svt_dev_subassign_place_svt_fill
        else:
            self.vals, rt = D._assign_values(value, dev)
            self.what = (self.vals.data_ptr(), self.vals.numel(), rt)
            self.pc, self.pf = lib.svt_dev_subassign_place_vector_count, lib.svt_dev_subassign_place_vector_fill
        self.pws = torch.empty(lib.svt_dev_subassign_place_ws_bytes(X.nrow, X.ncol), dtype=torch.uint8, device=dev)
        self.ycp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.tab = [None if s is None else torch.empty(n, dtype=torch.uint8, device=dev) for s, n in zip(self.sub, (X.nrow, X.ncol))]
        self.tp = [None if t is None else t.data_ptr() for t in self.tab]
        self.ynnz = ctypes.c_int64(0)
        self.place_count()
        n = self.ynnz.value
        self.yri = torch.empty(n, dtype=torch.int32, device=dev)
        self.yv = torch.empty(n, dtype=torch.float64, device=dev)
        self.place_fill()
        self.Y = D.DeviceCSC(X.nrow, self.ycp, self.yri, self.yv)
        self.mws = torch.empty(lib.svt_dev_arith_merge_ws_bytes(X.ncol, X.nnz, n), dtype=torch.uint8, device=dev)
        self.ocp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.onnz = ctypes.c_int64(0)
        self.arith_count()
        na = self.onnz.value
        self.merge_count()
        m = max(na, self.onnz.value)
        self.ori = torch.empty(m, dtype=torch.int32, device=dev)
        self.ov = torch.empty(m, dtype=torch.float64, device=dev)

    def _ok(self, rc):
        assert rc == 0, self.D._lib().svt_last_error()

    def place_count(self):
        X = self.X
        self._ok(self.pc(X.nrow, X.ncol, *self.idx, *self.what, self.ycp.data_ptr(), *self.tp, ctypes.byref(self.ynnz),
                         self.pws.data_ptr(), self.pws.numel(), stream()))

    def place_fill(self):
        X = self.X
        self._ok(self.pf(X.nrow, X.ncol, *self.idx, *self.what, self.ycp.data_ptr(), self.ynnz.value, self.yri.data_ptr(),
                         self.yv.data_ptr(), self.pws.data_ptr(), self.pws.numel(), stream()))

    def merge_count(self):
        self._ok(self.D._lib().svt_dev_assign_merge_count(self.X.handle, self.Y.handle, *self.tp, self.ocp.data_ptr(),
                                                          ctypes.byref(self.onnz), self.mws.data_ptr(), self.mws.numel(), stream()))

    def merge_fill(self):
        self._ok(self.D._lib().svt_dev_assign_merge_fill(self.X.handle, self.Y.handle, *self.tp, self.ocp.data_ptr(),
                                                         self.ori.data_ptr(), self.ov.data_ptr(), self.mws.data_ptr(),
                                                         self.mws.numel(), stream()))

    def arith_count(self):
        self._ok(self.D._lib().svt_dev_arith_merge_count(self.X.handle, self.Y.handle, ARITH_ADD, self.ocp.data_ptr(),
                                                         ctypes.byref(self.onnz), self.mws.data_ptr(), self.mws.numel(), stream()))

    def arith_fill(self):
        self._ok(self.D._lib().svt_dev_arith_merge_fill(self.X.handle, self.Y.handle, ARITH_ADD, self.ocp.data_ptr(),
                                                        self.ori.data_ptr(), self.ov.data_ptr(), None, self.mws.data_ptr(),
                                                        self.mws.numel(), stream()))

    def whole(self):
        self.R = self.X.subassign(self.rows, self.leaves, self.value)
        torch.cuda.synchronize()


class RowFilter:
    """svt_dev_subset_rows_count / _fill keeping ``keep`` (strictly increasing)"""

    def __init__(self, D, X, keep):
        lib, dev = D._lib(), X.val.device
        self.lib, self.X, self.keep = lib, X, keep
        self.ws = torch.empty(lib.svt_dev_subset_rows_ws_bytes(X.nrow, X.ncol, X.nnz), dtype=torch.uint8, device=dev)
        self.cp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.nnz = ctypes.c_int64(0)
        self.count()
        self.ri = torch.empty(self.nnz.value, dtype=torch.int32, device=dev)
        self.vv = torch.empty(self.nnz.value, dtype=torch.float64, device=dev)

    def count(self):
        assert self.lib.svt_dev_subset_rows_count(self.X.handle, self.keep.data_ptr(), self.keep.numel(), self.cp.data_ptr(),
                                                  ctypes.byref(self.nnz), self.ws.data_ptr(), self.ws.numel(), stream()) == 0

    def fill(self):
        assert self.lib.svt_dev_subset_rows_fill(self.X.handle, self.cp.data_ptr(), self.ri.data_ptr(), self.vv.data_ptr(),
                                                 self.ws.data_ptr(), self.ws.numel(), stream()) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=1_000_000)
    ap.add_argument("--ncol", type=int, default=10_000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None, help="libsvt_hip.so of the parent commit, for Arith x + y on both builds")
    ap.add_argument("--arith-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.arith_child:
        arith_child(args.arith_child, args.nrow, args.ncol, args.density, args.rounds, args.calls)
        return
    import sparsearray_amd.device as D
    from sparsearray_amd import _hip
    _hip.init()
    dev = torch.device("cuda", 0)
    nrow, ncol = args.nrow, args.ncol
    cp, ri, v = synth.random_device_csc(nrow, ncol, args.density, seed=7, device=dev)
    X = D.DeviceCSC(nrow, cp, ri, v)
    g = torch.Generator(device="cpu").manual_seed(11)
    nj, ni = min(1000, ncol), max(1, nrow // 10)
    cols = torch.randperm(ncol, generator=g)[:nj].sort().values.to(torch.int32).to(dev)
    perm = torch.randperm(nrow, generator=g)
    rows = perm[:ni].sort().values.to(torch.int32).to(dev)
    keep = perm[ni:].sort().values.to(torch.int32).to(dev)
    bi = perm[:min(1000, nrow)].sort().values.to(torch.int32).to(dev)
    half = torch.arange(0, ncol // 2, dtype=torch.int32, device=dev)
    V = X.subset(cols=half)
    work = [Work(D, X, "cols <- 0", None, cols, 0.0), Work(D, X, "rows <- 0", rows, None, 0.0),
            Work(D, X, "block <- 1.5", bi, cols, 1.5), Work(D, X, "put-back of x[, 1:5000]", None, half, V)]
    filt = RowFilter(D, X, keep)
    # the results, before anything is timed
    for w in work:
        for _ in range(2):
            w.place_count(), w.place_fill(), w.arith_count(), w.arith_fill(), w.merge_count(), w.merge_fill()
        w.whole()
        n = w.onnz.value
        assert w.R.nnz == n and torch.equal(w.R.col_ptr, w.ocp) and torch.equal(w.R.row_idx, w.ori[:n]) and \
            torch.equal(w.R.val.view(torch.int64), w.ov[:n].view(torch.int64)), w.label
    colmask = torch.zeros(ncol, dtype=torch.bool, device=dev)
    colmask[cols.long()] = True
    col_of = torch.repeat_interleave(torch.arange(ncol, device=dev), X.col_ptr[1:] - X.col_ptr[:-1])
    rowmask = torch.zeros(nrow, dtype=torch.bool, device=dev)
    rowmask[rows.long()] = True
    for w, gone in ((work[0], colmask[col_of]), (work[1], rowmask[X.row_idx.long()])):
        assert torch.equal(w.R.row_idx, X.row_idx[~gone]) and torch.equal(w.R.val.view(torch.int64), X.val[~gone].view(torch.int64))
    R = work[3].R
    assert torch.equal(R.col_ptr, X.col_ptr) and torch.equal(R.row_idx, X.row_idx) and \
        torch.equal(R.val.view(torch.int64), X.val.view(torch.int64))
    assert filt.nnz.value == work[1].R.nnz
    del col_of
    T = {(w.label, k): [] for w in work for k in ("pc", "pf", "mc", "mf", "ac", "af", "whole")}
    F = {"count": [], "fill": []}
    for _ in range(args.rounds):
        for w in work:
            T[(w.label, "pc")].append(host_ms(w.place_count))
            T[(w.label, "pf")].append(device_ms(w.place_fill, args.calls))
            T[(w.label, "ac")].append(host_ms(w.arith_count))
            T[(w.label, "af")].append(device_ms(w.arith_fill, args.calls))
            T[(w.label, "mc")].append(host_ms(w.merge_count))
            T[(w.label, "mf")].append(device_ms(w.merge_fill, args.calls))
            T[(w.label, "whole")].append(host_ms(w.whole))
        F["count"].append(host_ms(filt.count))
        F["fill"].append(device_ms(filt.fill, args.calls))
    lines = [f"Subassignment x[i, j] <- value against its yardsticks, device level, ms ({torch.cuda.get_device_name(0)}).",
             f"operand {nrow} x {ncol} at {args.density:g}: {X.nnz} nonzeros, doubles.  {args.rounds} interleaved rounds; count: one "
             f"call by the host clock (it synchronises the stream once); fill: {args.calls} calls between two device events; whole: "
             "DeviceCSC.subassign and a synchronisation, by the host clock.",
             "spread = (max - min) / median; ratio = median / median of the yardstick named in the row.", "",
             f"  {'workload':<30} {'call':<6} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'ratio':>7}"]
    for w in work:
        L = w.label
        lines.append(f"{L}: Y has {w.ynnz.value} entries, merged length {X.nnz + w.ynnz.value}, result {w.R.nnz} nonzeros")
        lines.append(row("  placement", "count", T[(L, "pc")]))
        lines.append(row("  placement", "fill", T[(L, "pf")]))
        lines.append(row("  Arith merge x + Y (yardstick)", "count", T[(L, "ac")]))
        lines.append(row("  Arith merge x + Y (yardstick)", "fill", T[(L, "af")]))
        lines.append(row("  assign merge / Arith merge", "count", T[(L, "mc")], T[(L, "ac")]))
        lines.append(row("  assign merge / Arith merge", "fill", T[(L, "mf")], T[(L, "af")]))
        lines.append(row("  DeviceCSC.subassign", "whole", T[(L, "whole")]))
    lines.append(f"row filter keeping the {keep.numel()} rows that `rows <- 0` leaves (svt_dev_subset_rows, yardstick of the filter case)")
    lines.append(row("  row filter", "count", F["count"]))
    lines.append(row("  row filter", "fill", F["fill"]))
    lines.append(row("  assign merge, rows <- 0 / filter", "count", T[("rows <- 0", "mc")], F["count"]))
    lines.append(row("  assign merge, rows <- 0 / filter", "fill", T[("rows <- 0", "mf")], F["fill"]))
    lines.append(row("  assign merge, cols <- 0 / filter", "count", T[("cols <- 0", "mc")], F["count"]))
    lines.append(row("  assign merge, cols <- 0 / filter", "fill", T[("cols <- 0", "mf")], F["fill"]))
    if args.parent_lib:
        from sparsearray_amd._hip import LIB_PATH
        del work, filt, V, R
        torch.cuda.empty_cache()
        runs = []
        for label, path in (("this build", LIB_PATH), ("parent", args.parent_lib), ("this build", LIB_PATH), ("parent", args.parent_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arith-child", os.path.abspath(path), "--nrow", str(nrow),
                                  "--ncol", str(ncol), "--density", str(args.density), "--rounds", str(args.rounds), "--calls",
                                  str(args.calls)], capture_output=True, text=True, check=True, timeout=300)
            runs.append((label, json.loads(out.stdout.strip().split("\n")[-1])))
        assert all(r["check"] == runs[0][1]["check"] for _, r in runs), "the two builds computed different results"
        lines.append(f"Arith x + y, two operands of the config (merged length {runs[0][1]['merged']}), a process per run, alternated; "
                     "the same checksum of the result from all four:")
        for k, (label, r) in enumerate(runs):
            lines.append(row(f"  {label}, run {k // 2 + 1}", "count", r["count"]))
            lines.append(row(f"  {label}, run {k // 2 + 1}", "fill", r["fill"]))
        med = lambda k, key: statistics.median(runs[k][1][key])       # noqa: E731
        for key in ("count", "fill"):
            new, par = (med(0, key) + med(2, key)) / 2, (med(1, key) + med(3, key)) / 2
            lines.append(f"  {key}: this build / parent = {new / par:.3f}; parent run 2 / parent run 1 = {med(3, key) / med(1, key):.3f}; "
                         f"this build run 2 / run 1 = {med(2, key) / med(0, key):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
