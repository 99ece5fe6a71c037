"""Device-level timing of pmin() / pmax() and is.na() against their yardsticks, in one run on one GPU.

Operand: BASELINE config 2, 1e6 x 1e4 at 1 % (1e8 nonzeros, doubles); for the merge a second operand of the same shape, and
a second, independent pair.  Each workload is a count call and a fill call on its own buffers, or a chain of device
methods timed as a whole:

    merge         pmin(x, y) against x + y (svt_dev_arith_merge_count / _fill), the yardstick: the same tiles, the same
                  bytes read, at most as many written
    chain         the reference's .pminmax2 composed from the device methods: compare -> nzwhich -> x[L] -> x[L] <- v ->
                  is.na -> nzwhich -> x[L] -> x[L] <- v, on the host clock from the first call to a final synchronisation
    scalar map    pmin(x, s) against x / s (the yardstick of sweep_timing.py) and against the clamp chain
                  x[nzwhich(x > s)] <- s
    sweep         sweep(2, caps, "pmin") with caps the resident colQuantiles(x, 0.999) against sweep(2, "/") by the resident
                  colSums (probability 0.999, not 0.99: at 1 % density the 0.99 quantile of a column is its zero background)
    is.na         is.na(x) against compare(x, "!=", 0), both maps with a logical result
    regression    with --parent-lib: x + y and x / s on this build and on the library of the parent commit, a child process
                  per run, alternated

A count call synchronises its stream once and is timed by the host clock around it; a fill call is asynchronous and is
timed by device events around CALLS calls (tools/sweep_timing.py, whose helpers this imports).  Everything is warmed, then
timed in turn, round after round.  Reported: median / min / max, the spread (max - min) / median and the ratio to the
workload's yardstick.  Results are checked before anything is timed: pmin(x, y) against the chain's arrays bit for bit
(one checksum from both), pmin(x, s) against the clamp chain's arrays and torch.minimum, the sweep against torch.minimum
with the gathered caps, is.na and x != 0 by their counts.

    python tools/pminmax_timing.py [--out FILE] [--rounds 11] [--calls 5] [--parent-lib PATH]
                                   [--nrow 1000000 --ncol 10000 --density 0.01]

profiles/pminmax_timing.txt holds one output of it.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sweep_timing import Call, Operand, device_ms, host_ms, row, scalar_map          # noqa: E402
from sparsearray_amd import synth                                                    # noqa: E402
from sparsearray_amd._abi import PROTOTYPES                                          # noqa: E402
from sparsearray_amd.svt import REALSXP                                              # noqa: E402

ADD, DIV, NE, PMIN, IS_NA = 1, 4, 2, 1, 1
SCALAR = 3.0


def checksum(cp, ri, vv):
    return [int(ri.numel()), int(cp.sum().item()), int(ri.to(torch.int64).sum().item()), int(vv.view(torch.int64).sum().item())]


def add_merge(lib, X, Y, hx, hy):
    return Call(lib, X, "x + y (yardstick)", lib.svt_dev_arith_merge_count, lib.svt_dev_arith_merge_fill, (hx, hy, ADD), (), (None,),
                lib.svt_dev_arith_merge_ws_bytes(X.ncol, X.nnz, Y.nnz), torch.float64)


# ---------------------------------------------------------------------------
# the child: x + y and x / s on the library at `path`, through ctypes alone (the parent's library lacks the new symbols)
# ---------------------------------------------------------------------------
def child(path, nrow, ncol, density, rounds, calls):
    lib = ctypes.CDLL(path)
    for name in ("svt_init", "svt_last_error", "svt_wrap_device_csc", "svt_dev_arith_map_ws_bytes", "svt_dev_arith_map_count",
                 "svt_dev_arith_map_fill", "svt_dev_arith_merge_ws_bytes", "svt_dev_arith_merge_count", "svt_dev_arith_merge_fill"):
        f = getattr(lib, name)
        f.restype, f.argtypes = PROTOTYPES[name]
    assert lib.svt_init(0) == 0, lib.svt_last_error()
    dev = torch.device("cuda", 0)
    ops = []
    for seed in (7, 8):
        cp, ri, v = synth.random_device_csc(nrow, ncol, density, seed=seed, device=dev)
        X = Operand(nrow, cp, ri, v)
        ops.append((X, lib.svt_wrap_device_csc(REALSXP, nrow, ncol, X.nnz, cp.data_ptr(), ri.data_ptr(), v.data_ptr())))
    (X, hx), (Y, hy) = ops
    work = {"merge": add_merge(lib, X, Y, hx, hy), "map": scalar_map(lib, X, hx)}
    out = {}
    for key, w in work.items():
        for _ in range(3):
            w.count(), w.fill()
        torch.cuda.synchronize()
        out[key] = {"count": [], "fill": [], "check": checksum(w.cp, w.ri, w.vv)}
    for _ in range(rounds):
        for key, w in work.items():
            out[key]["count"].append(host_ms(w.count))
            out[key]["fill"].append(device_ms(w.fill, calls))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=1_000_000)
    ap.add_argument("--ncol", type=int, default=10_000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None, help="libsvt_hip.so of the parent commit, for x + y and x / s on both builds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.nrow, args.ncol, args.density, args.rounds, args.calls)
        return
    import sparsearray_amd.device as D
    from sparsearray_amd import _hip
    lib = _hip.init()
    dev = torch.device("cuda", 0)
    nrow, ncol = args.nrow, args.ncol
    lines = [f"pmin() / pmax() and is.na() against their yardsticks, device level, ms ({torch.cuda.get_device_name(0)}).",
             f"operands {nrow} x {ncol} at {args.density:g}, doubles; the merge's with one NaN per thousand entries.  {args.rounds} interleaved rounds; count: one call by the host "
             f"clock (it synchronises the stream once); fill: {args.calls} calls between two device events; a chain: its device "
             "methods by the host clock, from the first call to a final synchronisation.",
             "spread = (max - min) / median; ratio = median / median of the yardstick named in the block.", "",
             f"  {'workload':<34} {'call':<6} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'ratio':>7}"]

    def report(w, T, ref):
        lines.append(f"{w.label}: result {w.nnz.value} nonzeros")
        for k in ("count", "fill"):
            lines.append(row("", k, T[(w.label, k)], T[(ref.label, k)]))
        both = [a + b for a, b in zip(T[(w.label, "count")], T[(w.label, "fill")])]
        ref_both = [a + b for a, b in zip(T[(ref.label, "count")], T[(ref.label, "fill")])]
        lines.append(row("", "both", both, ref_both))
        return ref_both

    def timed(work, chains=()):
        T = {(w.label, k): [] for w in work for k in ("count", "fill")}
        C = {label: [] for label, _ in chains}
        for _ in range(args.rounds):
            for w in work:
                T[(w.label, "count")].append(host_ms(w.count))
                T[(w.label, "fill")].append(device_ms(w.fill, args.calls))
            for label, fn in chains:
                C[label].append(host_ms(lambda: (fn(), torch.cuda.synchronize())))
        return T, C

    def warm(work):
        for w in work:
            for _ in range(2):
                w.count(), w.fill()
        torch.cuda.synchronize()

    # ---- the merge, on two independent pairs ----
    for pair, (sx, sy) in enumerate(((7, 8), (17, 18))):
        X = D.DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, args.density, seed=sx, device=dev))
        Y = D.DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, args.density, seed=sy, device=dev))
        X.val[::1000] = float("nan")                    # one entry in a thousand is NaN: every step of the chain has work
        Y.val[::1000] = float("nan")
        need = lib.svt_dev_arith_merge_ws_bytes(ncol, X.nnz, Y.nnz)
        pmin = Call(lib, X, "pmin(x, y)", lib.svt_dev_pminmax_merge_count, lib.svt_dev_pminmax_merge_fill, (X.handle, Y.handle, PMIN),
                    (), (), need, torch.float64)
        add = add_merge(lib, X, Y, X.handle, Y.handle)

        def chain(X=X, Y=Y):
            replace_idx = Y.compare("<", X).nzwhich()
            ans = X.subassign_lindex(replace_idx, Y.subset_lindex(replace_idx))
            restore_idx = X.is_na().nzwhich()
            return ans.subassign_lindex(restore_idx, X.subset_lindex(restore_idx))

        warm([pmin, add])
        R = chain()
        torch.cuda.synchronize()
        one, eight = checksum(pmin.cp, pmin.ri, pmin.vv), checksum(R.col_ptr, R.row_idx, R.val)
        assert one == eight and torch.equal(pmin.vv.view(torch.int64), R.val.view(torch.int64)), "pmin(x, y) and the chain differ"
        del R
        T, C = timed([pmin, add], [("chain", chain)])
        lines.append(f"-- merge, pair {pair + 1} (seeds {sx}, {sy}: {X.nnz} + {Y.nnz} nonzeros); yardstick x + y; checksum of pmin(x, y) "
                     f"and of the chain's result {one}")
        add_both = report(pmin, T, add)
        report(add, T, add)
        lines.append("the eight-step chain: the same arrays")
        lines.append(row("", "all", C["chain"], add_both))
        med = lambda k: statistics.median(T[("pmin(x, y)", k)])                # noqa: E731
        lines.append(f"  chain / pmin(x, y) both = {statistics.median(C['chain']) / (med('count') + med('fill')):.2f}")
        del pmin, add, T, C, chain
        if pair == 0:
            del Y
        torch.cuda.empty_cache()
    del X, Y
    torch.cuda.empty_cache()

    # ---- the scalar map, the sweep and is.na on one operand ----
    X = D.DeviceCSC(nrow, *synth.random_device_csc(nrow, ncol, args.density, seed=7, device=dev))
    cap = torch.quantile(X.val[:1_000_000], 0.75).item()
    assert cap > 0
    need = lib.svt_dev_arith_map_ws_bytes(ncol, X.nnz)
    pmin_s = Call(lib, X, f"pmin(x, {cap:.4g})", lib.svt_dev_pminmax_map_count, lib.svt_dev_pminmax_map_fill, (X.handle, PMIN, cap, REALSXP),
                  (), (), need, torch.float64)
    yard = scalar_map(lib, X, X.handle)

    def clamp():
        return X.subassign_lindex(X.compare(">", cap).nzwhich(), cap)

    warm([pmin_s, yard])
    R = clamp()
    torch.cuda.synchronize()
    one = checksum(pmin_s.cp, pmin_s.ri, pmin_s.vv)
    assert one == checksum(R.col_ptr, R.row_idx, R.val), "pmin(x, s) and the clamp chain differ"
    assert torch.equal(pmin_s.vv, torch.minimum(X.val, torch.tensor(cap, dtype=torch.float64, device=dev)))
    del R
    T, C = timed([pmin_s, yard], [("clamp", clamp)])
    lines.append(f"-- scalar map ({X.nnz} nonzeros); yardstick x / s; checksum of pmin(x, s) and of the clamp chain's result {one}")
    yard_both = report(pmin_s, T, yard)
    report(yard, T, yard)
    lines.append("the clamp chain x[nzwhich(x > s)] <- s: the same arrays")
    lines.append(row("", "all", C["clamp"], yard_both))
    del pmin_s, T, C

    sums, _ = D.colstats(X, "sum")
    caps = D.colquantiles(X, [0.999])[0].contiguous()
    assert bool((caps >= 0).all())
    form, bad = D.sweep_form((nrow, ncol), 2), ctypes.c_int64(-1)
    sw_div = Call(lib, X, 'sweep(2, "/") by resident colSums', lib.svt_dev_arith_sweep_count, lib.svt_dev_arith_sweep_fill,
                  (X.handle, DIV, sums.data_ptr(), REALSXP, ncol, *form), (ctypes.byref(bad),), (None,), need, torch.float64)
    sw_pmin = Call(lib, X, 'sweep(2, caps, "pmin")', lib.svt_dev_pminmax_sweep_count, lib.svt_dev_pminmax_sweep_fill,
                   (X.handle, PMIN, caps.data_ptr(), REALSXP, ncol, *form), (ctypes.byref(bad),), (), need, torch.float64)
    warm([sw_pmin, sw_div])
    col_of = torch.repeat_interleave(torch.arange(ncol, device=dev), X.col_ptr[1:] - X.col_ptr[:-1])
    want = torch.minimum(X.val, caps[col_of])
    assert sw_pmin.nnz.value == int((want != 0).sum().item()) and torch.equal(sw_pmin.vv, want[want != 0])
    del col_of, want
    T, _ = timed([sw_pmin, sw_div])
    lines.append(f"-- sweep; yardstick sweep(2, \"/\"); caps = resident colQuantiles(x, 0.999), {int((caps > 0).sum().item())} of "
                 f"{ncol} positive")
    report(sw_pmin, T, sw_div)
    report(sw_div, T, sw_div)
    del sw_pmin, sw_div, T

    X.val[::1000] = float("nan")                        # one entry in a thousand is NaN
    is_na = Call(lib, X, "is.na(x)", lib.svt_dev_isfun_map_count, lib.svt_dev_isfun_map_fill, (X.handle, IS_NA), (), (), need, torch.int32)
    ne0 = Call(lib, X, "x != 0 (yardstick)", lib.svt_dev_compare_map_count, lib.svt_dev_compare_map_fill, (X.handle, NE, 0.0, REALSXP),
               (), (), need, torch.int32)
    warm([is_na, ne0])
    assert is_na.nnz.value == int(torch.isnan(X.val).sum().item()) and ne0.nnz.value == int((X.val != 0).sum().item())
    T, _ = timed([is_na, ne0])
    lines.append("-- is.na on the operand with one NaN per thousand entries; yardstick compare(x, \"!=\", 0), whose result "
                 "keeps every entry: the fills write 0.1 % and 100 % of the entries")
    report(is_na, T, ne0)
    report(ne0, T, ne0)

    if args.parent_lib:
        from sparsearray_amd._hip import LIB_PATH
        del is_na, ne0, yard, X, sums, caps, T
        torch.cuda.empty_cache()
        runs = []
        for label, path in (("this build", LIB_PATH), ("parent", args.parent_lib), ("this build", LIB_PATH), ("parent", args.parent_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path), "--nrow", str(nrow),
                                  "--ncol", str(ncol), "--density", str(args.density), "--rounds", str(args.rounds), "--calls",
                                  str(args.calls)], capture_output=True, text=True, check=True, timeout=900)
            runs.append((label, json.loads(out.stdout.strip().split("\n")[-1])))
        lines.append("-- regression: x + y and x / s on this build and on the parent commit's library, a process per run, alternated; "
                     "the same checksum of the result from all four")
        for key, name in (("merge", "x + y"), ("map", "x / s")):
            assert all(r[key]["check"] == runs[0][1][key]["check"] for _, r in runs), "the two builds computed different results"
            for k, (label, r) in enumerate(runs):
                lines.append(row(f"  {name}, {label}, run {k // 2 + 1}", "count", r[key]["count"]))
                lines.append(row(f"  {name}, {label}, run {k // 2 + 1}", "fill", r[key]["fill"]))
            med = lambda k, c: statistics.median(runs[k][1][key][c])       # noqa: E731
            for c in ("count", "fill"):
                new, par = (med(0, c) + med(2, c)) / 2, (med(1, c) + med(3, c)) / 2
                lines.append(f"  {name} {c}: this build / parent = {new / par:.3f}; parent run 2 / parent run 1 = {med(3, c) / med(1, c):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
