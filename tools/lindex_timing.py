"""Device-level timing of subsetting and subassignment by an L-index against their yardsticks, in one run on one GPU.

Operand: BASELINE config 2, 1e6 x 1e4 at 1 % (1e8 nonzeros, doubles).  The index is a sample of K of the stored cells
(what ``which(x > s)`` gives), sorted as nzwhich() leaves it, and the same cells shuffled.  Per K in (1e6, 1e7):

    gather         svt_dev_subset_lindex, sorted and shuffled
    placement      svt_dev_subassign_place_lindex_count (one or two synchronisations inside) and _fill, by both routes
    merge          svt_dev_assign_cells_merge_count / _fill of x and the placed Y
    Arith merge    svt_dev_arith_merge_count / _fill of x + Y for the SAME x and placed Y, in the same rounds: the same
                   kernel family on the same merged length nnz(x) + K.  ratio = merge / Arith merge
    composition    DeviceCSC.subassign_lindex, its allocations and synchronisations inside
    clamp chain    x.subassign_lindex(x.compare(">", s).nzwhich(), s) with s chosen so that about K entries exceed it

A count call synchronises its stream and is timed by the host clock around it (the stream is idle before); a fill or a
gather is asynchronous and is timed by device events around CALLS calls.  Everything is warmed, then timed in turn,
round after round.  Reported: median / min / max over the rounds and the spread (max - min) / median.  Results are
checked before anything is timed: the gather returns the values of the sampled entries, the two routes give the same
arrays.

Next to each time, the bytes the algorithm asks for, computed here from the shapes, and their rate as a share of the
8 TB/s HBM roofline (a whole-call rate over peak: launches and synchronisations are inside it):

    gather       per index: the index twice (check pass, gather) 16, the value 8, the result 8, and a binary search of
                 the leaf's rows, ceil(log2(mean leaf length)) probes of 4 bytes -- probes of one search share cache
                 lines at its end, so this counts requests, not lines
    placement    sorted route, per index: check 8 in, 12 out (key, position); fill 8 + 8 in, 12 out: 48.  Unsorted route:
                 that plus, per pass of the sort, 36 (svt_sort.h: the keys read twice, keys and positions read and
                 written once), plus 16 for the run-end flags and 32 for their scan
    merge        count and fill each read 12 per entry of x and of Y; the fill writes 12 per result entry

    python tools/lindex_timing.py [--out FILE] [--rounds 7] [--calls 3] [--nrow 1000000 --ncol 10000 --density 0.01]

profiles/lindex_timing.txt holds one output of it.
"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsearray_amd import synth                                           # noqa: E402
from sparsearray_amd.svt import REALSXP                                     # noqa: E402

ARITH_ADD = 1
PEAK = 8.0e12                                                               # bytes / s


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
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


def row(label, t, nbytes=None, ref=None):
    med = statistics.median(t)
    s = f"  {label:<44} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {(max(t) - min(t)) / med:7.2f}"
    if nbytes is not None:
        rate = nbytes / (med * 1e-3)
        s += f" {nbytes / 1e6:10.1f} {rate / 1e9:8.1f} {100.0 * rate / PEAK:6.2f}"
    else:
        s += " " * 27
    return s + (f" {med / statistics.median(ref):7.2f}" if ref else "")


HEADER = (f"  {'':<44} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'MB asked':>10} {'GB/s':>8} {'% peak':>6} {'ratio':>7}\n"
          f"  {'':<44} {'ms':>9} {'ms':>9} {'ms':>9}")


class Assign:
    """x[L] <- vals in its parts: the placement, the merge under the rule of the cells, the Arith merge of the same two
    operands"""

    def __init__(self, D, X, L, vals):
        lib, dev = D._lib(), X.val.device
        self.D, self.X, self.L, self.vals, self.K = D, X, L, vals, L.numel()
        self.pws = torch.empty(lib.svt_dev_subassign_place_lindex_ws_bytes(self.K, X.ncol), dtype=torch.uint8, device=dev)
        self.ycp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.got = ctypes.c_int64(0)
        self.what = (X.nrow, X.ncol, L.data_ptr(), self.K, 0, None, vals.data_ptr(), vals.numel(), REALSXP, self.ycp.data_ptr())
        self.place_count()
        self.y_nnz = self.got.value
        self.yri = torch.empty(self.y_nnz, dtype=torch.int32, device=dev)
        self.yv = torch.empty(self.y_nnz, dtype=torch.float64, device=dev)
        self.place_fill()
        self.Y = D.DeviceCSC(X.nrow, self.ycp, self.yri, self.yv)
        self.mws = torch.empty(lib.svt_dev_arith_merge_ws_bytes(X.ncol, X.nnz, self.y_nnz), dtype=torch.uint8, device=dev)
        self.ocp = torch.empty(X.ncol + 1, dtype=torch.int64, device=dev)
        self.merge_count()
        self.nnz = self.got.value
        self.ori = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.ov = torch.empty(self.nnz, dtype=torch.float64, device=dev)
        self.merge_fill()
        # the Arith merge in a workspace and a col_ptr of its own: its fill reads what ITS count left
        self.aws, self.acp = torch.empty_like(self.mws), torch.empty_like(self.ocp)
        self.arith_count()
        self.a_nnz = self.got.value
        self.ari = torch.empty(self.a_nnz, dtype=torch.int32, device=dev)
        self.av = torch.empty(self.a_nnz, dtype=torch.float64, device=dev)

    def _ok(self, rc):
        assert rc == 0, self.D._lib().svt_last_error()

    def place_count(self):
        self._ok(self.D._lib().svt_dev_subassign_place_lindex_count(*self.what, ctypes.byref(self.got), self.pws.data_ptr(),
                                                                    self.pws.numel(), stream()))

    def place_fill(self):
        self._ok(self.D._lib().svt_dev_subassign_place_lindex_fill(*self.what, self.y_nnz, self.yri.data_ptr(), self.yv.data_ptr(),
                                                                   self.pws.data_ptr(), self.pws.numel(), stream()))

    def merge_count(self):
        self._ok(self.D._lib().svt_dev_assign_cells_merge_count(self.X.handle, self.Y.handle, self.ocp.data_ptr(),
                                                                ctypes.byref(self.got), self.mws.data_ptr(), self.mws.numel(), stream()))

    def merge_fill(self):
        self._ok(self.D._lib().svt_dev_assign_cells_merge_fill(self.X.handle, self.Y.handle, self.ocp.data_ptr(), self.ori.data_ptr(),
                                                               self.ov.data_ptr(), self.mws.data_ptr(), self.mws.numel(), stream()))

    def arith_count(self):
        self._ok(self.D._lib().svt_dev_arith_merge_count(self.X.handle, self.Y.handle, ARITH_ADD, self.acp.data_ptr(),
                                                         ctypes.byref(self.got), self.aws.data_ptr(), self.aws.numel(), stream()))

    def arith_fill(self):
        self._ok(self.D._lib().svt_dev_arith_merge_fill(self.X.handle, self.Y.handle, ARITH_ADD, self.acp.data_ptr(), self.ari.data_ptr(),
                                                        self.av.data_ptr(), None, self.aws.data_ptr(), self.aws.numel(), stream()))

    def result(self):
        self.merge_count()
        self.merge_fill()
        torch.cuda.synchronize()
        return self.ocp.clone(), self.ori.clone(), self.ov.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--nrow", type=int, default=1000000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--K", type=int, nargs="+", default=[1000000, 10000000])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lindex_timing: no GPU; nothing here is measured without one")
    import sparsearray_amd.device as D
    lib = D._lib()
    dev = torch.device("cuda", 0)
    cp, ri, v = synth.random_device_csc(a.nrow, a.ncol, a.density, seed=7, device=dev)
    X = D.DeviceCSC(a.nrow, cp, ri, v)
    which = X.nzwhich()
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    passes = D.lindex_sort_passes(a.nrow, a.ncol)
    probes = max(1, math.ceil(math.log2(max(2.0, X.nnz / a.ncol))))
    lines = [f"lindex_timing: {a.nrow} x {a.ncol} at {a.density:g}: nnz(x) = {X.nnz}; rounds {a.rounds}, calls {a.calls}; "
             f"{torch.cuda.get_device_name(0)} ({lib.svt_device_arch().decode()})",
             f"sort passes for this array: {passes}; probes counted per lookup: {probes}", ""]
    for K in a.K:
        K = min(K, X.nnz)
        pick = torch.randperm(X.nnz, generator=g, device=dev)[:K].sort().values
        Ls = which[pick].contiguous()
        Lu = Ls[torch.randperm(K, generator=g, device=dev)].contiguous()
        vals_s = torch.rand(K, generator=g, device=dev, dtype=torch.float64) + 0.5
        vals_u = vals_s[torch.searchsorted(Ls, Lu)].contiguous()        # the same value for the same cell
        # checks first
        assert torch.equal(X.subset_lindex(Ls), X.val[pick])
        assert torch.equal(X.subset_lindex(Lu), X.val[pick][torch.searchsorted(Ls, Lu)])
        D.lindex_route_counts(reset=True)
        S, U = Assign(D, X, Ls, vals_s), Assign(D, X, Lu, vals_u)
        assert D.lindex_route_counts() == {"sorted": 1, "unsorted": 1} and S.y_nnz == U.y_nnz == K
        assert all(torch.equal(p, q) for p, q in zip(S.result(), U.result())), "the two routes differ"
        out = torch.empty(K, dtype=torch.float64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)

        def gather(L):
            assert lib.svt_dev_subset_lindex(X.handle, L.data_ptr(), K, out.data_ptr(), bad.data_ptr(), stream()) == 0
        work = {
            "gather, sorted": lambda: device_ms(lambda: gather(Ls), a.calls),
            "gather, shuffled": lambda: device_ms(lambda: gather(Lu), a.calls),
            "placement count, sorted route": lambda: host_ms(S.place_count),
            "placement fill,  sorted route": lambda: device_ms(S.place_fill, a.calls),
            "placement count, unsorted route": lambda: host_ms(U.place_count),
            "placement fill,  unsorted route": lambda: device_ms(U.place_fill, a.calls),
            "merge count (rule of the cells)": lambda: host_ms(S.merge_count),
            "merge fill  (rule of the cells)": lambda: device_ms(S.merge_fill, a.calls),
            "Arith merge count, same x and Y": lambda: host_ms(S.arith_count),
            "Arith merge fill,  same x and Y": lambda: device_ms(S.arith_fill, a.calls),
            "composition subassign_lindex, sorted": lambda: host_ms(lambda: X.subassign_lindex(Ls, vals_s)),
            "composition subassign_lindex, shuffled": lambda: host_ms(lambda: X.subassign_lindex(Lu, vals_u)),
        }
        for f in work.values():                             # warm
            f()
        t = {k: [] for k in work}
        for _ in range(a.rounds):
            for k, f in work.items():
                t[k].append(f())
        gb = K * (16 + 8 + 8 + 4 * probes)
        pc_s, pf = K * 20, K * 28
        pc_u = pc_s + K * (36 * passes + 16 + 32)
        mb = 12 * (X.nnz + K)
        lines += [f"K = {K}  (Y: {K} entries; merged length {X.nnz + K}; result {S.nnz} entries)", HEADER,
                  row("gather, sorted", t["gather, sorted"], gb), row("gather, shuffled", t["gather, shuffled"], gb),
                  row("placement count, sorted route", t["placement count, sorted route"], pc_s),
                  row("placement fill,  sorted route", t["placement fill,  sorted route"], pf),
                  row("placement count, unsorted route", t["placement count, unsorted route"], pc_u),
                  row("placement fill,  unsorted route", t["placement fill,  unsorted route"], pf + K * 12),
                  row("merge count (rule of the cells)", t["merge count (rule of the cells)"], mb, t["Arith merge count, same x and Y"]),
                  row("merge fill  (rule of the cells)", t["merge fill  (rule of the cells)"], mb + 12 * S.nnz,
                      t["Arith merge fill,  same x and Y"]),
                  row("Arith merge count, same x and Y", t["Arith merge count, same x and Y"], mb),
                  row("Arith merge fill,  same x and Y", t["Arith merge fill,  same x and Y"], mb + 12 * S.a_nnz),
                  row("composition subassign_lindex, sorted", t["composition subassign_lindex, sorted"]),
                  row("composition subassign_lindex, shuffled", t["composition subassign_lindex, shuffled"])]
        both = statistics.median(t["merge count (rule of the cells)"]) + statistics.median(t["merge fill  (rule of the cells)"])
        arith = statistics.median(t["Arith merge count, same x and Y"]) + statistics.median(t["Arith merge fill,  same x and Y"])
        extra = statistics.median(t["placement count, unsorted route"]) - statistics.median(t["placement count, sorted route"])
        per_pass = extra * 1e-3 / passes / K
        lines += [f"  merge count + fill over Arith merge count + fill on the same entries: {both / arith:.2f}",
                  f"  the sort: ({statistics.median(t['placement count, unsorted route']):.3f} - "
                  f"{statistics.median(t['placement count, sorted route']):.3f}) ms over {passes} passes (run-end flags, scan and "
                  f"the second synchronisation included) = {per_pass * 1e9:.3f} ns per pair per pass; at the expected 36 B per "
                  f"pair per pass that is {36 / per_pass / 1e9:.0f} GB/s, {100 * 36 / per_pass / PEAK:.1f} % of peak", ""]
        del S, U
        # the clamp chain: s = the value that about K entries exceed
        s = float(torch.quantile(X.val[:: max(1, X.nnz // 1000000)].float(), 1.0 - K / X.nnz))

        def chain():
            return X.subassign_lindex(X.compare(">", s).nzwhich(), s)
        R = chain()
        assert torch.equal(R.val, torch.clamp(X.val, max=s)) and torch.equal(R.row_idx, X.row_idx)
        n_over = int((X.val > s).sum())
        chain()
        tc = [host_ms(chain) for _ in range(a.rounds)]
        lines += [f"  clamp chain x[nzwhich(x > {s:g})] <- {s:g}: {n_over} entries capped", row("compare -> nzwhich -> subassign_lindex", tc), ""]
        del R
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
