"""Device-level timing of the sparse x sparse product with a sparse result (svt_dev_spgemm_count / _fill), in one run on
one GPU.

    config 3      A 1e6 x 1e4 at 1 %, B 1e4 x 128 at 1 %: the sparse-result product next to svt_dev_matmul_csc_csc, the
                  dense-result product on the same operands in the same process (unchanged by this work: the yardstick)
    no dense form A the same, B 1e4 x 1e4 with 2 nonzeros per column (synth.random_device_csc with total_nnz): time,
                  nonzeros of the result, peak device memory of the composition next to the 80 GB of a dense result
    crossprod     crossprod(X) of the reference's published 25000 x 400 at 7 % shape: the sparse-result product on
                  (t(X), X) next to svt_dev_crossprod_csc_csc on the same pair; t(X) is made once, outside the clock
    regression    with --parent-lib: svt_dev_matmul_csc_csc and svt_dev_crossprod_csc_csc at config 3 on this build and
                  on the library of the parent commit, a child process per run, alternated

A count call synchronises its stream once and is timed by the host clock around it; a fill call and the dense-result
calls are asynchronous and are timed by device events around CALLS calls (tools/sweep_timing.py, whose helpers this
imports).  Everything is warmed, then timed in turn, round after round.  Reported: median / min / max, the spread
(max - min) / median, the ratio to the block's yardstick, and per sparse-result workload the bytes the call must move --
the runs of A the pairs read (12 B an entry) twice, B (12 B an entry) twice, 12 B per result entry written -- with the
rate they imply over count + fill.

    python tools/spgemm_timing.py [--out FILE] [--rounds 11] [--calls 5] [--parent-lib PATH] [--only sparse]

profiles/spgemm_timing.txt holds one output of it.  With SVT_HIP_TUNING=1 (the tuning build) SVT_SPGEMM_PS and
SVT_SPGEMM_WAVES choose the panel height and the wavefronts per workgroup: --only sparse times the first two blocks alone.
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
from sweep_timing import Call, Operand, device_ms, host_ms, row, stream               # noqa: E402
from sparsearray_amd import synth                                                    # noqa: E402
from sparsearray_amd._abi import PROTOTYPES                                          # noqa: E402
from sparsearray_amd.svt import REALSXP                                              # noqa: E402

NROW, NINNER, DENSITY = 1_000_000, 10_000, 0.01


def checksum(t):
    return int(t.view(torch.int64).sum().item())


def operands(dev):
    A = synth.random_device_csc(NROW, NINNER, DENSITY, seed=7, device=dev)
    B = synth.random_device_csc(NINNER, 128, DENSITY, seed=8, device=dev)
    return A, B


# ---------------------------------------------------------------------------
# the child: the two dense-result products at config 3 on the library at `path`, through ctypes alone
# ---------------------------------------------------------------------------
def child(path, rounds, calls):
    lib = ctypes.CDLL(path)
    for name in ("svt_init", "svt_last_error", "svt_wrap_device_csc", "svt_dev_matmul_csc_csc_ws_bytes", "svt_dev_matmul_csc_csc",
                 "svt_dev_crossprod_csc_csc_ws_bytes", "svt_dev_crossprod_csc_csc"):
        f = getattr(lib, name)
        f.restype, f.argtypes = PROTOTYPES[name]
    assert lib.svt_init(0) == 0, lib.svt_last_error()
    dev = torch.device("cuda", 0)
    (acp, ari, av), (bcp, bri, bv) = operands(dev)
    hA = lib.svt_wrap_device_csc(REALSXP, NROW, NINNER, ari.numel(), acp.data_ptr(), ari.data_ptr(), av.data_ptr())
    hB = lib.svt_wrap_device_csc(REALSXP, NINNER, 128, bri.numel(), bcp.data_ptr(), bri.data_ptr(), bv.data_ptr())
    out = torch.empty((128, NROW), dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_m = torch.empty(lib.svt_dev_matmul_csc_csc_ws_bytes(hA), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(lib.svt_dev_crossprod_csc_csc_ws_bytes(hA), dtype=torch.uint8, device=dev)

    def matmul():
        assert lib.svt_dev_matmul_csc_csc(hA, hB, out.data_ptr(), NROW, ws_m.data_ptr(), ws_m.numel(), flag.data_ptr(), stream()) == 0

    def crossprod():            # crossprod(t(A), B) = A %*% B through the other kernel: its first operand is t(t(A)) = A
        assert lib.svt_dev_crossprod_csc_csc(hA, hB, 0, out.data_ptr(), NROW, ws_c.data_ptr(), ws_c.numel(), flag.data_ptr(),
                                             stream()) == 0, lib.svt_last_error()

    res = {}
    for key, fn in (("matmul_csc_csc", matmul), ("crossprod_csc_csc", crossprod)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        res[key] = {"t": [], "check": checksum(out), "flag": int(flag.item())}
    for _ in range(rounds):
        for key, fn in (("matmul_csc_csc", matmul), ("crossprod_csc_csc", crossprod)):
            res[key]["t"].append(device_ms(fn, calls))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libsvt_hip.so of the parent commit, for the dense-result products on both builds")
    ap.add_argument("--only", default=None, choices=("sparse",), help="the sparse-result product of the first two blocks alone")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.rounds, args.calls)
        return
    import sparsearray_amd.device as D
    from sparsearray_amd import _hip
    lib = _hip.init()
    dev = torch.device("cuda", 0)
    P = D.spgemm_panel(NROW)
    knobs = {k: os.environ[k] for k in ("SVT_HIP_TUNING", "SVT_SPGEMM_PS", "SVT_SPGEMM_WAVES") if k in os.environ}
    lines = [f"Sparse x sparse product with a sparse result, device level, ms ({torch.cuda.get_device_name(0)}); panels of {P} rows"
             + (f"; {knobs}" if knobs else "") + ".",
             f"{args.rounds} interleaved rounds after a warm-up; count: one call by the host clock (it synchronises the stream once); "
             f"fill and the dense-result products: {args.calls} calls between two device events.",
             "spread = (max - min) / median; ratio = median / median of the yardstick named in the block.", "",
             f"  {'workload':<34} {'call':<6} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'ratio':>7}"]

    def sparse_call(A, B, label):
        need = lib.svt_dev_spgemm_ws_bytes(A.handle, B.ncol)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        c = Call(lib, Operand(A.nrow, torch.empty(B.ncol + 1, dtype=torch.int64, device=dev), A.row_idx, A.val), label,
                 lambda *a: lib.svt_dev_spgemm_count(*a[:6], flag.data_ptr(), a[6]), lib.svt_dev_spgemm_fill, (A.handle, B.handle),
                 (), (), need, torch.float64)
        c.flag, c.need = flag, need
        return c

    def must_move(A, B, nnz_out):
        """bytes: the runs of A the pairs read, twice; B twice; 12 B per result entry"""
        leaf = (A.col_ptr[1:] - A.col_ptr[:-1])
        runs = int(leaf[B.row_idx.to(torch.int64)].sum().item())
        return 2 * 12 * runs + 2 * 12 * B.nnz + 12 * nnz_out, runs

    def timed(work, dense=()):
        T = {(w.label, k): [] for w in work for k in ("count", "fill")}
        Dn = {label: [] for label, _ in dense}
        for w in work:
            for _ in range(2):
                w.count(), w.fill()
        for _, fn in dense:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for w in work:
                T[(w.label, "count")].append(host_ms(w.count))
                T[(w.label, "fill")].append(device_ms(w.fill, args.calls))
            for label, fn in dense:
                Dn[label].append(device_ms(fn, args.calls))
        return T, Dn

    def report(w, T, A, B, ref=None):
        both = [a + b for a, b in zip(T[(w.label, "count")], T[(w.label, "fill")])]
        nbytes, runs = must_move(A, B, w.nnz.value)
        lines.append(f"{w.label}: result {w.nnz.value} nonzeros, not_finite {int(w.flag.item())}; workspace {w.need / 2 ** 20:.1f} MiB; "
                     f"{runs} entries of A in the runs the pairs read")
        for k in ("count", "fill"):
            lines.append(row("", k, T[(w.label, k)]))
        lines.append(row("", "both", both, ref))
        med = statistics.median(both)
        lines.append(f"  must move {nbytes / 1e9:.3f} GB (runs of A twice, B twice, 12 B per result entry): {nbytes / med / 1e6:.1f} GB/s over count + fill")
        return both

    (acp, ari, av), (bcp, bri, bv) = operands(dev)
    A, B = D.DeviceCSC(NROW, acp, ari, av), D.DeviceCSC(NINNER, bcp, bri, bv)

    # ---- config 3 ----
    sp = sparse_call(A, B, "A %*% B, sparse result")
    out = torch.empty((128, NROW), dtype=torch.float64, device=dev)
    ws_d = torch.empty(lib.svt_dev_matmul_csc_csc_ws_bytes(A.handle), dtype=torch.uint8, device=dev)

    def dense_product():
        D.matmul_csc_csc(A, B, out=out, ws=ws_d)

    dense = [] if args.only else [("A %*% B, dense result (yardstick)", dense_product)]
    T, Dn = timed([sp], dense)
    if not args.only:
        # the two results agree up to the dense kernel's order of additions (a cell that cancels keeps its rounding noise there)
        ref, _ = D.matmul_csc_csc(A, B)
        S = D.DeviceCSC(NROW, sp.cp, sp.ri, sp.vv).to_dense()
        torch.cuda.synchronize()
        assert torch.allclose(S, ref.t(), rtol=1e-12, atol=1e-12), "sparse and dense results differ"
        del ref, S
    lines.append(f"-- config 3: A {NROW} x {NINNER} at {DENSITY:g} ({A.nnz} nonzeros), B {NINNER} x 128 at {DENSITY:g} ({B.nnz} nonzeros)")
    ref_t = Dn[dense[0][0]] if dense else None
    report(sp, T, A, B, ref_t)
    if dense:
        lines.append(row(dense[0][0], "call", ref_t, ref_t))
        lines.append(f"  the dense result is {128 * NROW * 8 / 1e9:.2f} GB written; sparse result both / dense result = "
                     f"{(statistics.median(T[(sp.label, 'count')]) + statistics.median(T[(sp.label, 'fill')])) / statistics.median(ref_t):.2f}")
    del sp, out, ws_d, T, Dn, B
    torch.cuda.empty_cache()

    # ---- the shape that has no dense form ----
    wcp, wri, wv = synth.random_device_csc(NINNER, NINNER, 0.0, seed=9, device=dev, total_nnz=2 * NINNER)
    W = D.DeviceCSC(NINNER, wcp, wri, wv)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    R, flag = A.matmul_sparse(W)
    torch.cuda.synchronize()
    peak, held = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()
    nnz_R = R.nnz
    del R, flag
    torch.cuda.empty_cache()
    sp = sparse_call(A, W, "A %*% W, sparse result")
    T, _ = timed([sp])
    lines.append(f"-- no dense form: A the same, W {NINNER} x {NINNER} with {W.nnz} nonzeros ({W.nnz / NINNER:g} per column); a dense "
                 f"result would be {NROW * NINNER * 8 / 1e9:.0f} GB")
    assert sp.nnz.value == nnz_R
    report(sp, T, A, W)
    lines.append(f"  the composition svt_dev_spgemm: peak device memory {peak / 1e9:.2f} GB with the operands ({before / 1e9:.2f} GB) resident; "
                 f"{held / 1e9:.2f} GB held after it (operands + result of {nnz_R * 12 / 1e9:.2f} GB)")
    del sp, T, W, A
    torch.cuda.empty_cache()

    if not args.only:
        # ---- crossprod(X), 25000 x 400 at 7 % ----
        X = D.DeviceCSC(25000, *synth.random_device_csc(25000, 400, 0.07, seed=11, device=dev))
        Xt = X.t()
        sp = sparse_call(Xt, X, "crossprod(X), sparse result")
        out = torch.empty((400, 400), dtype=torch.float64, device=dev)
        ws_g = torch.empty(lib.svt_dev_crossprod_csc_csc_ws_bytes(Xt.handle), dtype=torch.uint8, device=dev)

        def gram():
            D.crossprod_csc_csc(Xt, X, sym=True, out=out, ws=ws_g)

        T, Dn = timed([sp], [("crossprod_csc_csc(sym) (yardstick)", gram)])
        lines.append(f"-- crossprod(X): X 25000 x 400 at 0.07 ({X.nnz} nonzeros); both on (t(X), X), t(X) made once outside the clock")
        report(sp, T, Xt, X, Dn["crossprod_csc_csc(sym) (yardstick)"])
        lines.append(row("crossprod_csc_csc(sym) (yardstick)", "call", Dn["crossprod_csc_csc(sym) (yardstick)"], Dn["crossprod_csc_csc(sym) (yardstick)"]))
        del sp, T, Dn, X, Xt, out, ws_g
        torch.cuda.empty_cache()

    if args.parent_lib and not args.only:
        from sparsearray_amd._hip import LIB_PATH
        runs = []
        for label, path in (("this build", LIB_PATH), ("parent", args.parent_lib), ("this build", LIB_PATH), ("parent", args.parent_lib)):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path), "--rounds", str(args.rounds),
                                "--calls", str(args.calls)], capture_output=True, text=True, check=True, timeout=600)
            runs.append((label, json.loads(o.stdout.strip().split("\n")[-1])))
        lines.append("-- regression: the dense-result products at config 3 on this build and on the parent commit's library, a process per "
                     "run, alternated; the same checksum of the result from all four (crossprod_csc_csc on (A, B): crossprod(t(A), B))")
        for key in ("matmul_csc_csc", "crossprod_csc_csc"):
            assert all(r[key]["flag"] == 0 for _, r in runs)
            same = all(r[key]["check"] == runs[0][1][key]["check"] for _, r in runs)
            for k, (label, r) in enumerate(runs):
                lines.append(row(f"  {key}, {label}, run {k // 2 + 1}", "call", r[key]["t"]))
            med = lambda k: statistics.median(runs[k][1][key]["t"])       # noqa: E731
            new, par = (med(0) + med(2)) / 2, (med(1) + med(3)) / 2
            lines.append(f"  {key}: this build / parent = {new / par:.3f}; parent run 2 / parent run 1 = {med(3) / med(1):.3f}; "
                         f"checksums {'equal' if same else 'DIFFER (the kernel adds in no fixed order)'}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
