"""aperm with the permutations that move the rows through the boxed driver: the four 3-d ones at BASELINE config 5
(2e4 x 2e4 x 64 @ 0.5 %, 1.28e8 nonzeros) unforced and with the box limit forced to 2^24 and 2^26 (wall time per call,
best of a few, and a bit-for-bit check), then the full-size calls of tests/test_hip_aperm_past_2e31.py (~2.27e9
nonzeros as 32768 x 1120 x 1000, default boxes of 2^28).  The route counters' deltas tell how many route steps the
boxes took.  python tools/debug/boxed_aperm_time.py [mid|full]   (default: both)
Under `rocprofv3 --kernel-trace --stats` the kernels split into count (abox_axis_count_kernel, abox_leaf_len_kernel,
scans), gather (aperm_leaf_count_kernel / aperm_leaf_copy_kernel / box_rebase_kernel), placement (box_place_kernel)
and the routes' own."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sparsearray_amd import device, synth
from sparsearray_amd.device import DeviceCSC

PERMS = [(2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]
R, S = 32768, 16


def build(ncol):
    """the closed form of tests/test_hip_past_2e31.py over ncol columns (int values)"""
    j = torch.arange(ncol, dtype=torch.int64, device="cuda")
    L = 2000 + (j * 7919) % 49 - 24
    L = torch.where(j % 1000 == 0, torch.full_like(L, R), L)
    cp = torch.zeros(ncol + 1, dtype=torch.int64, device="cuda")
    cp[1:] = torch.cumsum(L, 0)
    nnz = int(cp[-1])
    ri = torch.empty(nnz, dtype=torch.int32, device="cuda")
    val = torch.empty(nnz, dtype=torch.int32, device="cuda")
    for j0 in range(0, ncol, 40000):
        j1 = min(j0 + 40000, ncol)
        jj = torch.repeat_interleave(j[j0:j1], L[j0:j1])
        k = torch.arange(int(cp[j1] - cp[j0]), dtype=torch.int64, device="cuda") - (cp[jj] - cp[j0])
        rows = torch.where(jj % 1000 == 0, k, k * S + (5 * jj) % S)
        v = (31 * jj + 17 * k) % 2001 - 1000
        v = torch.where(v == 0, torch.full_like(v, 1001), v)
        ri[int(cp[j0]):int(cp[j1])] = rows.to(torch.int32)
        val[int(cp[j0]):int(cp[j1])] = v.to(torch.int32)
        del jj, k, rows, v
    return DeviceCSC(R, cp, ri, val)


def timed(A, dim, perm, reps=3):
    best, T, tdim = 1e30, None, None
    for _ in range(reps):
        T = None
        torch.cuda.empty_cache()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        T, tdim = A.aperm(dim, perm); torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, T, tdim


def routes_of(fn):
    r0 = device.aperm_route_counts()
    out = fn()
    r1 = device.aperm_route_counts()
    return out, {k: r1[k] - r0[k] for k in r0 if r1[k] != r0[k]}


def mid():
    D = (20_000, 20_000, 64)
    cp, ri, v = synth.random_device_csc(D[0], D[1] * D[2], 0.005, seed=5, device=torch.device("cuda", 0))
    A = DeviceCSC(D[0], cp, ri, v)
    for perm in PERMS:
        device.set_box_nnz(0)
        t_un, U, _ = timed(A, D, perm)
        line = f"config 5 aperm {perm} nnz {A.nnz}: unforced {t_un:.2f} ms"
        for lg in (24, 26):
            c0 = device.boxed_calls()
            device.set_box_nnz(1 << lg)
            try:
                (t_box, Bx, _), routes = routes_of(lambda: timed(A, D, perm, reps=2))
            finally:
                device.set_box_nnz(0)
            bits = (lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t)
            same = all(bool(torch.equal(a, b)) for a, b in
                       zip((U.col_ptr, U.row_idx, bits(U.val)), (Bx.col_ptr, Bx.row_idx, bits(Bx.val))))
            line += (f"; boxes of 2^{lg}: {t_box:.1f} ms, boxed calls {device.boxed_calls() - c0}, route steps of 2 calls "
                     f"{routes}, bit-identical {same}")
            del Bx
        print(line, flush=True)
        del U


def full():
    A = build(1_120_000)
    dim = (32768, 1120, 1000)
    device.set_box_nnz(0)
    for perm in ((2, 1, 3), (3, 1, 2)):
        (t, T, tdim), routes = routes_of(lambda: timed(A, dim, perm, reps=1))
        print(f"full {dim} nnz {A.nnz} aperm {perm}: {t:.0f} ms, route steps {routes}", flush=True)
        back = (2, 1, 3) if perm == (2, 1, 3) else (2, 3, 1)
        (t, T2, _), routes = routes_of(lambda: timed(T, tdim, back, reps=1))
        print(f"full {tuple(tdim)} aperm {back}: {t:.0f} ms, route steps {routes}, "
              f"round trip identical {bool(torch.equal(T2.row_idx, A.row_idx)) and bool(torch.equal(T2.val, A.val))}", flush=True)
        del T, T2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    if which in ("mid", "both"):
        mid()
        torch.cuda.empty_cache()
    if which in ("full", "both"):
        full()
