"""t() through the boxed driver against the unboxed routes on one operand both take (~1.5e9 nonzeros, boxes of
2^29), then the boxed t() of the full-size operand of tests/test_hip_past_2e31.py (~2.27e9 nonzeros).  Wall time per
call, best of a few, and a bit-for-bit check.  python tools/debug/boxed_t_time.py [ncol_mid]"""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sparsearray_amd import device
from sparsearray_amd.device import DeviceCSC

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


def timed(A, reps=3):
    best, T = 1e30, None
    for _ in range(reps):
        T = None
        torch.cuda.empty_cache()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        T = A.t(); torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, T


ncol_mid = int(sys.argv[1]) if len(sys.argv) > 1 else 740_000
A = build(ncol_mid)
device.set_box_nnz(0)
t_un, U = timed(A)
key_un = (U.col_ptr.clone(), U.row_idx.clone(), U.val.clone())
del U
c0 = device.boxed_calls()
device.set_box_nnz(1 << 29)
try:
    t_box, Bx = timed(A)
finally:
    device.set_box_nnz(0)
same = all(bool(torch.equal(a, b)) for a, b in zip(key_un, (Bx.col_ptr, Bx.row_idx, Bx.val)))
print(f"mid {R}x{ncol_mid} nnz {A.nnz}: unboxed {t_un:.1f} ms, boxed (2^29) {t_box:.1f} ms, "
      f"ratio {t_box / t_un:.2f}, boxed calls {device.boxed_calls() - c0}, bit-identical {same}", flush=True)
del A, Bx, key_un
torch.cuda.empty_cache()
A = build(1_120_000)
t_full, T = timed(A, reps=2)
print(f"full {R}x1120000 nnz {A.nnz}: boxed (default 2^30) {t_full:.1f} ms", flush=True)
