"""Wall time of whole R-level calls through Session and the ctypes packer on a SMALL operand (BASELINE config 1, 1e4 x 1e3 @
1 %, as an SVT_SparseArray with its 1000 leaves): argument checks, the leaf table, the library call and the shaping of the
result -- the per-call Python overhead that tools/debug/host_call_latency.py, which calls the C ABI itself, leaves out.
    python tools/debug/session_call_latency.py [reps]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401
import sparsearray_amd
from helpers import random_csc
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
hip = sparsearray_amd.hip_session()
cp, ri, v = random_csc(10_000, 1_000, 0.01, seed=1)
x = sparsearray_amd.SVT_SparseArray.from_csc((10_000, 1_000), "double", cp, ri, v)
y = np.asfortranarray(np.random.default_rng(2).uniform(-1, 1, (10_000, 16)))
rows = [("colSums(x)", lambda: hip.colSums(x)), ("rowMeans(x)", lambda: hip.rowMeans(x)),
        ("colMedians(x)", lambda: hip.colMedians(x)), ("rowQuantiles(x)", lambda: hip.rowQuantiles(x)),
        ("rowRanks(x)", lambda: hip.rowRanks(x)), ("crossprod(x, y[1e4 x 16])", lambda: hip.crossprod(x, y)),
        ("t(x)", lambda: hip.t(x)), ("x[i, j] (500 rows, 100 columns)", lambda: hip.subset(x, range(1, 1001, 2), range(1, 101)))]
for name, fn in rows:
    fn(); fn()
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); best = min(best, time.perf_counter() - t0)
    print(f"session {name:34s} {best * 1e3:8.3f} ms", flush=True)
