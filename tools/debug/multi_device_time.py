"""Host-level crossprod(A, Y) of BASELINE config 2a (A 1e6 x 1e4 @ 1 %, Y 1e6 x 128) over device lists of length 1, 2, 4
and 8 (svt_set_devices), cold: host operands, every call uploads its shards (the resident cache is off).  Per call: the
wall time, and from the library (SVT_SHARD_TIMING=1, stderr) every shard's upload, product and reduce-scatter times.

    python tools/debug/multi_device_time.py                    # lists {0}, {0,0}, {0,0,0,0}, {0}*8: one GPU
    python tools/debug/multi_device_time.py --devices 0,1,2,3,4,5,6,7   # prefixes of that list: a multi-GPU node

On one GPU the shards share one PCIe link and one chip: the numbers say what the sharded path costs there, not how it
scales."""
import argparse
import os
import sys
import time

os.environ["SVT_SHARD_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sparsearray_amd  # noqa: E402
from sparsearray_amd import SVT_SparseArray, _hip, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--devices", default=None, help="comma-separated ordinals; lists are its prefixes of length 1/2/4/8")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
pool = [int(d) for d in args.devices.split(",")] if args.devices else [0] * 8

hip = sparsearray_amd.hip_session()
NROW, NCOL, K = 1_000_000, 10_000, 128
cp, ri, v = synth.random_device_csc(NROW, NCOL, 0.01, seed=7, device="cuda")
A = SVT_SparseArray.from_csc((NROW, NCOL), "double", cp.cpu().numpy(), ri.cpu().numpy(), v.cpu().numpy())
Y = synth.random_dense(NROW, K, seed=107, device="cuda").cpu().numpy().T
del cp, ri, v
_hip.set_shard_min_nnz(0)
ref = None
for n in (1, 2, 4, 8):
    if n > len(pool):
        break
    _hip.set_devices(pool[:n])
    label = "{" + ",".join(map(str, pool[:n])) + "}"
    for r in range(args.reps):
        t0 = time.perf_counter()
        out = np.asarray(hip.crossprod(A, Y))
        ms = (time.perf_counter() - t0) * 1e3
        sys.stderr.flush()
        if ref is None:
            ref = out
        print(f"{label} call {r}: {ms:.1f} ms wall, max |diff| vs one device {np.max(np.abs(out - ref)):.3e}",
              flush=True)
