"""Differential fuzzing of the device transposition (bucketed count / scan / scatter, and its key-sort
fallback for the shapes it does not take) against a stable sort by row on the GPU: random shapes from one
row to 3e5, from one column to 2e5, densities from 1e-4 to 1, skewed rows and columns, both value types.
    python tools/debug/fuzz_transpose.py [ncases] [seed]
    python tools/debug/fuzz_transpose.py --routes      the route table (below) instead"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sparsearray_amd.device import DeviceCSC


def routes_table():
    """Which routes (device.aperm_route_counts()) fixed operands take: the shapes of the device-level aperm tests and of
    the boxed t() / aperm() tests with their box limits, seeded.  One line per call; two builds of the library that
    are meant to route alike give the same output."""
    from sparsearray_amd import device
    dev = torch.device("cuda", 0)

    def operand(a):
        flat = a.reshape(-1, order="F")
        nz = np.flatnonzero(flat)
        cp = np.zeros(a.size // a.shape[0] + 1, np.int64)
        np.cumsum(np.bincount(nz // a.shape[0], minlength=len(cp) - 1), out=cp[1:])
        return DeviceCSC(a.shape[0], torch.as_tensor(cp, device=dev), torch.as_tensor((nz % a.shape[0]).astype(np.int32), device=dev),
                         torch.as_tensor(flat[nz], device=dev))

    def dense(dim, nnz, dtype, seed):
        rng = np.random.default_rng(seed)
        a = np.zeros(dim, dtype=np.float64 if dtype == "double" else np.int32, order="F")
        if nnz:
            idx = rng.choice(a.size, size=nnz, replace=False)
            a.reshape(-1, order="F")[idx] = rng.normal(size=nnz) if dtype == "double" else rng.integers(1, 1000, size=nnz)
        return a

    def run(name, A, dim, perm, limit=0):
        device.aperm_route_counts(reset=True)
        b0 = device.boxed_calls()
        try:
            device.set_box_nnz(limit)
            A.t() if perm is None else A.aperm(dim, perm)
            torch.cuda.synchronize()
        finally:
            device.set_box_nnz(0)
        rc = device.aperm_route_counts()
        print(f"{name} dim {'x'.join(map(str, dim))} perm {perm} box {limit}: " + " ".join(str(v) for v in rc.values())
              + f" | boxed {device.boxed_calls() - b0}", flush=True)

    d3 = [((700, 40, 23), 20000, p, "double") for p in ((3, 2, 1), (1, 3, 2), (2, 3, 1), (3, 1, 2), (2, 1, 3))]
    swapped = [((3000, 2500, 5), 750_000, (2, 1, 3), "double"), ((3000, 2500, 5), 750_000, (2, 1, 3), "integer"),
               ((1234, 777, 3, 2), 400_000, (2, 1, 3, 4), "double"), ((5000, 300, 7), 900_000, (2, 1, 3), "double"),
               ((700, 40, 23), 20000, (2, 1, 3), "double"), ((3000, 2500, 5), 750_000, (2, 3, 1), "double"),
               ((3000, 2500, 5), 750_000, (3, 2, 1), "double"), ((3000, 2500, 5), 750_000, (3, 2, 1), "integer"),
               ((5000, 300, 7), 900_000, (2, 3, 1), "integer")]
    slab = [((700, 40, 23), 20000, (3, 1, 2), "integer"), ((5000, 9, 64), 30000, (3, 1, 2), "double"),
            ((300, 6, 5, 4), 9000, (3, 1, 2, 4), "double"), ((300, 6, 5, 4), 9000, (4, 1, 3, 2), "double"),
            ((64, 50, 1), 1500, (3, 1, 2), "double"), ((20000, 3, 64), 800000, (3, 1, 2), "double"),
            ((900, 30, 16), 0, (3, 1, 2), "double")]
    general = [((1500, 900, 4, 3), 1_500_000, (2, 4, 1, 3), "double"), ((1500, 900, 4, 3), 1_500_000, (3, 1, 4, 2), "double"),
               ((1500, 4, 900, 3), 1_500_000, (3, 2, 4, 1), "double"), ((1500, 4, 900, 3), 1_500_000, (3, 4, 2, 1), "integer"),
               ((1200, 5, 3, 700, 2), 1_200_000, (4, 5, 1, 3, 2), "double"), ((1200, 5, 3, 700, 2), 1_200_000, (4, 1, 2, 3, 5), "double"),
               ((300, 6, 5, 4), 9000, (2, 4, 3, 1), "double"), ((300, 6, 5, 4), 9000, (4, 3, 2, 1), "integer"),
               ((40, 30, 20, 10, 3), 50_000, (5, 3, 1, 4, 2), "double")]
    for group, cases, seed in (("aperm", d3, 44), ("swapped", swapped, 46), ("slab", slab, 45), ("general", general, 47)):
        for dim, nnz, perm, dtype in cases:
            run(f"{group} {dtype}", operand(dense(dim, nnz, dtype, seed)), dim, perm)
    # one slab over the slab form's cap inside the general form, and inside the 3-d "via" route
    dim, rng = (3000, 4, 6, 5), np.random.default_rng(49)
    a = np.zeros(dim, order="F")
    blk = np.zeros((dim[0], dim[2]))
    blk.reshape(-1)[rng.choice(blk.size, size=12_000, replace=False)] = rng.normal(size=12_000)
    a[:, 0, :, 0] = blk
    mask = np.ones(dim, dtype=bool); mask[:, 0, :, 0] = False
    a.reshape(-1, order="F")[rng.choice(np.flatnonzero(mask.reshape(-1, order="F")), size=80_000, replace=False)] = rng.normal(size=80_000)
    run("slab_refused general", operand(a), dim, (3, 4, 1, 2))
    a3 = np.asfortranarray(a.transpose(0, 2, 1, 3).reshape((3000, 6, 20), order="F"))
    run("slab_refused via", operand(a3), (3000, 6, 20), (3, 2, 1))
    # the boxed drivers
    rm3 = [(2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]
    boxed = [((700, 40, 23), 20000, rm3), ((5000, 300, 7), 900_000, [(2, 1, 3)]), ((900, 30, 16), 40000, [(3, 1, 2)]),
             ((1500, 900, 4, 3), 1_500_000, [(2, 4, 1, 3), (3, 1, 4, 2)]), ((1500, 4, 900, 3), 1_500_000, [(3, 2, 4, 1), (3, 4, 2, 1)]),
             ((1200, 5, 3, 700, 2), 1_200_000, [(4, 5, 1, 3, 2), (4, 1, 2, 3, 5)]), ((300, 6, 5, 4), 9000, [(2, 4, 3, 1), (4, 3, 2, 1)]),
             ((40, 30, 20, 10, 3), 50_000, [(5, 3, 1, 4, 2)]), ((300, 500), 20000, [(2, 1)]), ((64, 50, 1), 1500, [(3, 1, 2), (3, 2, 1)]),
             ((50, 1, 40), 1200, [(2, 1, 3), (2, 3, 1)]), ((1, 60, 45), 1500, rm3), ((900, 30, 16), 0, [(3, 1, 2), (2, 1, 3)])]
    for dim, nnz, perms in boxed:
        for dtype in ("double", "integer"):
            A = operand(dense(dim, nnz, dtype, 50))
            for perm in perms:
                for limit in (257, 4096, 100000):
                    run(f"boxed aperm {dtype}", A, dim, perm, limit)
    for nrow, ncol, nnz in ((700, 900, 54000), (500, 3000, 18000), (5000, 400, 8000), (1, 6000, 2400), (9000, 1, 6000),
                            (300, 100_000, 2400), (3000, 2000, 600_000), (50000, 300, 3000)):
        A = operand(dense((nrow, ncol), nnz, "double", 51))
        for limit in (257, 4096, 100000):
            run("boxed t", A, (nrow, ncol), None, limit)


if len(sys.argv) > 1 and sys.argv[1] == "--routes":
    routes_table()
    sys.exit(0)

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
dev = torch.device("cuda", 0)
bad = 0
for case in range(ncases):
    nrow = int(rng.choice([1, 2, 63, 64, 65, 255, 1000, 1024, 1025, 4097, 20000, 65537, 300000]))
    ncol = int(rng.choice([1, 2, 255, 256, 257, 1000, 5000, 40000, 200000]))
    dens = float(rng.choice([0.0001, 0.001, 0.01, 0.05, 0.3, 1.0]))
    if nrow * ncol * dens > 3e7:
        dens = 3e7 / (nrow * ncol)
    kind = int(rng.integers(0, 4))
    g = torch.Generator(device=dev); g.manual_seed(int(rng.integers(0, 2 ** 31)))
    # a dense mask would not fit: draw linear positions
    n_try = int(nrow * ncol * dens)
    if n_try <= 0:
        n_try = 1
    lin = torch.randint(0, nrow * ncol, (n_try,), generator=g, device=dev, dtype=torch.int64)
    if kind == 1:                                   # a band of heavy rows
        r0 = int(rng.integers(0, nrow))
        extra = torch.arange(ncol, device=dev, dtype=torch.int64) * nrow + r0
        lin = torch.cat([lin, extra])
    if kind == 2:                                   # a few fully dense columns
        for c0 in rng.integers(0, ncol, size=min(3, ncol)):
            lin = torch.cat([lin, int(c0) * nrow + torch.arange(nrow, device=dev, dtype=torch.int64)])
    if kind == 3:                                   # rows crowded at the low end
        lin = (lin // nrow) * nrow + (lin % nrow) % max(1, nrow // 7)
    lin = torch.unique(lin)                         # sorted: column-major order
    ri = (lin % nrow).to(torch.int32)
    col = lin // nrow
    cp = torch.zeros(ncol + 1, dtype=torch.int64, device=dev)
    cp[1:] = torch.cumsum(torch.bincount(col, minlength=ncol), 0)
    is_int = bool(rng.integers(0, 2))
    if is_int:
        v = torch.randint(-50, 50, (lin.numel(),), generator=g, device=dev, dtype=torch.int32)
    else:
        v = torch.randn(lin.numel(), generator=g, device=dev, dtype=torch.float64)
    A = DeviceCSC(nrow, cp, ri, v)
    # every third case with columns that split into slabs: the operand read as an nrow x d2 x nslab array and
    # aperm(x, c(2, 1, 3)) -- the batched form of the bucketed transposition -- and the two permutations composed from it,
    # against a sort of the permuted indices
    nslab = next((q for q in (7, 5, 4, 3, 2) if ncol % q == 0 and ncol // q >= 1), 0) if case % 3 == 2 else 0
    if nslab:
        d2 = ncol // nslab
        j, sl = col % d2, col // d2
        subs, dims3 = [ri.to(torch.int64), j, sl], (nrow, d2, nslab)
        for perm in ((2, 1, 3), (2, 3, 1), (3, 2, 1)):
            if dims3[perm[1] - 1] * dims3[perm[2] - 1] > 5e7:          # (new leaves: their pointers alone would be GBs)
                continue
            P, new_dim = A.aperm(dims3, perm)
            torch.cuda.synchronize()
            ns = [subs[q - 1] for q in perm]
            nd = tuple(dims3[q - 1] for q in perm)
            key = ns[0] + nd[0] * (ns[1] + nd[1] * ns[2])                # linear index in the permuted array
            order = torch.sort(key, stable=True).indices
            want_cp = torch.zeros(nd[1] * nd[2] + 1, dtype=torch.int64, device=dev)
            want_cp[1:] = torch.cumsum(torch.bincount(ns[1] + nd[1] * ns[2], minlength=nd[1] * nd[2]), 0)
            ok3 = new_dim == nd and torch.equal(P.col_ptr, want_cp) and \
                torch.equal(P.row_idx, ns[0][order].to(torch.int32)) and torch.equal(P.val, v[order])
            if not ok3:
                bad += 1
                print(f"MISMATCH (aperm {perm}) case {case}: dim {dims3} nnz {lin.numel()} kind {kind} int {is_int}", flush=True)
            del P, key, order, want_cp, ns
        del j, sl, subs
    # round 5: every fourth case the columns read as three or four further axes and a RANDOM permutation of all axes (the
    # composed route: leaf-preserving step, first two axes swapped or slab form, leaf-preserving step; or the own radix sort)
    if case % 4 == 1 and ncol >= 8:
        facs, rest = [], ncol
        for q in (2, 3, 5, 7, 2, 3):
            if rest % q == 0 and rest // q >= 1 and len(facs) < 3:
                facs.append(q); rest //= q
        if len(facs) >= 2:
            dimsN = (nrow, rest) + tuple(facs)
            strides, st = [], 1
            for dsz in dimsN[1:]:
                strides.append(st); st *= dsz
            subsN = [ri.to(torch.int64)] + [(col // stv) % dsz for stv, dsz in zip(strides, dimsN[1:])]
            for _ in range(3):
                perm = tuple(int(q) + 1 for q in rng.permutation(len(dimsN)))
                nd = tuple(dimsN[q - 1] for q in perm)
                nl = int(np.prod(nd[1:], dtype=np.int64))
                if nl > 5e7:
                    continue
                P, new_dim = A.aperm(dimsN, perm)
                torch.cuda.synchronize()
                ns = [subsN[q - 1] for q in perm]
                leafN = torch.zeros_like(ns[0]); mul = 1
                for a in range(1, len(nd)):
                    leafN = leafN + ns[a] * mul; mul *= nd[a]
                order = torch.sort(ns[0] + nd[0] * leafN, stable=True).indices
                want_cp = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
                want_cp[1:] = torch.cumsum(torch.bincount(leafN, minlength=nl), 0)
                okN = new_dim == nd and torch.equal(P.col_ptr, want_cp) and \
                    torch.equal(P.row_idx, ns[0][order].to(torch.int32)) and torch.equal(P.val, v[order])
                if not okN:
                    bad += 1
                    print(f"MISMATCH (aperm {perm}) case {case}: dim {dimsN} nnz {lin.numel()} kind {kind} int {is_int}", flush=True)
                del P, order, want_cp, leafN, ns
            del subsN
    T = A.t()
    torch.cuda.synchronize()
    order = torch.sort(ri.to(torch.int64), stable=True).indices
    want_idx = col[order].to(torch.int32)
    want_val = v[order]
    want_cp = torch.zeros(nrow + 1, dtype=torch.int64, device=dev)
    want_cp[1:] = torch.cumsum(torch.bincount(ri.to(torch.int64), minlength=nrow), 0)
    ok = torch.equal(T.col_ptr, want_cp) and torch.equal(T.row_idx, want_idx) and torch.equal(T.val, want_val)
    if not ok:
        bad += 1
        print(f"MISMATCH case {case}: nrow {nrow} ncol {ncol} nnz {lin.numel()} kind {kind} int {is_int}", flush=True)
    del A, T, lin, ri, col, cp, v, order, want_idx, want_val, want_cp
print(f"{ncases} cases, {bad} mismatches")
from sparsearray_amd.device import aperm_route_counts
rc = aperm_route_counts()
tot = max(1, sum(rc.values()))
print("routes taken (steps of composed routes included): " + ", ".join(f"{k} {v}" for k, v in rc.items())
      + f"; key sorts = {100.0 * (rc['t_key_sort'] + rc['key_sort_32'] + rc['key_sort_64']) / tot:.1f} % of {tot} route steps")
sys.exit(1 if bad else 0)
