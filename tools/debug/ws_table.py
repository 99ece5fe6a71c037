"""Workspace sizes of the device transposition and aperm over a fixed grid, one line per query: the numbers that callers
which allocate once and reuse (DeviceCSC, the host entry points) rely on.  Needs no GPU -- the size functions touch no
device.  A change to kernels_transpose.hip that is meant to leave the sizes alone is checked by running this before and
after and comparing the two outputs:
    python tools/debug/ws_table.py > after.txt
tests/test_ws_bytes.py walks the same grid (grid(), queries())."""
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NNZ = (0, 1, 1000, 10 ** 6, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 31)
BOX = (0, 4096, 10 ** 5)
DIMS = (
    # 2-d
    (700, 40), (20000, 2000), (300000, 200000),
    (0, 5),                                     # an extent of 0
    (3, 2 ** 31),                               # 2^31 leaves
    # 3-d: the shapes of the device-level aperm tests (first two axes swapped, via an intermediate, slab form)
    (700, 40, 23), (3000, 2500, 5), (5000, 300, 7), (5000, 9, 64), (64, 50, 1), (20000, 3, 64), (900, 30, 16),
    (3000, 6, 20), (20000, 20000, 64),
    (100, 0, 7),
    (10, 70000, 40000),                         # 2.8e9 leaves whichever axis leads
    # 4-d: the general (composed) form, the slab form refused inside it, many more leaves than nonzeros
    (1234, 777, 3, 2), (300, 6, 5, 4), (1500, 900, 4, 3), (1500, 4, 900, 3), (3000, 4, 6, 5),
    (20000, 2000, 10, 64),
    # 5-d
    (1200, 5, 3, 700, 2), (40, 30, 20, 10, 3), (7, 0, 3, 2, 2),
)


def library():
    sys.path.insert(0, ROOT)
    from sparsearray_amd._hip import load_library
    return load_library()


def grid():
    """(box limit, nnz, dim) in a fixed order."""
    return itertools.product(BOX, NNZ, DIMS)


def queries(lib):
    """Yields (box, nnz, dim, what, bytes): what is "t" (svt_dev_transpose_ws_bytes of dim[0] rows), "aperm"
    (svt_dev_aperm_ws_bytes) or a 1-based permutation (svt_dev_aperm_perm_ws_bytes).  Leaves the box limit at 0."""
    try:
        for box, nnz, dim in grid():
            lib.svt_dev_set_box_nnz(box)
            nd = len(dim)
            cdim = (ctypes.c_int64 * nd)(*dim)
            yield box, nnz, dim, "t", lib.svt_dev_transpose_ws_bytes(dim[0], nnz)
            yield box, nnz, dim, "aperm", lib.svt_dev_aperm_ws_bytes(nnz, nd, cdim)
            for perm in itertools.permutations(range(1, nd + 1)):
                cperm = (ctypes.c_int * nd)(*perm)
                yield box, nnz, dim, perm, lib.svt_dev_aperm_perm_ws_bytes(nnz, nd, cdim, cperm)
    finally:
        lib.svt_dev_set_box_nnz(0)


if __name__ == "__main__":
    n = 0
    for box, nnz, dim, what, b in queries(library()):
        print(f"box {box} nnz {nnz} dim {'x'.join(map(str, dim))} {what if isinstance(what, str) else 'perm ' + ','.join(map(str, what))}: {b}")
        n += 1
    print(f"{n} rows")
