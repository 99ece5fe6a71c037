"""Workspace sizes of the device aperm (no compute calls: runs without a GPU).  include/svt_hip.h promises that
svt_dev_aperm_ws_bytes() is at least the need of every permutation, svt_dev_aperm_perm_ws_bytes(): callers that
allocate once for an array and then permute it any way rely on it.  Walked over the grid of tools/debug/ws_table.py:
every route's shapes, nonzero counts on both sides of 2^31, an extent of 0, 2^31 leaves, three box limits."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ws_table():
    spec = importlib.util.spec_from_file_location("ws_table", os.path.join(ROOT, "tools", "debug", "ws_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_aperm_ws_bytes_covers_every_permutation():
    wt = _ws_table()
    whole, nperm, bad = {}, 0, []
    for box, nnz, dim, what, b in wt.queries(wt.library()):
        if what == "aperm":
            whole[(box, nnz, dim)] = b
        elif what != "t":
            nperm += 1
            if b > whole[(box, nnz, dim)]:
                bad.append((box, nnz, dim, what, b, whole[(box, nnz, dim)]))
    assert len(whole) == len(wt.BOX) * len(wt.NNZ) * len(wt.DIMS)
    assert nperm > 10000
    assert not bad, f"{len(bad)} permutations need more than svt_dev_aperm_ws_bytes(): first {bad[:5]}"
