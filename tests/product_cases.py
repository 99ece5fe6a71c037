"""The cases of the product accuracy tests (test_products_accuracy_cpu.py, test_hip_products_accuracy.py): operands
built by hand at the structural edges of the panel-blocked layouts, the value palettes, and the runners that hold a
result against exact_products.  Every case names the path it is meant to take; the device runner asserts it through
``PbcPlan.plan()`` (svt_dev_crossprod_pbc_plan), so a retuned split rule cannot silently move a case elsewhere.

An operand is built once per process (``structure`` is cached) and every palette is laid over the same nonzero
pattern; the exact result is cached per (structure, palette, K).
"""
from __future__ import annotations

import functools

import numpy as np

import exact_products as xp
from sparsearray_amd import NA_real, SVT_SparseArray

PALETTES = ("full", "spread", "tiny_leaves", "scaled", "cancel", "tracer")
STRUCTURAL = ("tracer", "tiny_leaves", "spread")


# ---------------------------------------------------------------------------
# nonzero patterns
# ---------------------------------------------------------------------------
def _csc_from_pairs(ncol, row, col):
    order = np.lexsort((row, col))
    row, col = np.asarray(row)[order], np.asarray(col)[order]
    assert len(row) == 0 or np.all((np.diff(col) > 0) | (np.diff(row) > 0)), "duplicate (row, column)"
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=ncol))]).astype(np.int64)
    return cp, row.astype(np.int32)


def pattern_random(nrow, ncol, density, seed, band=None):
    """floor(nrow ncol density) nonzeros, uniform; ``band`` = (first row, rows): all of them inside that band."""
    rng = np.random.default_rng(seed)
    rows = nrow if band is None else band[1]
    nnz = int(nrow * ncol * density)
    lin = np.sort(rng.choice(rows * ncol, size=min(nnz, rows * ncol), replace=False))
    return _csc_from_pairs(ncol, lin % rows + (0 if band is None else band[0]), lin // rows)


# records per (group of 16 columns, 128-row panel) tile: 0, 1, 7, 8, 9, 16 and 17 (batches of 8 records), an empty
# first and an empty last tile of a group, empty tiles between full ones, a group without any nonzero
BATCH_EDGE_TILES = [[0, 8, 0, 16, 0], [1, 7, 9, 17, 8], [0, 0, 0, 0, 0], [17, 16, 9, 8, 7], [8, 0, 8, 0, 1],
                    [0, 0, 0, 0, 1], [1, 0, 0, 0, 0], [9, 0, 17, 0, 0]]


def pattern_batch_edges():
    nrow, ncol, cbw = 640, 120, 16
    row, col = [], []
    for g, counts in enumerate(BATCH_EDGE_TILES):
        width = min(cbw, ncol - g * cbw)
        for p, cnt in enumerate(counts):
            j = np.arange(cnt)
            row.append(p * 128 + (j * 37) % 128)
            col.append(g * cbw + (j * 5) % width)
    return (nrow, ncol) + _csc_from_pairs(ncol, np.concatenate(row), np.concatenate(col))


def pattern_per_leaf(nrow, ncol, per_leaf, seed, tail_from=None):
    """``per_leaf`` nonzeros in every leaf; ``tail_from``: every second leaf holds its last one at a row >= tail_from
    (the rows of the last row chunk)."""
    rng = np.random.default_rng(seed)
    hi = nrow if tail_from is None else tail_from
    row = np.sort(rng.integers(0, hi // per_leaf, (ncol, per_leaf)) + np.arange(per_leaf) * (hi // per_leaf), axis=1)
    if tail_from is not None:
        row[::2, -1] = rng.integers(tail_from, nrow, len(row[::2]))
    col = np.repeat(np.arange(ncol), per_leaf)
    return _csc_from_pairs(ncol, row.reshape(-1), col)


def _rand(nrow, ncol, density, seed, band=None):
    return lambda: (nrow, ncol) + pattern_random(nrow, ncol, density, seed, band)


STRUCTURES = {
    "small256": _rand(256, 41, 0.15, 1), "small257": _rand(257, 41, 0.15, 2), "small383": _rand(383, 41, 0.15, 3),
    "batch_edges": pattern_batch_edges,
    "ktiles": _rand(300, 90, 0.2, 4),
    "split16384": _rand(16384, 100, 0.01, 5), "split16383": _rand(16383, 101, 0.01, 6),
    "split16255": _rand(16255, 100, 0.01, 7), "split16462": _rand(16385 + 77, 101, 0.01, 8),
    "split_band": _rand(16384, 100, 0.01, 9, band=(7000, 300)),
    "many_blocks": lambda: (2100, 80 * 263) + pattern_per_leaf(2100, 80 * 263, 3, 10),
    "gather5000": _rand(5000, 170, 0.004, 11),
    "gather64p": _rand(64 * 512, 170, 0.002, 12),
    "gatherx64": _rand(64 * 512, 300, 0.001, 13), "gatherx67": _rand(67 * 512 - 5, 300, 0.001, 14),
    "chunks_gather": lambda: (512 * 512 + 513, 5 * 4096) + pattern_per_leaf(512 * 512 + 513, 5 * 4096, 2, 15,
                                                                              tail_from=512 * 512),
    "chunks_gather2": lambda: (320 * 512 + 600, 5 * 4096) + pattern_per_leaf(320 * 512 + 600, 5 * 4096, 2, 16,
                                                                               tail_from=320 * 512),
    "spare256p": lambda: (256 * 128, 16 * 80) + pattern_per_leaf(256 * 128, 16 * 80, 20, 23),
    "general255": _rand(255, 90, 0.2, 17),
    "nonfinite_dma": _rand(3000, 150, 0.02, 18), "nonfinite_gather": _rand(6000, 170, 0.004, 19),
    "host_0.5": _rand(20000, 300, 0.005, 20), "host_0.1": _rand(40000, 300, 0.001, 21),
    "host_wide": _rand(60000, 1000, 0.01, 22),
}
for _cbw in (5, 16, 17, 32, 33, 40):
    STRUCTURES[f"cols{_cbw}_block_plus_1"] = _rand(300, 16 * _cbw + 1, 0.1, 100 + _cbw)
    STRUCTURES[f"cols{_cbw}_minus_1"] = _rand(300, _cbw - 1, 0.3, 200 + _cbw)


class Structure:
    def __init__(self, name):
        self.name = name
        self.nrow, self.ncol, self.cp, self.ri = STRUCTURES[name]()
        self.nnz = len(self.ri)
        self.leaf = np.repeat(np.arange(self.ncol, dtype=np.int64), np.diff(self.cp))


@functools.lru_cache(maxsize=None)
def structure(name) -> Structure:
    return Structure(name)


# ---------------------------------------------------------------------------
# value palettes (sparse operand x dense operand)
# ---------------------------------------------------------------------------
def _full(rng, shape):
    v = rng.standard_normal(shape)                          # full 53-bit mantissas, magnitudes near 1
    v[v == 0] = 1.0
    return v


def tracer_a(row, col):
    """a = +-(1 + (7 r + 13 c) mod 31), the sign from (3 r + c) mod 2."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    return ((1 + (7 * row + 13 * col) % 31) * (1 - 2 * ((3 * row + col) % 2))).astype(np.float64)


def tracer_y(nrow, K):
    """Y[r, k] = ((40503 r + 9973 k) mod 2**20) - 2**19."""
    r, k = np.arange(nrow, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return (((40503 * r + 9973 * k) % (1 << 20)) - (1 << 19)).astype(np.float64)


def palette(st: Structure, name, K):
    """(val, Y) of the palette laid over the structure; Y is (nrow, K)."""
    rng = np.random.default_rng(sorted(PALETTES).index(name) * 1000 + K)
    nnz, nrow = st.nnz, st.nrow
    if name == "tracer":
        return tracer_a(st.ri, st.leaf), tracer_y(nrow, K)
    if name == "spread":                                    # exponents uniform over 2**+-60, per element
        val = np.ldexp(rng.uniform(0.5, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz), rng.integers(-60, 61, nnz))
        Y = np.ldexp(rng.uniform(0.5, 1.0, (nrow, K)) * rng.choice([-1.0, 1.0], (nrow, K)),
                     rng.integers(-60, 61, (nrow, K)))
        return val, Y
    val, Y = _full(rng, nnz), rng.uniform(-1.0, 1.0, (nrow, K))
    Y[Y == 0] = 0.5
    if name == "tiny_leaves":                               # whole cells far below any absolute floor
        val = val * np.where(st.leaf % 3 == 0, 2.0 ** -60, 1.0)
        Y = Y * np.where(np.arange(K) % 5 == 0, 2.0 ** -40, 1.0)[None, :]
    elif name == "scaled":
        val, Y = val * 2.0 ** 400, Y * 2.0 ** -400
    elif name == "cancel":                                  # pairs (v, -v (1 + 2**-30)) on rows where Y is equal
        first = np.concatenate([[True], st.leaf[1:] != st.leaf[:-1]]) if nnz else np.zeros(0, bool)
        pos = np.arange(nnz) - np.maximum.accumulate(np.where(first, np.arange(nnz), 0))
        odd = pos % 2 == 1
        val[odd] = -val[np.flatnonzero(odd) - 1] * (1.0 + 2.0 ** -30)
        Y = np.repeat(Y[:1, :], nrow, axis=0)
    elif name != "full":
        raise KeyError(name)
    return val, Y


class Expected:
    """The operands of (structure, palette, K) and the exact result: ``p`` (xp.Product) or, for the tracer, the
    int64 arrays E, M, n."""


@functools.lru_cache(maxsize=6)
def expected(sname, pname, K) -> Expected:
    st = structure(sname)
    e = Expected()
    e.st, e.palette, e.K = st, pname, K
    e.val, e.Y = palette(st, pname, K)
    if pname == "tracer":
        e.E, e.M, e.n = xp.tracer_sparse_dense(st.cp, st.ri, e.val, e.Y)
        e.p = None
    else:
        if e.Y.size <= 1 << 22:
            xp.assert_ranges(e.Y)
        e.p = xp.exact_sparse_dense(st.cp, st.ri, e.val, e.Y)
    return e


def check_dense(got, e: Expected, what, rec=None, who="", kernel=""):
    """``got``: (ncol, K).  Tracer: identical to the exact integers.  Else the finite rule, every cell."""
    what = f"{e.st.name} {e.palette} K={e.K} {what}"
    if e.p is None:
        xp.check_identical_product(got, e.E, what)
        worst = 0.0
    else:
        v = xp.check_product(got, e.p, what)
        assert v.ncompared == int((e.p.n > 0).sum())       # no cell left out
        if rec is None:
            v.require()
        worst = v.worst
    if rec is not None:
        key = (who, kernel, e.palette)
        rec[key] = max(rec.get(key, 0.0), worst)


def svt_of(st: Structure, val, type="double"):
    return SVT_SparseArray.from_csc((st.nrow, st.ncol), type, st.cp, st.ri,
                                    val if type == "double" else np.asarray(val).astype(np.int32))


# ---------------------------------------------------------------------------
# the device-level cases of crossprod(x, Y): structure, layout, K, palettes, and the plan each must take
# ---------------------------------------------------------------------------
def _npanels(nrow, logR):
    return (nrow + (1 << logR) - 1) >> logR


DENSE_CASES = {}


def _add(name, **kw):
    DENSE_CASES[name] = kw


# LDS-DMA (CBW, 16, 7).  Fewer than 512 (column block, dense tile) units and fewer than 128 panels: one row split per
# panel (pbc_fill_splits, cut to the panels by pbc_splits), partial sums, never the direct write.
for _n, _np in (("small256", 2), ("small257", 3), ("small383", 3)):
    _add(_n, structure=_n, K=1, layout=(40, 16, 7), palettes=PALETTES,
         plan=dict(kind="dma", kernel="dma", NV=3, nsplit=_np, panels_per_split=1, direct=False, launches=1))
for _lay in ((16, 16, 7), (40, 16, 7)):
    _add(f"batch_edges_cbw{_lay[0]}", structure="batch_edges", K=64, layout=_lay, palettes=PALETTES,
         variants=("cm", "tr", "ld"),
         plan=dict(kind="dma", kernel="dma", NV=(_lay[0] + 15) // 16, nsplit=5, direct=False, launches=1))
for _cbw in (5, 16, 17, 32, 33, 40):
    for _s in (f"cols{_cbw}_block_plus_1", f"cols{_cbw}_minus_1"):
        _add(_s, structure=_s, K=70, layout=(_cbw, 16, 7), palettes=STRUCTURAL,
             plan=dict(kind="dma", kernel="dma", NV=(_cbw + 15) // 16, nsplit=3, direct=False, launches=1))
for _K in (63, 64, 65, 128, 130):
    _add(f"ktiles_K{_K}", structure="ktiles", K=_K, layout=(40, 16, 7), palettes=STRUCTURAL,
         variants=("cm", "tr", "ld") if _K in (65, 128) else ("cm",),
         plan=dict(kind="dma", kernel="dma", NV=3, nsplit=3, direct=False, launches=1))
# Row splits.  128 panels and more, fewer than 512 units: the candidate search of pick_nsplit; a candidate needs 16
# panels per split, so 128 / 129 panels leave 8 splits.  127 panels: pbc_fill_splits, one split per panel.  (16383
# rows are 128 panels, the last one partial; 16255 rows are the 127.)  Even / odd ncol: both forms of pbc_reduce_kernel.
_add("split16384", structure="split16384", K=70, layout=(40, 16, 7), palettes=STRUCTURAL,
     plan=dict(kind="dma", kernel="dma", NV=3, nsplit=8, panels_per_split=16, direct=False, launches=1))
_add("split16383", structure="split16383", K=70, layout=(40, 16, 7), palettes=STRUCTURAL,
     plan=dict(kind="dma", kernel="dma", NV=3, nsplit=8, panels_per_split=16, direct=False, launches=1))
_add("split16255", structure="split16255", K=70, layout=(40, 16, 7), palettes=STRUCTURAL,
     plan=dict(kind="dma", kernel="dma", NV=3, nsplit=127, panels_per_split=1, direct=False, launches=1))
_add("split16462", structure="split16462", K=70, layout=(40, 16, 7), palettes=STRUCTURAL,
     plan=dict(kind="dma", kernel="dma", NV=3, nsplit=8, panels_per_split=17, direct=False, launches=1))
_add("split_band", structure="split_band", K=70, layout=(40, 16, 7), palettes=STRUCTURAL,
     plan=dict(kind="dma", kernel="dma", NV=3, nsplit=8, panels_per_split=16, direct=False, launches=1))
# Gather (CBW, 4, 9..15), fewer than 64 panels: Kp % 128 != 0 -> gather, else gather2; one row chunk.
for _lay in ((40, 4, 9), (16, 4, 10), (33, 4, 9)):
    for _K in (64, 70, 128, 130, 250):                      # Kp = 64, 128, 128, 192, 256
        _kp = (_K + 63) // 64 * 64
        _add(f"gather5000_cbw{_lay[0]}_K{_K}", structure="gather5000", K=_K, layout=_lay, palettes=STRUCTURAL,
             variants=("cm", "tr") if _K in (70, 128) else ("cm",),
             plan=dict(kind="gather", kernel="gather2" if _kp % 128 == 0 else "gather", NV=(_lay[0] + 15) // 16,
                       direct=False, launches=1))


# The cases below need knobs, several products or a large operand: test_hip_products_accuracy.py runs each in a test
# of its own ("own": the generic device runner leaves them alone); the CPU half takes them like the others.
_add("many_blocks", structure="many_blocks", K=128, layout=(5, 16, 7), palettes=STRUCTURAL, own=True, cpu_K=16,
     plan=dict(kind="dma", kernel="dma", NV=1, nsplit=1, direct=True))
# 256 panels, 16 column blocks of 80 leaves x one dense tile = 16 units.  Default: the candidate search of pick_nsplit
# (8 splits in one half-filled round, 15, or 16 in one full round: 16 wins).  With 32 CUs spared: 224 / 16 = 14 splits
# of 19 panels, the 224 workgroups of the packed launch.  DENSE_CASES names the default plan, SPARED_PLAN the other.
_add("spare256p", structure="spare256p", K=64, layout=(5, 16, 7), palettes=STRUCTURAL, own=True, cpu_K=8,
     plan=dict(kind="dma", kernel="dma", NV=1, nsplit=16, panels_per_split=16, direct=False, launches=1))
SPARED_PLAN = dict(kind="dma", kernel="dma", NV=1, nsplit=14, panels_per_split=19, direct=False, launches=1)
_add("from_first_col", structure="batch_edges", K=64, layout=(5, 16, 7), palettes=STRUCTURAL, own=True,
     plan=dict(kind="dma", kernel="dma", NV=1, nsplit=5, direct=False, launches=1))
_add("gather64p_unpaced", structure="gather64p", K=128, layout=(40, 4, 9), palettes=STRUCTURAL, own=True,
     plan=dict(kind="gather", kernel="gather2", NV=3, direct=False, launches=1))
for _s in ("gatherx64", "gatherx67"):
    for _K in (128, 256):
        _add(f"{_s}_K{_K}", structure=_s, K=_K, layout=(40, 4, 9), palettes=STRUCTURAL, own=True,
             plan=dict(kind="gather", kernel="gatherx", nsplit=8, panels_per_split=8 if _s == "gatherx64" else 9,
                       direct=False, launches=1))
# Several row chunks per product: 4096 wavefronts per launch already (pick_nsplit_gather: one split), 514 panels
# against a chunk of 256 << 1, 322 against 160 << 1 (pbc_gather_chunk: 512-row panels).  cpu_K: the CPU half's width.
# One split and K a multiple of 64: with the output laid out like the partials (pbc_direct) the chunks add up in `out`
# itself; given by rows ("tr") they add up in the partials and pbc_reduce_kernel copies them.  The test runs both (by rows: the tracer).
_add("chunks_gather", structure="chunks_gather", K=64, layout=(5, 4, 9), palettes=STRUCTURAL, own=True, cpu_K=2,
     plan=dict(kind="gather", kernel="gather", NV=1, nsplit=1, panels_per_split=514, direct=True, launches=2))
_add("chunks_gather2", structure="chunks_gather2", K=128, layout=(5, 4, 9), palettes=STRUCTURAL, own=True, cpu_K=2,
     plan=dict(kind="gather", kernel="gather2", NV=1, nsplit=1, panels_per_split=322, direct=True, launches=2))


def generic_device_cases():
    return [n for n, c in DENSE_CASES.items() if not c.get("own")]


def assert_plan(got: dict, want: dict, what):
    for k, v in want.items():
        assert got[k] == v, f"{what}: plan[{k!r}] = {got[k]!r}, the case is built for {v!r} (whole plan: {got})"


# ---------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------
def run_dense_case_oracle(oracle, name, rec=None):
    """The reference through every rule of the case (the CPU half: the bounds are theorems about any order)."""
    c = DENSE_CASES[name]
    for pname in c["palettes"]:
        e = expected(c["structure"], pname, c.get("cpu_K", c["K"]))
        got = np.asarray(oracle.crossprod(svt_of(e.st, e.val), np.asfortranarray(e.Y)))
        check_dense(got, e, "oracle", rec, "oracle", c["plan"]["kernel"])


def device_run(plan, e: Expected, variant="cm", first_col=None, sentinel=None):
    """One product of the resident operand through ``plan`` (device.PbcPlan); returns the (ncol, K) host result.
    variant: "cm" column-major Y, out (1, ncol);  "tr" Y by rows (tr_y), out (K, 1);  "ld" column-major with
    ldY = nrow + 3 and NaNs in the padding rows."""
    import torch
    st, K = e.st, e.K
    fill = 3.0 if sentinel is None else sentinel
    if variant == "tr":
        Yd = torch.as_tensor(np.ascontiguousarray(e.Y), device="cuda")              # (nrow, K): K x nrow col-major
        out = torch.full((st.ncol, K), fill, dtype=torch.float64, device="cuda")
        args = (Yd, K, out)
        kw = dict(stride_c=K, stride_k=1, tr_y=True)
    else:
        ld = st.nrow + (3 if variant == "ld" else 0)
        host = np.full((K, ld), np.nan)
        host[:, :st.nrow] = e.Y.T
        Yd = torch.as_tensor(host, device="cuda")
        out = torch.full((K, st.ncol), fill, dtype=torch.float64, device="cuda")
        args = (Yd, ld, out)
        kw = {}
    if first_col is None:
        plan.run(*args, **kw)
    else:
        plan.run_from(first_col, *args, **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got if variant == "tr" else got.T


def plan_kwargs(K, variant):
    return dict(stride_c=K, stride_k=1, tr_y=True) if variant == "tr" else {}


def run_dense_case_device(name, rec=None, who="hip device level"):
    """The case through svt_dev_crossprod_pbc: the plan it names, then every palette and variant."""
    from sparsearray_amd.device import DeviceCSC, PbcPlan
    c = DENSE_CASES[name]
    st = structure(c["structure"])
    for pname in c["palettes"]:
        e = expected(c["structure"], pname, c["K"])
        A = DeviceCSC.from_host(st.nrow, st.cp, st.ri, e.val)
        plan = PbcPlan(A, c["K"], *c["layout"])
        for variant in c.get("variants", ("cm",)):
            want = dict(c["plan"])
            if variant == "tr":
                want["direct"] = False
            assert_plan(plan.plan(**plan_kwargs(c["K"], variant)), want, f"{name} {variant}")
            check_dense(device_run(plan, e, variant), e, variant, rec, who, c["plan"]["kernel"])


# ---------------------------------------------------------------------------
# sparse x sparse
# ---------------------------------------------------------------------------
def sparse_values(row, col, kind, which, seed):
    """Values of a sparse operand, as doubles: "tracer" (integers of magnitude <= 31) or "spread" (exponents uniform
    over 2**+-60, per element)."""
    if kind == "tracer":
        row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
        a, b, m = ((7, 13, 31), (11, 17, 29))[which]
        return ((1 + (a * row + b * col) % m) * (1 - 2 * ((3 * row + col) % 2))).astype(np.float64)
    if kind == "spread":
        rng = np.random.default_rng(seed)
        n = len(row)
        return np.ldexp(rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n), rng.integers(-60, 61, n))
    raise KeyError(kind)


class SparseOperand:
    def __init__(self, nrow, ncol, cp, ri):
        self.nrow, self.ncol, self.cp, self.ri = nrow, ncol, cp, ri
        self.col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(cp))

    def values(self, kind, which, type, seed):
        """An integer operand carries the tracer's integers under either palette."""
        if type == "integer":
            return sparse_values(self.ri, self.col, "tracer", which, seed).astype(np.int32)
        return sparse_values(self.ri, self.col, kind, which, seed)

    def csc(self, v):
        return self.cp, self.ri, v

    def svt(self, v, type):
        return SVT_SparseArray.from_csc((self.nrow, self.ncol), type, self.cp, self.ri, v)


def sparse_operand(nrow, ncol, density, seed, heavy_row=None):
    """Uniform pattern; ``heavy_row`` = (row, nonzeros): that row filled to that many nonzeros."""
    cp, ri = pattern_random(nrow, ncol, density, seed)
    if heavy_row is not None:
        r, cnt = heavy_row
        col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(cp))
        keep = ri != r
        cols = np.sort(np.random.default_rng(seed + 1).choice(ncol, size=cnt, replace=False))
        cp, ri = _csc_from_pairs(ncol, np.concatenate([ri[keep], np.full(cnt, r)]), np.concatenate([col[keep], cols]))
    return SparseOperand(nrow, ncol, cp, ri)


TYPE_PAIRS = [("double", "double"), ("double", "integer"), ("integer", "double"), ("integer", "integer")]


def check_sparse(got, p: xp.Product, kind, what, rec=None, who="", kernel=""):
    """``got``: p.shape.  Integer operands within the integer-exact rule: identical; else the finite rule."""
    if kind == "tracer":
        assert xp.integer_exact(p, 31, 31)
        xp.check_identical_product(got, xp.exact_int(p), what)
        worst = 0.0
    else:
        v = xp.check_product(got, p, what)
        assert v.ncompared == int((p.n > 0).sum())
        if rec is None:
            v.require()
        worst = v.worst
    if rec is not None:
        key = (who, kernel, kind)
        rec[key] = max(rec.get(key, 0.0), worst)


def sparse_kinds(types):
    """Palettes of a type pair.  "spread" lays the spread doubles over every double operand and leaves an integer
    operand its tracer values, so a mixed kernel is held to gamma(n) M on full-mantissa doubles as well; two integer
    operands have the tracer only."""
    return ("tracer",) if types == ("integer", "integer") else ("tracer", "spread")


# x %*% y: result rows on both sides of the 8192-row LDS panel of kernels_spmm.hip
MATMUL_ROWS = (8191, 8192, 8193, 16385)


@functools.lru_cache(maxsize=None)
def matmul_operands(nrow):
    return sparse_operand(nrow, 400, 0.004, 300 + nrow % 7), sparse_operand(400, 50, 0.05, 310)


# crossprod(x, y) and crossprod(x): the lane-group width G of launch_gram (kernels_gram.hip), which has no query.  The
# walk of a lane group is a row of x cut into panels: run = nnz(x) / nrow(x), divided by the number of column panels in
# the panel form and halved in the symmetric form; G = 8 below 32, 16 below 64, else the 32-wide kernels.  Each case
# names the G it is built for under (form, blocking) and ``gram_lane_group`` -- the same arithmetic -- asserts it.
# "ps": log2 of the panel width the case's "panels" run sets (64 columns hold at most 64 nonzeros of a row, so the wider
# forms need wider panels); "heavy": one row of 100 times the mean.
GRAM_PANEL_DEFAULT = (20400, 13)                            # one block up to 20400 result rows (symmetric: 16384)
GRAM_ROWS = {
    "short": dict(nrow=160, nx=700, d=0.02, ps=6, G={"gen one": 8, "gen pan": 8, "sym one": 8, "sym pan": 8}),
    "medium": dict(nrow=160, nx=700, d=0.07, ps=6, G={"gen one": 16, "gen pan": 8, "sym one": 8, "sym pan": 8}),
    "long": dict(nrow=160, nx=700, d=0.2, ps=6, G={"gen one": 32, "gen pan": 8, "sym one": 32, "sym pan": 8}),
    "one_heavy_row": dict(nrow=160, nx=1500, d=0.004, ps=6, heavy=(77, 600),
                          G={"gen one": 8, "gen pan": 8, "sym one": 8, "sym pan": 8}),
    "sym_medium": dict(nrow=160, nx=700, d=0.13, ps=6, G={"gen one": 32, "gen pan": 8, "sym one": 16, "sym pan": 8}),
    "panels_medium": dict(nrow=40, nx=700, d=0.2, ps=8, G={"gen one": 32, "gen pan": 16, "sym one": 32, "sym pan": 8}),
    "panels_long": dict(nrow=40, nx=700, d=0.35, ps=8, G={"gen one": 32, "gen pan": 32, "sym one": 32, "sym pan": 16}),
    "panels_sym_long": dict(nrow=24, nx=512, d=0.55, ps=8,
                            G={"gen one": 32, "gen pan": 32, "sym one": 32, "sym pan": 32}),
}


def gram_lane_group(nnz, nrow, nx, sym, one_block_max, log2_panel):
    """The lane-group width launch_gram takes under set_sparse_crossprod_panel(one_block_max, log2_panel)."""
    one_block_max = GRAM_PANEL_DEFAULT[0] if one_block_max < 0 else min(one_block_max, GRAM_PANEL_DEFAULT[0])
    ps = GRAM_PANEL_DEFAULT[1] if not 4 <= log2_panel <= 14 else log2_panel
    run = nnz / nrow
    if nx > (min(one_block_max, 16384) if sym else one_block_max):
        run /= (nx + (1 << ps) - 1) >> ps
    if sym:
        run *= 0.5
    G = 64
    while G > 8 and run < 2.0 * G:
        G >>= 1
    return min(G, 32)


def gram_panel(name, panels):
    """The arguments of set_sparse_crossprod_panel for the one-block run or the "panels" run of a case."""
    return (0, GRAM_ROWS[name]["ps"]) if panels else (-1, -1)


@functools.lru_cache(maxsize=None)
def gram_operands(name):
    g = GRAM_ROWS[name]
    x = sparse_operand(g["nrow"], g["nx"], g["d"], 400 + len(name), heavy_row=g.get("heavy"))
    y = sparse_operand(g["nrow"], 60, 0.1, 410)
    for key, want in g["G"].items():
        sym, panels = key.startswith("sym"), key.endswith("pan")
        got = gram_lane_group(len(x.ri), x.nrow, x.ncol, sym, *gram_panel(name, panels))
        assert got == want, f"{name}: {key} takes G = {got}, the case is built for {want}"
    return x, y


# ---------------------------------------------------------------------------
# non-finite dense operand: an Inf, a NaN and an NA on rows that some leaves hold and others do not; a saturated column
# ---------------------------------------------------------------------------
NONFINITE_CASES = {"dma": dict(structure="nonfinite_dma", K=20, layout=(40, 16, 7), kernel="dma"),
                   "gather": dict(structure="nonfinite_gather", K=64, layout=(40, 4, 10), kernel="gather")}


def nonfinite_operands(name, saturated=False):
    """(structure, val, Y): the "full" palette with the non-finite entries planted in Y."""
    c = NONFINITE_CASES[name]
    st = structure(c["structure"])
    val, Y = palette(st, "full", c["K"])
    Y = Y.copy()
    if saturated:
        Y[:, 2] = np.nan                                    # more non-finite entries than any leaf has nonzeros
        return st, val, Y
    leaves = [c_ for c_ in (3, st.ncol // 2, st.ncol - 2) if st.cp[c_ + 1] > st.cp[c_]]
    assert len(leaves) == 3
    for (leaf, k), v in zip(zip(leaves, (1, 7, c["K"] - 1)), (np.inf, np.nan, NA_real)):
        r = int(st.ri[st.cp[leaf]])                         # on a nonzero of that leaf
        assert np.sum(st.ri == r) < st.ncol                 # ... and not of every leaf
        Y[r, k] = v
    return st, val, Y


# ---------------------------------------------------------------------------
# host entry points (a session: the product's, or the reference's for the CPU half)
# ---------------------------------------------------------------------------
HOST_CASES = [(s, t, p) for s in ("host_0.5", "host_0.1") for t in ("double", "integer")
              for p in ("tracer", "tiny_leaves")]
HOST_K = 24
# the kind of the layout svt_dev_pbc_build(A, 0, 0, 0) -- what the host entry points build -- picks for each operand:
# 25.6 nonzeros per (40-column group, 128-row panel) tile at 0.5 %, 5.1 at 0.1 % (pbc_auto_layout: gather below 12)
HOST_LAYOUT = {"host_0.5": "dma", "host_0.1": "gather", "host_wide": "dma"}


def host_expected(sname, type, pname, K=HOST_K):
    """An integer operand carries the tracer's values under either palette of the dense operand."""
    st = structure(sname)
    e = Expected()
    e.st, e.palette, e.K = st, pname, K
    e.val, e.Y = palette(st, pname, K)
    if type == "integer":
        e.val = tracer_a(st.ri, st.leaf).astype(np.int32)
    if pname == "tracer":
        e.E, e.M, e.n = xp.tracer_sparse_dense(st.cp, st.ri, e.val, e.Y)
        e.p = None
    else:
        e.p = xp.exact_sparse_dense(st.cp, st.ri, e.val, e.Y)
    return e


def run_host_case(session, sname, type, pname, rec=None, who="", K=HOST_K):
    """crossprod(x, Y) (svt_crossprod2_SVT_mat), crossprod(Y, x) (svt_crossprod2_mat_SVT) and t(x) %*% Y
    (svt_matmul_SVT_mat) of one operand: the same cells three times."""
    e = host_expected(sname, type, pname, K)
    st = e.st
    x = svt_of(st, e.val, type)
    tp, ti, tv = xp.transpose_csc(st.nrow, st.cp, st.ri, e.val)
    xt = SVT_SparseArray.from_csc((st.ncol, st.nrow), type, tp, ti, tv)
    Y = np.asfortranarray(e.Y if type == "double" or pname != "tracer" else e.Y.astype(np.int32))
    check_dense(np.asarray(session.crossprod(x, Y)), e, f"{type} crossprod(x, y)", rec, who, "host SVT_mat")
    check_dense(np.asarray(session.crossprod(Y, x)).T, e, f"{type} crossprod(y, x)", rec, who, "host mat_SVT")
    check_dense(np.asarray(session.matmul(xt, Y)), e, f"{type} t(x) %*% y", rec, who, "host matmul_SVT_mat")


# ---------------------------------------------------------------------------
# sparse x sparse runners: ``product(x_csc_values..)`` is the session's or the device level's
# ---------------------------------------------------------------------------
def run_matmul_case(product, nrow, types, rec=None, who=""):
    """x %*% y, x with ``nrow`` rows.  product(A, B, va, vb) -> (nrow, ncol(y)) array."""
    A, B = matmul_operands(nrow)
    for kind in sparse_kinds(types):
        va, vb = A.values(kind, 0, types[0], 1), B.values(kind, 1, types[1], 2)
        p = xp.exact_matmul_sparse(A.nrow, A.csc(va), B.csc(vb))
        check_sparse(product(A, B, va, vb), p, kind, f"matmul rows={nrow} {types} {kind}", rec, who, "spmm")


def run_gram_case(product, name, types, sym=False, rec=None, who="", kernel="gram"):
    """crossprod(x, y) (sym: crossprod(x)).  product(X, Y, vx, vy, sym) -> (ncol(x), ncol(y)) array."""
    X, Y = gram_operands(name)
    if sym:
        Y = X
    for kind in sparse_kinds(types):
        vx = X.values(kind, 0, types[0], 3)
        vy = vx if sym else Y.values(kind, 1, types[1], 4)
        p = xp.exact_sparse_sparse(X.nrow, X.csc(vx), Y.csc(vy))
        got = product(X, Y, vx, vy, sym)
        if sym:
            assert np.array_equal(got, got.T), f"{name}: crossprod(x) must be bit-symmetric"
        check_sparse(got, p, kind, f"crossprod {name} {types} {kind} sym={sym}", rec, who, kernel)


def _type_of(v):
    return "integer" if v.dtype == np.int32 else "double"


def oracle_matmul(oracle):
    return lambda A, B, va, vb: np.asarray(oracle.matmul(A.svt(va, _type_of(va)), B.svt(vb, _type_of(vb))))


def oracle_gram(oracle):
    def f(X, Y, vx, vy, sym):
        x = X.svt(vx, _type_of(vx))
        return np.asarray(oracle.crossprod(x) if sym else oracle.crossprod(x, Y.svt(vy, _type_of(vy))))
    return f
