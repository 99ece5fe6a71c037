"""Hand-built operands for the layout kernels (kernels_transpose.hip): one case per route of the dispatcher and per
data-dependent branch of the three bucketed passes, the plain 64-bit reference, the value palettes and the comparison.

The kernels only copy, so the rule is identity at tolerance 0: pointers and indices equal, values equal AS BITS
(``np.array_equal`` on floats cannot tell NaN payloads or -0.0 from 0.0), dtype and the logical flag kept.

Every case names the branch it is for and states what it expects BEFORE anything runs:

* ``plan``  -- fields of ``device.transpose_plan()`` (svt_dev_transpose_plan, the launch's own decision), and
* ``check`` -- the case's arithmetic in numpy from the plan's fbits / cbits (the nonzeros of the fullest
  256-column group x coarse bucket = what one pass-2 workgroup assembles, against T2_CAP; of the fullest fine bucket =
  what one pass-3 workgroup ranks, against T3_CAP / T3_STAGE), so that a retuned rule cannot move a case elsewhere
  without tests/test_transpose_cases_cpu.py failing, and
* ``route`` -- the exact delta of ``device.aperm_route_counts()`` for the one call.  The aperm routes are derived
  from the conditions written in launch_aperm_n() and its callees (order: leaf-preserving, 3-d through an
  intermediate, first two axes swapped, slab, general, key sort; a nested step skips the composed forms), not copied
  from a run.

Left out: ``key_sort_64`` needs a result of 2^31 - 1 leaves or more (a 17 GB pointer array), and operands of 2^31
nonzeros need 24 GB and more; tests/test_hip_aperm_past_2e31.py and test_hip_past_2e31.py cover what of that fits a
test.
"""
from __future__ import annotations

import functools
from math import prod

import numpy as np

T2_CAP, T3_CAP, T3_STAGE, T1_HIST, SLAB_CAP, T2_NT = 2048, 4096, 2048, 65536, 8192, 256

NA_REAL_BITS = 0x7FF00000000007A2
# doubles no float comparison tells apart: NA_real, two NaNs of other payloads (one negative), +-Inf, -0.0, stored 0.0
SPECIALS_F64 = np.array([NA_REAL_BITS, 0x7FF8000000000001, 0xFFF80000DEADBEEF, 0x7FF0000000000000, 0xFFF0000000000000,
                         0x8000000000000000, 0x0000000000000000], dtype=np.uint64).view(np.float64)
NA_INT = np.int32(-2 ** 31)
SPECIALS_I32 = np.array([NA_INT, 0, -1, 2 ** 31 - 1, 1], dtype=np.int32)       # NA_integer, a stored 0, the extremes
SPECIALS_LGL = np.array([1, NA_INT, 1, 1, NA_INT], dtype=np.int32)             # TRUE / NA
DTYPES = ("double", "integer", "logical")
PALETTES = ("tracer", "specials")


# ---------------------------------------------------------------------------
# patterns: sorted linear indices (column-major, int64) of the nonzeros of an array of extents `dim`
# ---------------------------------------------------------------------------
def _rand(dim, nnz, seed):
    size = prod(dim)
    return np.sort(np.random.default_rng(seed).choice(size, size=int(nnz), replace=False)).astype(np.int64)


def _mask(m):
    return np.flatnonzero(m.reshape(-1, order="F")).astype(np.int64)


def _two_windows(dim):
    rng = np.random.default_rng(5)
    m = np.zeros(dim, dtype=bool)
    m[35, :] = True                                       # a full row ...
    m[37, ::3] = True
    m[40:48, :] = rng.random((8, dim[1])) < 0.02          # ... and sparse rows in the same fine bucket
    m[dim[0] - 1, 7] = True                               # whole empty buckets in between
    return _mask(m)


def _sparse_plus_full_row(dim, dens, row, seed):
    m = np.random.default_rng(seed).random(dim) < dens
    m[row, :] = True
    return _mask(m)


def _sparse_plus_dense_cols(dim, dens, cols, seed):
    m = np.random.default_rng(seed).random(dim) < dens
    m[:, cols] = True
    return _mask(m)


def _dense(dim):
    return np.arange(prod(dim), dtype=np.int64)


def _two_per_column(dim):
    c = np.arange(dim[1], dtype=np.int64)
    r1, r2 = (c * 5) % 16, 16 + (c * 3) % 16
    return np.stack([c * dim[0] + r1, c * dim[0] + r2], axis=1).reshape(-1)


def _last_column_only(dim):
    rows = np.flatnonzero(np.random.default_rng(7).random(dim[0]) < 0.5)
    return (dim[1] - 1) * dim[0] + rows.astype(np.int64)


def _first_row_only(dim):
    cols = np.flatnonzero(np.random.default_rng(8).random(dim[1]) < 0.5)
    return cols.astype(np.int64) * dim[0]


def _swap_holes(dim, nnz, seed):
    """random, then one slab emptied and one column of another slab emptied"""
    lin = _rand(dim, nnz, seed)
    leaf = lin // dim[0]
    slab = leaf // dim[1]
    return lin[~((slab == 1) | (leaf == 7))]


def _slab_skew(dim, first, rest, seed):
    """aperm(x, c(3, 1, 2)) of (d0, nslab, dq): slab s = x[:, s, :]; `first` nonzeros in slab 0, `rest` in each other"""
    rng = np.random.default_rng(seed)
    d0, ns, dq = dim
    out = []
    for s in range(ns):
        cells = np.sort(rng.choice(d0 * dq, size=first if s == 0 else rest, replace=False)).astype(np.int64)
        r, k = cells % d0, cells // d0
        out.append(r + d0 * (s + ns * k))
    return np.sort(np.concatenate(out))


def _one_per_column(dim, seed):
    ncol = prod(dim[1:])
    r = np.random.default_rng(seed).integers(0, dim[0], size=ncol)
    return np.arange(ncol, dtype=np.int64) * dim[0] + r


def _refused_inside_general(dim):
    """one slab (fixed indices of axes 2 and 4) holds 12 000 of its 18 000 cells, the other 19 share 80 000"""
    rng = np.random.default_rng(49)
    m = np.zeros(dim, dtype=bool, order="F")
    blk = np.zeros(dim[0] * dim[2], dtype=bool)
    blk[rng.choice(blk.size, size=12_000, replace=False)] = True
    m[:, 0, :, 0] = blk.reshape(dim[0], dim[2])
    free = np.ones(dim, dtype=bool, order="F")
    free[:, 0, :, 0] = False
    rest = np.flatnonzero(free.reshape(-1, order="F"))
    m.reshape(-1, order="F")[rng.choice(rest, size=80_000, replace=False)] = True
    return _mask(m)


# ---------------------------------------------------------------------------
# the arithmetic of a t() case, from the plan
# ---------------------------------------------------------------------------
def loads(dim, lin, plan):
    """(nonzeros per (group, coarse bucket) as a 2-d array, nonzeros per fine bucket, nonzeros of the fullest fine
    bucket per group) of the 2-d operand under the plan's fbits / cbits."""
    row, col = lin % dim[0], lin // dim[0]
    fine = row >> plan["fbits"]
    wg = np.bincount((col >> 8) * plan["ncoarse"] + (fine >> plan["cbits"]), minlength=plan["ngroups"] * plan["ncoarse"])
    fb = np.bincount(fine, minlength=plan["nfb"])
    top = np.bincount((col >> 8)[fine == int(np.argmax(fb))], minlength=plan["ngroups"])
    return wg.reshape(plan["ngroups"], plan["ncoarse"]), fb, top


def _chk_plain(dim, lin, plan):
    wg, fb, _ = loads(dim, lin, plan)
    assert 0 < wg.max() <= T2_CAP and 0 < fb.max() <= T3_STAGE, (wg.max(), fb.max())


def _chk_two_windows(dim, lin, plan):
    wg, fb, _ = loads(dim, lin, plan)
    assert wg.max() <= T2_CAP and T3_STAGE < fb.max() <= T3_CAP, (wg.max(), fb.max())
    assert fb.min() == 0                                  # empty fine buckets too


def _chk_pass3_rounds(dim, lin, plan):
    wg, fb, top = loads(dim, lin, plan)
    assert fb.max() > 2 * T3_CAP, fb.max()                # at least three rounds
    assert (top > 0).all() and plan["ngroups"] > 1        # its pieces come from every group
    assert plan["fbits"] >= 1


def _chk_pass3_rounds_last(dim, lin, plan):
    _chk_pass3_rounds(dim, lin, plan)
    _, fb, _ = loads(dim, lin, plan)
    assert dim[0] % (1 << plan["fbits"]) != 0 and int(np.argmax(fb)) == plan["nfb"] - 1      # the ragged last bucket


def _chk_pass2_rounds(dim, lin, plan):
    wg, fb, _ = loads(dim, lin, plan)
    assert wg.max() > T2_CAP and 0 < wg[wg > 0].min() <= T2_CAP, (wg.max(), wg.min())      # both paths in one launch


def _chk_two_sweeps(dim, lin, plan):
    wg, fb, _ = loads(dim, lin, plan)
    assert plan["nfb"] > T1_HIST and wg.max() == T2_CAP   # (and a pass-2 workgroup exactly at the cap)


def _chk_one_sweep_wide(dim, lin, plan):
    assert T1_HIST // 2 < plan["nfb"] <= T1_HIST


def _chk_6000(dim, lin, plan):
    wg, fb, top = loads(dim, lin, plan)
    assert fb.min() > 20 * T3_CAP and (top > 0).all()     # every fine bucket in rounds, pieces from all 6000 groups


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
def _t(name, dim, build, branch, bucketed, plan=None, check=None, arena=None, route=None):
    p = {"bucketed": bucketed}
    p.update(plan or {})
    if route is None:
        route = {"t_bucketed": 1} if bucketed else {"t_key_sort": 1}
    return dict(name=name, dim=tuple(dim), perm=None, build=build, branch=branch, plan=p, check=check, route=route,
                arena=arena)


def slab_counts(dim, perm, lin):
    """nonzeros per slab of the slab form for aperm(x, perm): one slab per index of the axes perm[2:]"""
    rest, coord = lin.copy(), []
    for d in dim:
        coord.append(rest % d)
        rest //= d
    key, mul = np.zeros(lin.size, dtype=np.int64), 1
    for p in perm[2:]:
        key += coord[p - 1] * mul
        mul *= dim[p - 1]
    return np.bincount(key, minlength=mul)


def _slabs(largest=None, mean=None):
    """the largest slab exactly `largest` (else: within SLAB_CAP), nnz / nslab exactly `mean`"""
    def check(dim, perm, lin):
        n = slab_counts(dim, perm, lin)
        assert n.max() == largest if largest is not None else n.max() <= SLAB_CAP, n.max()
        assert mean is None or lin.size // n.size == mean, lin.size // n.size
    return check


def _a(name, dim, perm, build, branch, route, swap=None, arena=None, check=None):
    """swap: (dim0, dim1, nslab) -> expected `bucketed` of the plan of the batched transposition the route depends on;
    check(dim, perm, lin): the case's own arithmetic"""
    return dict(name=name, dim=tuple(dim), perm=tuple(perm), build=build, branch=branch, plan=None, check=check,
                route=route, swap=swap, arena=arena)


LP, SW, SLAB, VIA, GEN, K32, REFUSED = ("leaf_preserving", "first_two_axes_swapped", "slab", "via_intermediate_3d",
                                        "general_composed", "key_sort_32", "slab_refused_at_run_time")
_KEY_SORT_SHAPES = ((200, 70_000, 30_000, 1), (60_000, 50_000, 41_000, 2), (3_000_000, 9_000, 10_000, 3),
                    (20_000_000, 3_000, 70_001, 4), (100, 5, 3, 1))
_G4, _G4B, _G5, _G3S = (1500, 900, 4, 3), (1500, 4, 900, 3), (1200, 5, 3, 700, 2), (1500, 2, 2500, 2)

CASES = [
    # ---- t(): the bucketed form and its branches
    _t("t_plain_staged", (3000, 700), lambda d: _rand(d, 21_000, 41), "every pass-2 workgroup and fine bucket staged in LDS",
       True, check=_chk_plain, arena="bucketed staged"),
    _t("t_two_stage_windows", (1000, 2500), _two_windows, "pass 3 staged, two T3_STAGE windows", True, {"fbits": 6},
       _chk_two_windows),
    _t("t_pass3_rounds", (2000, 9000), lambda d: _sparse_plus_full_row(d, 0.01, 777, 11),
       "pass 3 unstaged: > T3_CAP, three rounds and more", True, check=_chk_pass3_rounds, arena="pass 3 in rounds"),
    _t("t_pass3_rounds_last_row", (1989, 9000), lambda d: _sparse_plus_full_row(d, 0.01, 1988, 12),
       "pass 3 unstaged in the ragged last fine bucket, the full row its last", True, check=_chk_pass3_rounds_last),
    _t("t_pass2_rounds_group", (3000, 3000), lambda d: _sparse_plus_dense_cols(d, 0.01, slice(256, 512), 13),
       "pass 2 unstaged: one group of 256 dense columns, the others staged", True, check=_chk_pass2_rounds),
    _t("t_pass2_rounds_two_columns", (3000, 3000), lambda d: _sparse_plus_dense_cols(d, 0.01, [300, 301], 14),
       "pass 2 unstaged through two dense columns only", True, check=_chk_pass2_rounds),
    _t("t_fbits0_two_count_sweeps", (70_000, 64), _dense, "fbits 0, nfb > T1_HIST: a second sweep of pass 1", True,
       {"fbits": 0}, _chk_two_sweeps),
    _t("t_fbits0_one_wide_sweep", (40_000, 32), _dense, "fbits 0, T1_HIST / 2 < nfb <= T1_HIST: one sweep, upper half of hist[]",
       True, {"fbits": 0}, _chk_one_sweep_wide),
    _t("t_cbits4", (5003, 3000), lambda d: _rand(d, 750_450, 41), "16 fine buckets per coarse one", True, {"cbits": 4}),
    _t("t_cbits5", (257, 5), lambda d: _rand(d, 385, 41), "32 fine buckets per coarse one", True, {"cbits": 5}),
    _t("t_6000_groups", (32, 1_536_000), _two_per_column, "ngroups == 6000: the largest dynamic LDS of pass 3", True,
       {"ngroups": 6000, "fbits": 0}, _chk_6000, arena="6000 groups"),
    _t("t_6001_groups", (32, 1_536_001), _two_per_column, "ngroups == 6001: refused, key sort", False,
       {"key_sort_passes": 1}),
    # t2_shape() accepts one quarter-full column of 16 384 rows (fbits 0: 16 384 fine buckets), but the head of the
    # workspace (table, fine-bucket bases, scan scratch) is larger than what t2_reserve() sets aside for 4096 nonzeros
    _t("t_reserve_fallback", (16_384, 1), lambda d: _rand(d, 4096, 15), "t2_head(sh).total > reserve: key sort", False,
       {"why_not": "reserve", "key_sort_passes": 2}),
] + [
    # ---- t(): the key sort, one to four passes of 8 bits
    # (the five shapes of test_transpose_shapes_for_the_own_radix_sort; the plan says the last one, three nonzeros in
    # 100 x 5, is a bucketed shape: one fine bucket of 32 rows holds "one nonzero per thread" by the rule's arithmetic)
    _t(f"t_key_sort_{nrow}x{ncol}", (nrow, ncol), functools.partial(lambda d, n: _rand(d, n, 48), n=nnz),
       f"key sort, {ps} passes" if nrow != 100 else "three nonzeros, bucketed", nrow == 100, {"key_sort_passes": ps},
       arena="key sort" if nrow == 60_000 else None)
    for nrow, ncol, nnz, ps in _KEY_SORT_SHAPES
] + [
    # ---- t(): degenerate shapes (their form is the plan's; stated here, asserted on the CPU)
    _t("t_one_row", (1, 3000), lambda d: _rand(d, 1500, 3), "1 x n", False),
    _t("t_one_column", (3000, 1), lambda d: _rand(d, 1500, 4), "n x 1", True),
    _t("t_one_nonzero", (50, 40), lambda d: np.array([1234], dtype=np.int64), "nnz 1", False),
    _t("t_last_column_only", (500, 300), _last_column_only, "every column empty but the last", False),
    _t("t_first_row_only", (500, 300), _first_row_only, "every row empty but the first", False),
    _t("t_no_nonzeros", (30, 20), lambda d: np.zeros(0, dtype=np.int64), "0 nonzeros: a memset, no route", False, route={}),
    # ---- aperm: first two axes swapped
    _a("a_swap01", (3000, 2500, 5), (2, 1, 3), lambda d: _swap_holes(d, 750_000, 46),
       "batched bucketed transposition; an emptied slab, an empty column", {SW: 1}, swap=((3000, 2500, 5), True), arena="swap01"),
    _a("a_swap01_4d", (1500, 2500, 2, 2), (2, 1, 3, 4), lambda d: _rand(d, 300_000, 46), "four slabs over two outer axes",
       {SW: 1}, swap=((1500, 2500, 4), True)),
    # many small slabs: the batched form refuses; dim[1] = 900 <= 1024 but 125 000 nonzeros per slab is no slab-form
    # shape; the general form has no step left to differ (q = 2, the rest in order) and needs the refused swap: key sort
    _a("a_swap01_refused", _G4, (2, 1, 3, 4), lambda d: _rand(d, 1_500_000, 47), "swap refused: many small slabs",
       {K32: 1}, swap=((1500, 900, 12), False)),
    # the other refused operands of test_device_aperm_first_two_axes_swapped: 66 666 and 128 571 nonzeros per slab at
    # 54 and 26 per row -- fine buckets below 512; no slab shapes; nothing for the general form to do: key sort.  The
    # last also as c(2,3,1): the 3-d form needs the same batched transposition
    _a("a_swap01_refused_4d", (1234, 777, 3, 2), (2, 1, 3, 4), lambda d: _rand(d, 400_000, 46), "swap refused: key sort", {K32: 1},
       swap=((1234, 777, 6), False)),
    _a("a_swap01_refused_tall", (5000, 300, 7), (2, 1, 3), lambda d: _rand(d, 900_000, 46), "swap refused: key sort", {K32: 1},
       swap=((5000, 300, 7), False)),
    _a("a_via_231_refused", (5000, 300, 7), (2, 3, 1), lambda d: _rand(d, 900_000, 46), "3-d form refused with its first step: key sort",
       {K32: 1}, swap=((5000, 300, 7), False)),
    # the same refusal on small slabs of a short axis: perm[1] == 1, dim[1] = 40 <= 1024, 869 nonzeros per slab
    _a("a_swap01_refused_to_slab", (700, 40, 23), (2, 1, 3), lambda d: _rand(d, 20_000, 46), "swap refused, slab form takes c(2,1,3)",
       {SLAB: 1}, swap=((700, 40, 23), False)),
    # ---- aperm: the slab form and its limits
    _a("a_slab_cap_8192", (512, 8, 32), (3, 1, 2), lambda d: _slab_skew(d, SLAB_CAP, 1000, 21), "largest slab exactly SLAB_CAP",
       {SLAB: 1}, arena="slab", check=_slabs(SLAB_CAP)),
    _a("a_slab_cap_8193", (512, 8, 32), (3, 1, 2), lambda d: _slab_skew(d, SLAB_CAP + 1, 1000, 21),
       "largest slab SLAB_CAP + 1: refused on seeing the data; general needs the swap of 512 x 32 x 8, refused: key sort",
       {REFUSED: 1, K32: 1}, swap=((512, 32, 8), False), check=_slabs(SLAB_CAP + 1)),
    _a("a_slab_dq_1024", (40, 6, 1024), (3, 1, 2), lambda d: _rand(d, 12_000, 22), "dim[perm[0]] == 1024: the slab's LDS tables full",
       {SLAB: 1}, check=_slabs()),
    _a("a_slab_dq_1025", (40, 6, 1025), (3, 1, 2), lambda d: _rand(d, 12_000, 22), "dim[perm[0]] == 1025: not a slab shape",
       {K32: 1}, swap=((40, 1025, 6), False)),
    _a("a_slab_mean_7372", (1024, 2, 16), (3, 1, 2), lambda d: _slab_skew(d, 7372, 7372, 23), "nnz / nslab == SLAB_CAP * 9 / 10",
       {SLAB: 1}, check=_slabs(7372, SLAB_CAP * 9 // 10)),
    _a("a_slab_mean_7373", (1024, 2, 16), (3, 1, 2), lambda d: _slab_skew(d, 7373, 7373, 23), "nnz / nslab one over: not a slab shape",
       {K32: 1}, swap=((1024, 16, 2), False), check=_slabs(7373, SLAB_CAP * 9 // 10 + 1)),
    # c(3, 4, 1, 2): general with the slab form for steps A + B (slab_first), one slab of 12 000 refuses at run time
    # inside the rest of the workspace: that step takes the key sort, step C moves whole leaves
    _a("a_slab_refused_inside_general", (3000, 4, 6, 5), (3, 4, 1, 2), _refused_inside_general, "slab refused inside general",
       {GEN: 1, REFUSED: 1, K32: 1, LP: 1}, swap=((3000, 6, 20), False), arena="slab refused inside general",
       check=lambda dim, perm, lin: _slabs(12_000, 4600)(dim, (3, 1, 2, 4), lin)),
    # ---- aperm: 3-d through an intermediate (the first step is launched directly: no first_two_axes_swapped count)
    _a("a_via_231", (1500, 2500, 3), (2, 3, 1), lambda d: _rand(d, 225_000, 24), "c(2,1,3) then c(1,3,2)", {VIA: 1, LP: 1},
       swap=((1500, 2500, 3), True), arena="via 3-d"),
    _a("a_via_321", (1500, 2500, 3), (3, 2, 1), lambda d: _rand(d, 225_000, 24), "c(2,1,3) then c(3,1,2) by the slab form (1500 slabs of 150)",
       {VIA: 1, SLAB: 1}, swap=((1500, 2500, 3), True)),
    # dim[2] on both sides of 1024: one nonzero per leaf makes 2 x 1024 slabs the batched form takes.  1024: via; its
    # second step is no slab shape (two slabs of 524 288): key sort.  1025: general, all three steps.
    _a("a_via_321_dim3_1024", (2, 1024, 1024), (3, 2, 1), lambda d: _one_per_column(d, 25), "c(3,2,1), dim[2] == 1024: via",
       {VIA: 1, K32: 1}, swap=((2, 1024, 1024), True)),
    _a("a_via_321_dim3_1025", (2, 1024, 1025), (3, 2, 1), lambda d: _one_per_column(d, 25), "c(3,2,1), dim[2] == 1025: general",
       {GEN: 1, LP: 2, SW: 1}, swap=((2, 1025, 1024), True)),
    # ---- aperm: the general permutations of test_device_aperm_general_permutations
    # (1500 x 900 x 12 slabs is refused by the batched form, see a_swap01_refused; 125 000 per slab is no slab shape)
    _a("a_general_2413", _G4, (2, 4, 1, 3), lambda d: _rand(d, 1_500_000, 47), "q = 2, swap refused, no slab_first: key sort", {K32: 1},
       swap=((1500, 900, 12), False)),
    # perm[1] == 1 and dim[2] = 4: a slab shape by its extents, but 1.5e6 / 2700 slabs = 555 per slab -- taken
    _a("a_general_3142", _G4, (3, 1, 4, 2), lambda d: _rand(d, 1_500_000, 47), "the slab form on its own", {SLAB: 1},
       check=_slabs(mean=555)),
    # q = 3 of 900: A moves leaves, B swaps 1500 x 900 x 12 -- refused; slab_first: 125 000 per slab -- no: key sort
    _a("a_general_3241", _G4B, (3, 2, 4, 1), lambda d: _rand(d, 1_500_000, 47), "q = 3, swap refused: key sort", {K32: 1},
       swap=((1500, 900, 12), False)),
    _a("a_general_3421", _G4B, (3, 4, 2, 1), lambda d: _rand(d, 1_500_000, 47), "q = 3, swap refused: key sort", {K32: 1},
       swap=((1500, 900, 12), False)),
    # five axes, q = 4 of 700: B would swap 1200 x 700 x 30 -- refused (40 000 per slab, fine buckets of 133); 40 000
    # per slab is no slab shape either, on its own (c(4,1,2,3,5)) or as slab_first: key sort
    _a("a_general_45132", _G5, (4, 5, 1, 3, 2), lambda d: _rand(d, 1_200_000, 47), "five axes, swap refused: key sort", {K32: 1},
       swap=((1200, 700, 30), False)),
    _a("a_general_41235", _G5, (4, 1, 2, 3, 5), lambda d: _rand(d, 1_200_000, 47), "perm[1] == 1, slabs too long, swap refused: key sort",
       {K32: 1}, swap=((1200, 700, 30), False)),
    # the composed form with the batched transposition as step B (none of the shapes above reaches it):
    # A c(1,3,2,4) moves leaves, B swaps 1500 x 2500 x 4, C moves leaves; without A (q = 2); without C (rest in order)
    _a("a_general_three_steps", _G3S, (3, 2, 4, 1), lambda d: _rand(d, 300_000, 46), "general: leaves, swap, leaves",
       {GEN: 1, LP: 2, SW: 1}, swap=((1500, 2500, 4), True), arena="general, bucketed step"),
    _a("a_general_no_first_step", (1500, 2500, 2, 2), (2, 4, 1, 3), lambda d: _rand(d, 300_000, 46), "general, q = 2: swap, leaves",
       {GEN: 1, SW: 1, LP: 1}, swap=((1500, 2500, 4), True)),
    _a("a_general_no_last_step", _G3S, (3, 1, 2, 4), lambda d: _rand(d, 300_000, 46), "general, dim[perm[0]] = 2500 > 1024: leaves, swap",
       {GEN: 1, LP: 1, SW: 1}, swap=((1500, 2500, 4), True)),
    # slab_first: 450 per slab -- A + B by the slab form in one step, then C
    _a("a_general_2431", (300, 6, 5, 4), (2, 4, 3, 1), lambda d: _rand(d, 9000, 47), "general, slab form first, then whole leaves",
       {GEN: 1, SLAB: 1, LP: 1}, swap=((300, 6, 20), False)),
    _a("a_general_4321", (300, 6, 5, 4), (4, 3, 2, 1), lambda d: _rand(d, 9000, 47), "general, slab form first, then whole leaves",
       {GEN: 1, SLAB: 1, LP: 1}, swap=((300, 4, 30), False), arena="general"),
    # q = 5 of 3: the array after step B has 40 * 6000 = 240 000 leaves, more than 2 * nnz + 1024: the general form
    # declines (its leaf-preserving steps would cost more than sorting the nonzeros): key sort
    _a("a_general_53142", (40, 30, 20, 10, 3), (5, 3, 1, 4, 2), lambda d: _rand(d, 50_000, 47), "five axes, too many leaves: key sort",
       {K32: 1}),
    # ---- aperm: leaf-preserving
    _a("a_leaf_132", (700, 40, 23), (1, 3, 2), lambda d: _rand(d, 20_000, 44), "whole leaves move", {LP: 1}, arena="leaf-preserving"),
    _a("a_leaf_1423", (300, 6, 5, 4), (1, 4, 2, 3), lambda d: _rand(d, 9000, 44), "whole leaves move, 4-d", {LP: 1}),
    _a("a_leaf_extent_1", (64, 50, 1), (1, 3, 2), lambda d: _rand(d, 1500, 44), "an extent of 1", {LP: 1}),
    # ---- aperm: the 32-bit key sort on its own: dim[1] > 1024 (no slab shape), slabs too thin for the batched form,
    # nothing left for the general form to do differently
    _a("a_key_sort_32", (300, 1100, 3), (2, 1, 3), lambda d: _rand(d, 5000, 26), "key_sort_32", {K32: 1},
       swap=((300, 1100, 3), False), arena="key_sort_32"),
    _a("a_no_nonzeros", (900, 30, 16), (3, 1, 2), lambda d: np.zeros(0, dtype=np.int64), "0 nonzeros: a memset, no route", {}),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALL = 2_000_000          # cases under this many dense cells check the reference against np.transpose


@functools.lru_cache(maxsize=None)
def pattern(name):
    c = BY_NAME[name]
    lin = np.asarray(c["build"](c["dim"]), dtype=np.int64)
    assert lin.ndim == 1 and (np.diff(lin) > 0).all() and (lin.size == 0 or (lin[0] >= 0 and lin[-1] < prod(c["dim"])))
    lin.setflags(write=False)
    return lin


def csc_of(dim, lin):
    """(col_ptr int64, row_idx int32) of the pattern in the device layout: leaves = prod(dim[1:])"""
    nleaf = prod(dim[1:])
    cp = np.zeros(nleaf + 1, dtype=np.int64)
    np.cumsum(np.bincount(lin // dim[0], minlength=nleaf), out=cp[1:])
    return cp, (lin % dim[0]).astype(np.int32)


# ---------------------------------------------------------------------------
# the reference: plain numpy, 64-bit
# ---------------------------------------------------------------------------
def ref_t(dim, lin):
    """t(): a stable argsort of the row indices.  (col_ptr, row_idx, order): entry i of the result is entry order[i]."""
    row, col = lin % dim[0], lin // dim[0]
    order = np.argsort(row, kind="stable")
    cp = np.zeros(dim[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=dim[0]), out=cp[1:])
    return cp, col[order].astype(np.int32), order


def ref_aperm(dim, perm, lin):
    """aperm(x, perm) (1-based): a stable sort of the linear index in the permuted array, int64."""
    assert prod(dim) < 2 ** 63
    new_dim = tuple(dim[p - 1] for p in perm)
    rest, coord = lin.copy(), []
    for d in dim:
        coord.append(rest % d)
        rest //= d
    new_lin, mul = np.zeros(lin.size, dtype=np.int64), 1
    for p in perm:
        new_lin += coord[p - 1] * mul
        mul *= dim[p - 1]
    order = np.argsort(new_lin, kind="stable")
    s = new_lin[order]
    nleaf = prod(new_dim[1:])
    cp = np.zeros(nleaf + 1, dtype=np.int64)
    np.cumsum(np.bincount(s // new_dim[0], minlength=nleaf), out=cp[1:])
    return cp, (s % new_dim[0]).astype(np.int32), order


@functools.lru_cache(maxsize=None)
def reference(name):
    c, lin = BY_NAME[name], pattern(name)
    out = ref_t(c["dim"], lin) if c["perm"] is None else ref_aperm(c["dim"], c["perm"], lin)
    for a in out:
        a.setflags(write=False)
    return out


def dense_of(dim, lin, val):
    a = np.zeros(prod(dim), dtype=val.dtype)
    a[lin] = val
    return a.reshape(dim, order="F")


def check_reference_against_numpy(name):
    """np.transpose of the dense array (tracer values: every cell is told apart) gives the same CSC arrays"""
    c, lin = BY_NAME[name], pattern(name)
    perm = c["perm"] or (2, 1)
    val = values("tracer", "double", lin)
    want = np.transpose(dense_of(c["dim"], lin, val), [p - 1 for p in perm])
    wl = np.flatnonzero(want.reshape(-1, order="F"))
    wcp, wri = csc_of(want.shape, wl)
    cp, ri, order = reference(name)
    assert np.array_equal(cp, wcp) and np.array_equal(ri, wri)
    assert np.array_equal(val[order], want.reshape(-1, order="F")[wl])


# ---------------------------------------------------------------------------
# value palettes
# ---------------------------------------------------------------------------
def values(palette, dtype, lin):
    """tracer: the value encodes the old position (doubles: old linear index + 1, exact below 2^53; integers and
    logicals -- the kernels copy a logical's 32 bits like an integer's -- that mod 2^31 - 2, + 1: never 0, never NA).
    specials: the values no float comparison tells apart, cycled over the input positions with an odd period, so that
    each lands in the first and in the last slot of some column's run (test_transpose_cases_cpu.py checks it)."""
    if palette == "tracer":
        if dtype == "double":
            assert lin.size == 0 or lin[-1] + 1 < 2 ** 53
            return (lin + 1).astype(np.float64)
        return (lin % (2 ** 31 - 2) + 1).astype(np.int32)
    table = {"double": SPECIALS_F64, "integer": SPECIALS_I32, "logical": SPECIALS_LGL}[dtype]
    return table[np.arange(lin.size) % len(table)]


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.int64) if v.dtype == np.float64 else v.view(np.int32)


def compare(got, want, what=""):
    """got, want: (col_ptr, row_idx, val, logical flag).  Identity: pointers and indices equal, values equal as bits,
    dtype and flag kept.  Names the first entry that differs and, for a tracer value, where it came from."""
    gcp, gri, gv, glg = got
    wcp, wri, wv, wlg = want
    assert gcp.dtype == np.int64 and gri.dtype == np.int32, f"{what}: index dtypes {gcp.dtype}, {gri.dtype}"
    assert gv.dtype == wv.dtype, f"{what}: value dtype {gv.dtype}, want {wv.dtype}"
    assert bool(glg) == bool(wlg), f"{what}: logical flag {glg}, want {wlg}"
    assert gcp.shape == wcp.shape and gri.shape == wri.shape and gv.shape == wv.shape, f"{what}: sizes differ"
    if not np.array_equal(gcp, wcp):
        j = int(np.flatnonzero(gcp != wcp)[0])
        raise AssertionError(f"{what}: col_ptr[{j}] = {gcp[j]}, want {wcp[j]}")
    bad = (gri != wri) | (bits(gv) != bits(wv))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        leaf = int(np.searchsorted(wcp, i, side="right") - 1)
        raise AssertionError(f"{what}: {int(bad.sum())} entries differ, first at {i} (leaf {leaf}): row {gri[i]} value "
                             f"{gv[i]!r} (bits {int(bits(gv)[i]):#x}), want row {wri[i]} value {wv[i]!r} "
                             f"(bits {int(bits(wv)[i]):#x})")


NP_DTYPE = {"double": np.float64, "integer": np.int32, "logical": np.int32}


def expected(name, dtype, palette):
    """(col_ptr, row_idx, val, logical flag) the call must produce, and the operand's values"""
    lin = pattern(name)
    cp, ri, order = reference(name)
    val = values(palette, dtype, lin)
    assert val.dtype == NP_DTYPE[dtype]
    return (cp, ri, val[order], dtype == "logical"), val
