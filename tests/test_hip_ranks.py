"""colRanks() / rowRanks() on the device (kernels_ranks.hip: the compact form -- a rank per stored value and a rank per
column for its zeros -- by three forms chosen per column) against the plain definition on the dense column and against
the host statement of sparsearray_amd/api.py, at tolerance 0: ranks are integers and (2L + E + 1) * 0.5 is exact.
Operands of 2^31 nonzeros or more are not tested: ranks run through the same 64-bit positions, no full-size case here."""
import numpy as np
import pytest

from helpers import assert_equal
from sparsearray_amd import NA_integer, NA_real, SVT_SparseArray, SparseArrayError, is_NA_real
from test_ranks_cpu import (TIES, check_argument_errors, check_known_values, check_ranks_on_cases, check_zero_extents,
                            dense_colranks)

pytestmark = pytest.mark.gpu


def _dtype(ties):
    return np.float64 if ties == "average" else np.int32


def _csc(dense, keep=None):
    """(col_ptr, row_idx, val) of a dense matrix, storing the cells of ``keep`` (default: the nonzero ones)."""
    keep = (dense != 0) | np.isnan(dense) if keep is None else keep
    cp = np.zeros(dense.shape[1] + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=0), out=cp[1:])
    ri = np.concatenate([np.flatnonzero(keep[:, j]) for j in range(dense.shape[1])]).astype(np.int32)
    val = np.concatenate([dense[keep[:, j], j] for j in range(dense.shape[1])])
    return cp, ri, val


def expand(nrow, cp, ri, rank_nz, zero_rank):
    """The dense (nrow, ncol) ranks from the compact form."""
    ncol = len(cp) - 1
    out = np.empty((nrow, ncol), dtype=rank_nz.dtype, order="F")
    for j in range(ncol):
        out[:, j] = zero_rank[j]
        out[ri[cp[j]:cp[j + 1]], j] = rank_nz[cp[j]:cp[j + 1]]
    return out


def _compact(A, ties, **kw):
    from sparsearray_amd.device import colranks
    rank_nz, zero_rank = colranks(A, ties_method=ties, **kw)
    return rank_nz.cpu().numpy(), zero_rank.cpu().numpy()


def _check_operand(hip, dense, type_, what, rows=False):
    """hip.colRanks (preserved shape), and with ``rows`` hip.rowRanks of the transposed operand, against the dense rule
    for the four methods."""
    stored = dense if type_ == "double" else np.where(np.isnan(dense), NA_integer, dense).astype(np.int32)
    x = SVT_SparseArray.from_dense(np.asfortranarray(stored), type_)
    xt = SVT_SparseArray.from_dense(np.asfortranarray(stored.T), type_) if rows else None
    for ties in TIES:
        want = dense_colranks(dense, ties)
        got = hip.colRanks(x, ties_method=ties, preserve_shape=True)
        assert got.dtype == _dtype(ties) and got.shape == dense.shape
        assert_equal(got, want, tol=0, strict_na=True, what=f"{what} {type_} {ties}")
        if rows:
            got = hip.rowRanks(xt, ties_method=ties)
            assert got.dtype == _dtype(ties) and got.shape == dense.T.shape
            assert_equal(got, want.T, tol=0, strict_na=True, what=f"{what} {type_} {ties} rows")


def test_hip_ranks_are_the_dense_rule(hip):
    check_ranks_on_cases(hip, "hip")


def test_hip_ranks_against_host_statement(hip, oracle):
    check_ranks_on_cases(hip, "hip vs oracle", reference=oracle)


def test_hip_ranks_known_values(hip):
    check_known_values(hip)


def _limits():
    """The last stored length of form 0 and of form 1, through svt_dev_colranks_form."""
    from sparsearray_amd.device import _lib, colranks_form_limits
    f0, f1 = colranks_form_limits()
    form = _lib().svt_dev_colranks_form
    assert [form(n) for n in (0, 1, f0, f0 + 1, f1, f1 + 1, 1 << 31)] == [0, 0, 0, 1, 1, 2, 2]
    assert f1 >= 10_500                                  # every column of BASELINE config 2 is sorted in LDS
    return f0, f1


@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_ranks_route_boundaries(hip, type_):
    """Columns whose stored lengths are each form's last, the next form's first and one beyond, in one operand,
    interleaved with empty columns: every list is built in one call."""
    f0, f1 = _limits()
    lens = [f0, 0, f0 + 1, f1 + 1, 0, f0 + 2, f1, 1, f1 + 2, 0, f0 - 1, f1 - 1, 2]
    nrow = f1 + 40
    rng = np.random.default_rng(81)
    dense = np.zeros((nrow, len(lens)))
    for j, n in enumerate(lens):
        v = np.round(rng.normal(size=n) * [2, 40, 1000][j % 3])           # heavy, moderate and few ties
        v[v == 0] = 1
        dense[rng.choice(nrow, n, replace=False), j] = v
    if type_ == "double":
        dense[dense != 0] += 0.25
        dense[np.flatnonzero(dense[:, 3])[:5], 3] = np.nan
        dense[np.flatnonzero(dense[:, 0])[:3], 0] = [np.inf, -np.inf, NA_real]
    else:
        dense[np.flatnonzero(dense[:, 3])[:5], 3] = np.nan
    assert [int(((dense[:, j] != 0) | np.isnan(dense[:, j])).sum()) for j in range(len(lens))] == lens
    _check_operand(hip, dense, type_, "boundaries", rows=True)


def _form1_operand(type_):
    """5000-row columns, fills from 30 % to 100 %, all sorted in LDS: more than 1024 equal values, keys that differ only
    in low mantissa bits, 1e200-scale values, duplicates on both sides of zero, +-Inf and missing values."""
    rng = np.random.default_rng(82)
    nrow = 5000
    cols = []
    for j in range(40):
        fill = [1.0, 0.97, 0.8, 0.6, 0.3][j % 5]
        m = rng.random(nrow) < fill
        kind = (j // 5) % 4
        if kind == 0:                                                           # more than 1024 equal values
            v = rng.choice([-1.5, 1.5, 7.0], nrow) if j % 2 else np.full(nrow, 2.0)
        elif kind == 1:                                                         # low mantissa bits
            v = (1.0 + rng.integers(0, 1 << 12, nrow) * 2.0 ** -52) * rng.choice([-1.0, 1.0], nrow)
        elif kind == 2:                                                         # 1e200 scale
            v = rng.normal(size=nrow) * 1e200
        else:                                                                   # duplicates on both sides of zero
            v = rng.integers(-3, 6, nrow).astype(np.float64)
        if type_ == "integer":
            v = np.round(v * (1 if kind == 3 else 1000)).clip(-2e9, 2e9) if kind != 1 else rng.integers(-2, 3, nrow) * 1.0
        col = np.zeros(nrow)
        col[m] = v[m]
        cols.append(col)
    a = np.stack(cols, axis=1)
    a[7, 3] = np.nan; a[:300, 11] = np.nan; a[9, 12] = np.nan
    if type_ == "double":
        a[17, 5] = np.inf; a[18, 5] = -np.inf; a[19, 6] = NA_real; a[20:30, 15] = np.inf
    return a


@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_ranks_sorted_in_lds(hip, type_):
    f0, f1 = _limits()
    a = _form1_operand(type_)
    stored = ((a != 0) | np.isnan(a)).sum(axis=0)
    assert (stored > f0).all() and (stored <= f1).all() and stored.max() == a.shape[0]
    _check_operand(hip, a, type_, "form 1")


@pytest.mark.parametrize("type_", ["double", "integer"])
def test_hip_ranks_long_columns(hip, type_):
    """300 000-row columns (the library's sort, lower and upper bounds in the sorted segments), doubles and integers with
    heavy ties, next to a column of form 1 and an empty one."""
    f0, f1 = _limits()
    rng = np.random.default_rng(83)
    nrow = 300_000
    tall = np.zeros((nrow, 5))
    tall[:, 0] = rng.normal(size=nrow) + 0.75
    tall[:, 1] = np.round(rng.normal(size=nrow), 1)
    tall[:, 2] = rng.integers(-2, 3, nrow)
    tall[rng.random(tall.shape) < 0.2] = 0.0
    tall[rng.choice(nrow, 3000, replace=False), 3] = np.round(rng.normal(size=3000) * 3)       # form 1
    if type_ == "integer":
        tall = np.round(tall * 10)
    tall[5, 0] = np.nan; tall[6:9, 2] = np.nan
    assert ((tall[:, :3] != 0).sum(axis=0) > f1).all()
    _check_operand(hip, tall, type_, "tall")


def test_device_colranks_stored_zeros_compact_form(hip):
    """Stored 0.0 and -0.0 get the zeros' rank in every form; a column without any zero has zero_rank NA; the compact
    form expanded is the dense rule; two calls give the same bits.  The long column holds 40 000 of 50 000 cells with
    the values 0..5."""
    from sparsearray_amd.device import DeviceCSC
    f0, f1 = _limits()
    rng = np.random.default_rng(84)
    nrow = 50_000
    assert f1 < 40_000 <= nrow
    dense = np.zeros((nrow, 6))
    keep = np.zeros(dense.shape, dtype=bool)
    for j, n in enumerate([40_000, 2000, 60, nrow, 0, 5]):
        rows = rng.choice(nrow, n, replace=False)
        keep[rows, j] = True
        v = rng.integers(0, 6, n).astype(np.float64) * ([1, -1, 1, 1, 1, 0][j])
        v[(v == 0) & (rng.random(n) < 0.5)] = -0.0
        dense[rows, j] = v
    dense[keep[:, 3], 3] += 1.0                          # column 3: every cell stored and none a zero
    cp, ri, val = _csc(dense, keep)
    assert (val == 0).sum() > 6000 and np.signbit(val[val == 0]).any() and not np.signbit(val[val == 0]).all()
    A = DeviceCSC.from_host(nrow, cp, ri, val)
    for ties in TIES:
        rank_nz, zero_rank = _compact(A, ties)
        assert rank_nz.dtype == _dtype(ties) and zero_rank.dtype == _dtype(ties)
        again = _compact(A, ties)
        assert rank_nz.tobytes() == again[0].tobytes() and zero_rank.tobytes() == again[1].tobytes(), ties
        want = dense_colranks(dense, ties)
        assert_equal(expand(nrow, cp, ri, rank_nz, zero_rank), want, tol=0, strict_na=True, what=f"compact {ties}")
        for j in range(6):                               # a stored zero carries the column's zero rank
            z = val[cp[j]:cp[j + 1]] == 0
            assert (rank_nz[cp[j]:cp[j + 1]][z] == zero_rank[j]).all()
        na = is_NA_real(zero_rank) if ties == "average" else zero_rank == NA_integer
        assert list(na) == [False, False, False, True, False, False], ties
        # host level on the same matrix (its zeros not stored): the same dense result
        x = SVT_SparseArray.from_dense(np.asfortranarray(dense), "double")
        assert_equal(hip.colRanks(x, ties_method=ties, preserve_shape=True), want, tol=0, strict_na=True,
                     what=f"compact vs dense {ties}")


def _resident_mixed():
    """Columns of all three forms, the long ones at the ends and in the middle."""
    from sparsearray_amd.device import DeviceCSC, colranks_form_limits
    f1 = colranks_form_limits()[1]
    rng = np.random.default_rng(85)
    nrow = f1 + 3000
    lens = [f1 + 100, 50, 3000, 0, f1 + 2000, 200, f1 + 1]
    dense = np.zeros((nrow, len(lens)))
    for j, n in enumerate(lens):
        dense[rng.choice(nrow, n, replace=False), j] = np.round(rng.normal(size=n) * 50) + 0.5
    cp, ri, val = _csc(dense)
    long_cols = [j for j, n in enumerate(lens) if n > f1]
    return DeviceCSC.from_host(nrow, cp, ri, val), dense, cp, ri, long_cols, sum(lens[j] for j in long_cols)


@pytest.mark.parametrize("ties", ["max", "average", "dense"])
def test_device_colranks_stays_inside_its_workspace(hip, ties):
    """The advertised size is enough at an odd address inside a 0xA5 arena, and nothing outside it is touched; one byte
    fewer than the size for no long column at all is an error."""
    import torch
    from sparsearray_amd.device import _lib, colranks, colranks_long_nnz
    A, dense, cp, ri, long_cols, long_nnz = _resident_mixed()
    assert colranks_long_nnz(A) == long_nnz
    nbytes = _lib().svt_dev_colranks_ws_bytes(A.ncol, long_nnz)
    floor = _lib().svt_dev_colranks_ws_bytes(A.ncol, 0)
    assert 0 < floor < nbytes
    pad = 519
    arena = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = arena[pad:pad + nbytes]
    rank_nz, zero_rank = _compact(A, ties, ws=ws)
    assert_equal(expand(A.nrow, cp, ri, rank_nz, zero_rank), dense_colranks(dense, ties), tol=0, strict_na=True,
                 what=f"arena {ties}")
    assert bool((arena[:pad] == 0xA5).all()) and bool((arena[pad + nbytes:] == 0xA5).all())
    with pytest.raises(SparseArrayError, match="svt_dev_colranks: workspace too small"):
        colranks(A, ties_method=ties, ws=ws[:floor - 1])


@pytest.mark.parametrize("ties", ["max", "average"])
def test_device_colranks_flag_on_a_short_workspace(hip, ties):
    """A workspace made for fewer long nonzeros than the operand holds: the flag is set (device.colranks raises), the
    long columns' outputs are untouched and the other columns are answered."""
    import torch
    from sparsearray_amd.device import _lib, colranks
    A, dense, cp, ri, long_cols, long_nnz = _resident_mixed()
    dt = torch.float64 if ties == "average" else torch.int32
    want = dense_colranks(dense, ties)
    for given in (0, long_nnz // 2):
        ws = torch.empty(_lib().svt_dev_colranks_ws_bytes(A.ncol, given), dtype=torch.uint8, device="cuda")
        rank_nz = torch.full((A.nnz,), -7, dtype=dt, device="cuda")
        zero_rank = torch.full((A.ncol,), -7, dtype=dt, device="cuda")
        with pytest.raises(SparseArrayError, match="fewer long nonzeros"):
            colranks(A, ties_method=ties, rank_nz=rank_nz, zero_rank=zero_rank, ws=ws)
        rn, rz = rank_nz.cpu().numpy(), zero_rank.cpu().numpy()
        for j in range(A.ncol):
            seg = rn[cp[j]:cp[j + 1]]
            if j in long_cols:
                assert (seg == -7).all() and rz[j] == -7, (given, j)
            else:
                assert rz[j] == want[:, j][dense[:, j] == 0][0] and (seg == want[ri[cp[j]:cp[j + 1]], j]).all(), (given, j)
    # and the flag is cleared again by a call that has room
    rank_nz, zero_rank = _compact(A, ties)
    assert_equal(expand(A.nrow, cp, ri, rank_nz, zero_rank), want, tol=0, strict_na=True, what="after the flag")


def test_hip_ranks_extents_and_errors(hip):
    check_zero_extents(hip)
    check_argument_errors(hip)
    # the library's own checks (what a caller of the C ABI meets)
    x = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3, 4)), "double")
    x3 = SVT_SparseArray((2, 2, 2), "double", [None] * 4)
    na = SVT_SparseArray.from_dense(np.asfortranarray(np.eye(3)), "double", na_background=True)
    with pytest.raises(SparseArrayError, match=r"the colRanks\(\) method for SparseArray objects only supports 2D"):
        hip.SparseArray_Call("C_colRanks_SVT", x3, "max", False)
    with pytest.raises(SparseArrayError, match=r"the rowRanks\(\) method for SparseArray objects only supports 2D"):
        hip.SparseArray_Call("C_rowRanks_SVT", x3, "max")
    with pytest.raises(SparseArrayError, match=r"colRanks\(\) is not supported on NaArray objects"):
        hip.SparseArray_Call("C_colRanks_SVT", na, "max", False)
    with pytest.raises(SparseArrayError, match=r"colRanks\(\) is not supported on NaArray objects"):
        hip.SparseArray_Call("C_rowRanks_SVT", na, "max")
    for bad in ("first", "last", "random", 4, -1):
        with pytest.raises(SparseArrayError, match="'ties.method' must be \"max\", \"average\", \"min\" or \"dense\""):
            hip.SparseArray_Call("C_colRanks_SVT", x, bad, False)
        with pytest.raises(SparseArrayError, match="'ties.method' must be \"max\", \"average\", \"min\" or \"dense\""):
            hip.SparseArray_Call("C_rowRanks_SVT", x, bad)
    got = hip.SparseArray_Call("C_colRanks_SVT", x, "min", True)
    assert got.dtype == np.int32 and [list(r) for r in got] == [[3, 1, 1, 1], [1, 3, 1, 1], [1, 1, 3, 1]]
    got = hip.SparseArray_Call("C_rowRanks_SVT", x, 1)
    assert got.dtype == np.float64 and [list(r) for r in got] == [[4.0, 2.0, 2.0, 2.0], [2.0, 4.0, 2.0, 2.0],
                                                                  [2.0, 2.0, 4.0, 2.0]]
    x0 = SVT_SparseArray((0, 3), "double", [None] * 3)
    assert hip.SparseArray_Call("C_colRanks_SVT", x0, "max", False).shape == (3, 0)
    assert hip.SparseArray_Call("C_rowRanks_SVT", x0, "max").shape == (0, 3)
    from sparsearray_amd.device import _lib
    assert _lib().svt_dev_colranks_ws_bytes(10, 1 << 32) == 0           # 2^32 long nonzeros or more: not offered
