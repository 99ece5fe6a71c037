"""Host-level entry points over a device list (svt_set_devices, include/svt_hip.h) on the GPU.

On one MI355X the lists repeat device 0 ({0,0}, {0,0,0}, {0}*8): every shard has its own host thread, staging
buffers and device buffers, so the row blocks, leaf ranges, reduce-scatter and status handling all run; only the
copies between distinct devices do not (test_distinct_devices_match_repeated_ordinals needs two GPUs).
Every case runs in a child process of its own under a time limit (the list is process-wide state).
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = {"x2": [0, 0], "x3": [0, 0, 0], "x8": [0] * 8}


def _child(name, *args, timeout=600):
    env = dict(os.environ)
    env.pop("SVT_SHARD_REFUSE", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), name, *map(str, args)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"{name} {args}: rc {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    assert "__CASE_OK__" in p.stdout, p.stdout[-3000:]


# ---------------------------------------------------------------------------------------------------------------
# pytest side
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lst", sorted(LISTS))
def test_golden_cases_through_a_sharded_session(lst):
    _child("golden", lst)


@pytest.mark.gpu
@pytest.mark.parametrize("lst", sorted(LISTS))
def test_row_sharded_products_mid_size(lst):
    _child("products", lst)


@pytest.mark.gpu
@pytest.mark.parametrize("lst", sorted(LISTS))
def test_column_sharded_stats_and_rowsum(lst):
    _child("colstats", lst)


@pytest.mark.gpu
def test_full_size_config_2a_four_shards():
    _child("full_size", timeout=900)


@pytest.mark.gpu
def test_device_list_errors_refusals_and_leaks():
    _child("errors")


@pytest.mark.gpu
def test_distinct_devices_match_repeated_ordinals():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    _child("distinct")


# ---------------------------------------------------------------------------------------------------------------
# child side
# ---------------------------------------------------------------------------------------------------------------
def _session(devs=None, min_nnz=0):
    import sparsearray_amd
    from sparsearray_amd import _hip
    hip = sparsearray_amd.hip_session()
    _hip.set_shard_min_nnz(min_nnz)
    if devs is not None:
        _hip.set_devices(devs)
        assert _hip.get_devices() == list(devs)
    return hip, _hip


def _random_svt(nrow, ncol, density, seed, kind="double"):
    from helpers import random_csc
    from sparsearray_amd import SVT_SparseArray
    cp, ri, v = random_csc(nrow, ncol, density, seed)
    if kind == "integer":
        rng = np.random.default_rng(seed + 1)
        v = rng.integers(-9, 10, size=len(ri)).astype(np.int32)
        v[v == 0] = 3
    return SVT_SparseArray.from_csc((nrow, ncol), kind, cp, ri, v)


def _abs_svt(x):
    from sparsearray_amd import SVT_SparseArray
    cp, ri, v = x.to_csc()
    return SVT_SparseArray.from_csc(tuple(x.dim), x.type, cp, ri, np.abs(v))


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), f"{what}: not bit-identical"


def _within(cur, ref, scale, tol, what):
    cur, ref = np.asarray(cur, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert cur.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(cur)), f"{what}: non-finite cells differ"
    assert np.array_equal(np.isnan(ref), np.isnan(cur)), f"{what}: NaN cells differ"
    assert np.array_equal(cur[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), f"{what}: infinite cells differ"
    err = np.abs(cur[fin] - ref[fin])
    bound = tol * np.asarray(scale, dtype=np.float64)[fin]
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} cells off, worst {err.max():.3e}"


def case_golden(lst):
    from helpers import check_case, golden_cases
    hip, _ = _session(LISTS[lst])
    n = 0
    for case in golden_cases():
        fn = case["fn"]
        if not (fn in ("crossprod", "rowsum") or fn.startswith("col") or fn == "matmul"):
            continue
        for lacunar in (True, False):
            check_case(hip, case, lacunar=lacunar, gpu=True)
            n += 1
    assert n > 300, n


def case_products(lst):
    hip, H = _session()
    rng = np.random.default_rng(11)
    nrow, ncol, K = 200_000, 2_000, 64
    A = _random_svt(nrow, ncol, 0.01, seed=3)
    Y = rng.standard_normal((nrow, K))
    Ym = rng.standard_normal((ncol, K))                   # A %*% Ym
    Ai = _random_svt(nrow, ncol, 0.01, seed=5, kind="integer")
    Yi = rng.integers(-50, 51, size=(nrow, K)).astype(np.int32)
    Ymi = rng.integers(-50, 51, size=(ncol, K)).astype(np.int32)
    Yinf = Y.copy()
    Yinf[12_345, 7] = np.inf
    Yinf[150_000, 40] = -np.inf
    # one device: no svt_set_devices call, then {0}
    c1 = np.asarray(hip.crossprod(A, Y))
    m1 = np.asarray(hip.matmul(A, Ym))
    H.set_devices([0])
    _same_bits(hip.crossprod(A, Y), c1, "{0} vs no list: crossprod")
    _same_bits(hip.matmul(A, Ym), m1, "{0} vs no list: %*%")
    ci1 = np.asarray(hip.crossprod(Ai, Yi))
    mi1 = np.asarray(hip.matmul(Ai, Ymi))
    cinf1 = np.asarray(hip.crossprod(A, Yinf))
    scale_c = np.asarray(hip.crossprod(_abs_svt(A), np.abs(Y)))
    scale_m = np.asarray(hip.matmul(_abs_svt(A), np.abs(Ym)))
    # sharded
    H.set_devices(LISTS[lst])
    cs = np.asarray(hip.crossprod(A, Y))
    _within(cs, c1, scale_c, 1e-12, "crossprod(A, Y)")
    _same_bits(hip.crossprod(A, Y), cs, "crossprod, two calls")
    ms = np.asarray(hip.matmul(A, Ym))
    _within(ms, m1, scale_m, 1e-12, "A %*% Y")
    _same_bits(hip.matmul(A, Ym), ms, "%*%, two calls")
    _same_bits(hip.crossprod(Ai, Yi), ci1, "integer crossprod")
    _same_bits(hip.matmul(Ai, Ymi), mi1, "integer %*%")
    # y given by rows (crossprod(A, t(y)) form)
    ct = np.asarray(hip._crossprod2_SparseMatrix_matrix(A, np.asfortranarray(Y.T), transpose_y=True))
    _within(ct, c1, scale_c, 1e-12, "crossprod(A, t(Yt))")
    cinf = np.asarray(hip.crossprod(A, Yinf))
    assert (~np.isfinite(cinf1)).any()
    _within(cinf, cinf1, scale_c, 1e-12, "one Inf in Y")          # (finite cells: terms of the finite Y)


_OPS = ["anyNA", "countNAs", "any", "all", "min", "max", "sum", "prod", "mean", "centered_X2_sum", "var1", "sd1"]


def _stat_operands():
    from helpers import random_csc
    from sparsearray_amd import SVT_SparseArray, NA_real
    rng = np.random.default_rng(21)
    out = {}
    for name, dim in (("2d", (3000, 400)), ("3d", (500, 20, 30))):
        nl = int(np.prod(dim[1:]))
        cp, ri, v = random_csc(dim[0], nl, 0.05, seed=len(name) + nl)
        vd = v.copy()
        pick = rng.choice(len(vd), size=40, replace=False)
        vd[pick[:15]] = NA_real
        vd[pick[15:25]] = np.nan
        vd[pick[25:30]] = np.inf
        vi = rng.integers(-1000, 1000, size=len(v)).astype(np.int32)
        vi[vi == 0] = 7
        vi[pick[:15]] = np.iinfo(np.int32).min                 # NA_integer_
        vl = np.ones(len(v), dtype=np.int32)
        vl[pick[30:]] = 0
        vl[pick[:5]] = np.iinfo(np.int32).min
        out[name] = {t: SVT_SparseArray.from_csc(dim, t, cp, ri, vv)
                     for t, vv in (("double", vd), ("integer", vi), ("logical", vl))}
    return out


def _stat(hip, op, x, na_rm, dims):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = hip._colStats(op, x, na_rm=na_rm, dims=dims)
    return np.asarray(r), sorted(str(m.message) for m in w)


def _rowsum(hip, x, group):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r, _ = hip.rowsum(x, group)
    return np.asarray(r), sorted(str(m.message) for m in w)


def case_colstats(lst):
    from helpers import assert_equal
    from sparsearray_amd import SVT_SparseArray
    hip, H = _session([0])
    X = _stat_operands()
    calls = []
    for name, by_type in X.items():
        for dims in ((1,) if name == "2d" else (1, 2)):
            for op in _OPS:
                for na_rm in (False, True):
                    for t, x in by_type.items():
                        if op in ("any", "all") and t == "double":
                            continue
                        calls.append((name, dims, op, na_rm, t, x))
    ref = [_stat(hip, op, x, na_rm, dims) for (_, dims, op, na_rm, _, x) in calls]
    # rowsum: integer (overflow in the last columns: the last shard's) and double
    rng = np.random.default_rng(5)
    nrow, ncol = 4000, 300
    dense_i = np.where(rng.random((nrow, ncol)) < 0.05, rng.integers(-100, 100, (nrow, ncol)), 0).astype(np.int32)
    dense_i[:2, -1] = 2 ** 30 + 1000                            # rows 0 and 1: one group below -> overflow
    xi = SVT_SparseArray.from_dense(dense_i, type="integer")
    xi_ok = SVT_SparseArray.from_dense(np.where(np.arange(ncol) == ncol - 1, 0, dense_i).astype(np.int32),
                                       type="integer")
    xd = SVT_SparseArray.from_dense(np.where(dense_i != 0, rng.standard_normal((nrow, ncol)), 0.0), type="double")
    group = np.concatenate([[1, 1], rng.integers(1, 40, nrow - 2)]).astype(np.int32)
    r_i, r_i_ok, r_d = _rowsum(hip, xi, group), _rowsum(hip, xi_ok, group), _rowsum(hip, xd, group)
    assert r_i[1] and not r_i_ok[1], (r_i[1], r_i_ok[1])

    H.set_devices(LISTS[lst])
    for (name, dims, op, na_rm, t, x), (want, want_w) in zip(calls, ref):
        got, got_w = _stat(hip, op, x, na_rm, dims)
        what = f"{name} dims={dims} {op} na_rm={na_rm} {t}"
        assert got_w == want_w, f"{what}: warnings {got_w} vs {want_w}"
        if want.dtype == np.float64:
            assert_equal(got, want, tol=1e-6, what=what, strict_na=True)
        else:
            _same_bits(got, want, what)
    g = _rowsum(hip, xi, group)
    assert g[1] == r_i[1]
    _same_bits(g[0], r_i[0], "integer rowsum, overflow in the last columns")
    g = _rowsum(hip, xi_ok, group)
    assert not g[1]
    _same_bits(g[0], r_i_ok[0], "integer rowsum")
    g = _rowsum(hip, xd, group)
    assert_equal(g[0], r_d[0], tol=1e-6, what="double rowsum")


def case_full_size():
    import torch
    from sparsearray_amd import SVT_SparseArray, synth
    hip, H = _session([0])
    NROW, NCOL, DENS, K = 1_000_000, 10_000, 0.01, 128
    cp, ri, v = synth.random_device_csc(NROW, NCOL, DENS, seed=7, device="cuda")
    Yd = synth.random_dense(NROW, K, seed=107, device="cuda")          # (K, nrow): column-major nrow x K
    A = SVT_SparseArray.from_csc((NROW, NCOL), "double", cp.cpu().numpy(), ri.cpu().numpy(), v.cpu().numpy())
    Y = Yd.cpu().numpy().T
    one = np.asarray(hip.crossprod(A, Y))
    scale = np.asarray(hip.crossprod(_abs_svt(A), np.abs(Y)))
    H.set_devices([0, 0, 0, 0])
    got = np.asarray(hip.crossprod(A, Y))
    _within(got, one, scale, 1e-12, "config 2a, 4 shards vs one device")
    rng = np.random.default_rng(1)
    for c, k in zip(rng.integers(0, NCOL, 64), rng.integers(0, K, 64)):
        s, e = int(cp[c]), int(cp[c + 1])
        terms = v[s:e] * Yd[k, ri[s:e].long()]
        exact, mag = float(terms.sum()), float(terms.abs().sum())
        assert abs(got[c, k] - exact) <= 1e-12 * mag, (c, k, got[c, k], exact)
    del cp, ri, v, Yd
    torch.cuda.empty_cache()


def case_errors():
    import ctypes
    import torch
    from sparsearray_amd import SparseArrayUnsupported
    from sparsearray_amd._hip import HipBackendError
    hip, H = _session()
    assert H.get_devices() == [0]
    H.set_devices([0, 0])
    try:
        H.set_devices([0, 4096])
        raise AssertionError("an out-of-range ordinal was accepted")
    except HipBackendError as e:
        assert "out of range" in str(e)
    assert H.get_devices() == [0, 0]
    H.set_devices([])
    assert H.get_devices() == [0]
    try:
        H.set_devices([0] * 17)
        raise AssertionError("17 entries were accepted")
    except HipBackendError:
        pass
    assert H.get_devices() == [0]
    # a refusal in one shard refuses the call (the glue then runs the CPU body)
    H.set_devices([0, 0, 0])
    x = _random_svt(5000, 300, 0.02, seed=9)
    y = np.random.default_rng(2).standard_normal((5000, 16))
    group = (np.arange(5000) % 7 + 1).astype(np.int32)
    want = np.asarray(hip.crossprod(x, y))
    os.environ["SVT_SHARD_REFUSE"] = "2"
    for call in (lambda: hip.crossprod(x, y), lambda: hip.matmul(x, y[:300]), lambda: hip.colSums(x),
                 lambda: hip.rowsum(x, group)):
        try:
            call()
            raise AssertionError("a shard's refusal did not reach the caller")
        except SparseArrayUnsupported as e:
            assert "shard 2" in str(e)
    del os.environ["SVT_SHARD_REFUSE"]
    _same_bits(hip.crossprod(x, y), want, "after a refusal")
    # no leaks: device memory in use after 50 sharded calls is what it was
    lib = H.init()
    for _ in range(2):
        hip.crossprod(x, y); hip.matmul(x, y[:300]); hip.colSums(x); hip.rowsum(x, group)
    torch.cuda.synchronize()
    lib.svt_dev_pbc_trim()
    free0, _ = torch.cuda.mem_get_info()
    calls = (lambda: hip.crossprod(x, y), lambda: hip.matmul(x, y[:300]), lambda: hip.colSums(x),
             lambda: hip.rowsum(x, group))
    for i in range(50):
        calls[i % 4]()
    torch.cuda.synchronize()
    lib.svt_dev_pbc_trim()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 <= (4 << 20), f"{(free0 - free1) / 2**20:.1f} MiB more in use after 50 sharded calls"
    assert ctypes is not None


def case_distinct():
    hip, H = _session()
    x = _random_svt(60_000, 700, 0.01, seed=13)
    y = np.random.default_rng(3).standard_normal((60_000, 48))
    H.set_devices([0, 0])
    want_c, want_m, want_s = hip.crossprod(x, y), hip.matmul(x, y[:700]), hip.colSums(x)
    H.set_devices([0, 1])
    _same_bits(hip.crossprod(x, y), want_c, "{0,1} vs {0,0}: crossprod")
    _same_bits(hip.matmul(x, y[:700]), want_m, "{0,1} vs {0,0}: %*%")
    _same_bits(hip.colSums(x), want_s, "{0,1} vs {0,0}: colSums")


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("__CASE_OK__")
