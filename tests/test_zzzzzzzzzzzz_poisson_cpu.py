"""The random count arrays without a device: the numpy restatement (tests/poisson_cases.py) against the known answers of
Philox4x32-10, the rules header (sparsearray_amd/csrc/svt_random_rules.h, through tests/random_rules_main.cpp) against the
restatement, svt_poisson_ticks against the longdouble restatement and against the true CDF, every refusal the library
decides on the host, and every check of the Session methods, raised before any call."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import poisson_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_longdouble = pytest.mark.skipif(not pc.HAVE_LONGDOUBLE, reason="numpy.longdouble has no 63-bit mantissa here")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """requests -> answers of tests/random_rules_main.cpp, built with the host compiler"""
    exe = tmp_path_factory.mktemp("random_rules") / "random_rules"
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "random_rules_main.cpp")], check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:-1]
    return ask


@pytest.fixture(scope="module")
def lib():
    from sparsearray_amd._hip import load_library
    return load_library()


def _hex(v):
    return f"{int(np.asarray(v, dtype=np.float64).reshape(1).view(np.uint64)[0]):x}"


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def test_restatement_gives_the_known_answers():
    for ctr, key, want in pc.KNOWN_ANSWERS:
        got = pc.philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == want
    # vectorised: the three at once
    c = [np.array([k[0][i] for k in pc.KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)]
    for (ctr, key, want), row in zip(pc.KNOWN_ANSWERS, range(3)):
        got = pc.philox4x32_10(*[x[row:row + 1] for x in c], *key)
        assert tuple(int(w[0]) for w in got) == want


def test_header_gives_the_known_answers(rules):
    asked = ["philox " + " ".join(f"{w:x}" for w in ctr + key) for ctr, key, _ in pc.KNOWN_ANSWERS]
    assert rules(asked) == [" ".join(f"{w:08x}" for w in want) for _, _, want in pc.KNOWN_ANSWERS]


CELLS = [0, 1, 2, 3, 4095, 4096, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33, 2 ** 40 + 1, 2 ** 62 + 5]
CELL_SEEDS = [0, 1, 2 ** 32, 2 ** 32 + 7, 2 ** 63, 2 ** 64 - 1]


@needs_longdouble
def test_header_cell_to_value_is_the_restatement(rules):
    asked, want = [], []
    for lam in (pc.DEFAULT_LAMBDA, 1.0, 4.0, 1e-16, 0.0):
        for seed in CELL_SEEDS:
            u = pc.cell_uniform(seed, np.array(CELLS, dtype=np.uint64))
            v = pc.values(seed, np.array(CELLS, dtype=np.uint64), lam)
            for cell, uu, vv in zip(CELLS, u, v):
                asked.append(f"cell {seed:x} {cell:x} {_hex(lam)}")
                want.append(f"{int(np.float64(uu).view(np.uint64)):016x} {int(vv)}")
    assert rules(asked) == want


def test_uniforms_lie_in_the_unit_interval_and_pairs_share_a_block():
    cells = np.arange(0, 4096, dtype=np.uint64) + np.uint64(2 ** 32 - 2048)
    u = pc.cell_uniform(12345, cells)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.unique(u).size == u.size
    # the odd cell takes words 2 and 3 of the block of its even neighbour
    w = pc.philox4x32_10(np.uint64(2 ** 31 - 1024), 0, 0, 0, 12345, 0)
    x = (int(w[3]) << 32 | int(w[2])) >> 11
    assert u[1] == x * 2.0 ** -53


# ---------------------------------------------------------------------------
# the ticks
# ---------------------------------------------------------------------------
def _lib_ticks(lib, lam):
    buf = (ctypes.c_double * 32)(*([-1.0] * 32))
    n = lib.svt_poisson_ticks(float(lam), buf)
    return n, np.array(buf[:max(n, 0)], dtype=np.float64), np.array(buf[:], dtype=np.float64)


@needs_longdouble
@pytest.mark.parametrize("lam,count", pc.TICK_COUNTS)
def test_ticks_of_the_library_are_the_restatement(lib, rules, lam, count):
    n, t, _ = _lib_ticks(lib, lam)
    wn, wt = pc.ticks(lam)
    assert n == wn == count
    assert np.array_equal(t.view(np.uint64), wt.view(np.uint64))
    assert rules([f"ticks {_hex(lam)}"]) == [" ".join([str(n)] + [f"{int(x):016x}" for x in t.view(np.uint64)])]
    if lam == 1e-16:
        assert t[-1] == 1.0
    if n > 0:
        assert (np.diff(t) > 0).all() and t[0] > 0.0 and t[-1] <= 1.0


def _reference_count(lam):
    """The return value of compute_cumsum_dpois as it is written, and nothing else of it"""
    dp = csdp = np.longdouble(math.exp(-float(lam)))  # (libm's exp, as in C: numpy's own may differ by an ulp)
    if csdp >= 1.0:
        return 0
    last = np.float64(csdp)
    for n in range(1, 32):
        dp = dp * np.longdouble(np.float64(lam) / np.float64(n))
        csdp = csdp + dp
        if np.float64(csdp) == last:
            return n
        last = np.float64(csdp)
    return -1


@needs_longdouble
def test_the_number_of_ticks_is_the_reference_s_and_the_ticks_ascend(lib):
    lams = np.concatenate([np.linspace(0.0, 4.6, 461), 10.0 ** np.arange(-18.0, 0.0, 0.5), [4.0, 4.5]])
    with np.errstate(all="ignore"):
        for lam in lams:
            n, t, _ = _lib_ticks(lib, lam)
            assert n == _reference_count(lam), lam
            if n > 0:
                assert (np.diff(t) >= 0).all() and 0.0 < t[0] and t[-1] <= 1.0, lam


@pytest.mark.parametrize("lam", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_a_lambda_that_is_no_rate_has_no_ticks(lib, lam):
    n, _, buf = _lib_ticks(lib, lam)
    assert n == -1 and (buf == -1.0).all()
    assert lib.svt_poisson_ticks(float(lam), None) == -1
    assert pc.ticks(lam)[0] == -1


def test_ticks_pointer_may_be_null(lib):
    assert lib.svt_poisson_ticks(1.0, None) == 18


@pytest.mark.parametrize("lam", [lam for lam, count in pc.TICK_COUNTS if count > 0] + [2.0, 3.3])
def test_every_tick_is_within_one_ulp_of_the_true_cdf(lib, lam):
    """|tick - CDF| in units of the tick's ulp, the CDF summed in mpmath at 200 bits; the lambdas are those of the table
    that have ticks, and 2 and 3.3, where the reference's own sum is 1.0 and 2.1 ulp off (1.6 at lambda = 4: its double
    exp() and double quotients lambda / n are each half an ulp off, and the sum is 55 times its first term).  The stored
    ticks come from the sum in long double throughout (svt_random_rules.h): 31 terms of 2^-64 each, then one rounding."""
    mpmath = pytest.importorskip("mpmath")
    n, t, _ = _lib_ticks(lib, lam)
    assert n > 0
    worst = 0.0
    with mpmath.workprec(200):
        L = mpmath.mpf(float(lam))
        term = cdf = mpmath.exp(-L)
        for k in range(n):
            if k > 0:
                term = term * L / k
                cdf = cdf + term
            worst = max(worst, abs(float((mpmath.mpf(float(t[k])) - cdf) / mpmath.mpf(float(np.spacing(t[k]))))))
    print(f"lambda = {lam!r}: {n} ticks, worst |tick - CDF| = {worst:.3f} ulp")
    assert worst <= 1.0, (lam, worst)


# ---------------------------------------------------------------------------
# the law, on the restatement (what fixes the seed the device test uses)
# ---------------------------------------------------------------------------
@needs_longdouble
def test_the_restatement_obeys_the_law_under_the_stated_seed():
    vals = pc.values(pc.LAW_SEED, np.arange(pc.LAW_N, dtype=np.uint64), pc.LAW_LAMBDA)
    assert pc.law_violations(vals) == []
    assert pc.law_violations(np.zeros(pc.LAW_N, dtype=np.int32)) != []       # (the check can fail)


# ---------------------------------------------------------------------------
# what the library refuses on the host: < 0, a message, nothing written (no device is touched)
# ---------------------------------------------------------------------------
REFUSED = [
    # lambda, nrow, first_leaf, nleaves, short workspace, message
    (1.0, 2 ** 31, 0, 1, False, b"2^31 - 1 rows"),
    (1.0, -1, 0, 1, False, b"negative extent"),
    (1.0, 5, 0, -1, False, b"negative extent"),
    (1.0, 5, -1, 3, False, b"negative extent"),
    (1.0, 2 ** 31 - 1, 2 ** 33, 2 ** 33, False, b"overflows 64 bits"),
    (1.0, 3, 2 ** 63 - 1, 1, False, b"overflows 64 bits"),
    (1.0, 37, 0, 333, True, b"workspace too small"),
    (4.5, 37, 0, 333, False, b"'lambda' too big?"),
    (-1.0, 37, 0, 333, False, b"'lambda' must be a non-negative number"),
    (float("nan"), 37, 0, 333, False, b"'lambda' must be a non-negative number"),
    (float("inf"), 37, 0, 333, False, b"'lambda' too big?"),
]


@pytest.mark.parametrize("lam,nrow,first,nleaves,short,msg", REFUSED)
def test_count_and_fill_refuse_on_the_host(lib, lam, nrow, first, nleaves, short, msg):
    nnz = ctypes.c_int64(-7)
    need = lib.svt_dev_poisson_ws_bytes(37 * 333)
    ws_bytes = need - 1 if short else 1 << 40
    # the pointers are never followed: the refusal comes first
    assert lib.svt_dev_poisson_count(lam, 5, nrow, first, nleaves, None, ctypes.byref(nnz), None, ws_bytes, None) < 0
    assert msg in lib.svt_last_error() and nnz.value == -7
    assert lib.svt_dev_poisson_fill(lam, 5, nrow, first, nleaves, None, None, None, None, ws_bytes, None) < 0
    assert msg in lib.svt_last_error()
    if not short:
        alloc, release = _never_called()
        assert lib.svt_dev_poisson(lam, 5, nrow, first, nleaves, alloc, release, None, ctypes.byref(nnz), None, None, None, None) < 0
        assert msg in lib.svt_last_error() and nnz.value == -7


def _never_called():
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN

    def alloc(nbytes, ctx):
        raise AssertionError("the allocator was called")

    def release(p, ctx):
        raise AssertionError("the allocator was called")
    return ALLOC_FN(alloc), FREE_FN(release)


def test_composition_needs_an_allocator(lib):
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN
    nnz = ctypes.c_int64(-7)
    assert lib.svt_dev_poisson(1.0, 5, 37, 0, 333, ALLOC_FN(), FREE_FN(), None, ctypes.byref(nnz), None, None, None, None) < 0
    assert b"an allocator is needed" in lib.svt_last_error() and nnz.value == -7


def test_rpois_refuses_on_the_host(lib):
    for args, msg in [((1.0, 0, 0, -1), b"'n' cannot be negative"), ((1.0, 0, -1, 5), b"'first' is negative"),
                      ((1.0, 0, 2 ** 63 - 1, 1), b"overflows"), ((4.5, 0, 0, 5), b"'lambda' too big?"),
                      ((-0.5, 0, 0, 5), b"non-negative"), ((1.0, 0, 0, 5), b"'out' is NULL")]:
        assert lib.svt_dev_rpois(*args, None, None) < 0
        assert msg in lib.svt_last_error(), args
    assert lib.svt_simple_rpois(-1, 1.0, 0, None) < 0 and b"'n' cannot be negative" in lib.svt_last_error()
    assert lib.svt_simple_rpois(5, 4.5, 0, None) < 0 and b"'lambda' too big?" in lib.svt_last_error()
    res, nnz = ctypes.c_void_p(0), ctypes.c_int64(-7)
    assert lib.svt_poissonSparseArray_begin(37, 333, 4.5, 0, ctypes.byref(res), ctypes.byref(nnz)) < 0
    assert b"'lambda' too big?" in lib.svt_last_error() and nnz.value == -7 and not res.value


def test_workspace_is_that_of_dense_to_sparse(lib):
    for n in (0, 1, 4095, 4096, 4097, 10 ** 10):
        assert lib.svt_dev_poisson_ws_bytes(n) == lib.svt_dev_from_dense_ws_bytes(n)


# ---------------------------------------------------------------------------
# the Session: every check before any call
# ---------------------------------------------------------------------------
class _NoCall:
    """A dispatcher that offers the entry points and must never be reached"""

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        raise AssertionError(f"{name} was called")


class _Recorder:
    def __init__(self):
        self.calls = []

    def has_entry(self, name):
        return True

    def __call__(self, name, *args):
        from sparsearray_amd import SVT_SparseArray
        self.calls.append((name, args))
        if name == "C_simple_rpois":
            return np.zeros(args[0], dtype=np.int32)
        dim = args[0]
        return SVT_SparseArray.from_csc(dim, "integer", np.zeros(int(np.prod(dim[1:])) + 1, dtype=np.int64),
                                        np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))


SESSION_REFUSALS = [
    (dict(dim=(3, 4), lambda_=1.0, density=0.1), "only one of 'lambda' and 'density' can be specified"),
    (dict(dim=(3, 4), lambda_=-0.5), "'lambda' must be a non-negative number"),
    (dict(dim=(3, 4), lambda_=float("nan")), "'lambda' must be a non-negative number"),
    (dict(dim=(3, 4), lambda_="1"), "'lambda' must be a non-negative number"),
    (dict(dim=(3, 4), lambda_=[1.0, 2.0]), "'lambda' must be a non-negative number"),
    (dict(dim=(3, 4), lambda_=True), "'lambda' must be a non-negative number"),
    (dict(dim=(3, 4), density=1.0), "'density' must be a number >= 0 and < 1"),
    (dict(dim=(3, 4), density=-0.1), "'density' must be a number >= 0 and < 1"),
    (dict(dim=(3, 4), density="x"), "'density' must be a number >= 0 and < 1"),
    (dict(dim="ab"), "'dim' must be an integer vector"),
    (dict(dim=(3, 4.5)), "'dim' must be an integer vector"),
    (dict(dim=(True, False)), "'dim' must be an integer vector"),
    (dict(dim=((3, 4), (5, 6))), "'dim' must be an integer vector"),
    (dict(dim=()), "'dim' must have at least one element"),
    (dict(dim=(3, -1)), "'dim' must contain non-negative integers"),
    (dict(dim=(3, float("nan"))), "'dim' must contain non-negative integers"),
    (dict(dim=(2 ** 31, 2)), "'dim' must contain non-negative integers"),
    (dict(dim=(3, 4), seed=-1), "'seed' must be an integer >= 0 and < 2\\^64"),
    (dict(dim=(3, 4), seed=2 ** 64), "'seed' must be an integer >= 0 and < 2\\^64"),
    (dict(dim=(3, 4), seed=1.5), "'seed' must be an integer >= 0 and < 2\\^64"),
    (dict(dim=(3, 4), dimnames=[["a", "b"], None]), "'dimnames' must be NULL or a list"),
    (dict(dim=(3, 4), dimnames=[None]), "'dimnames' must be NULL or a list"),
]


@pytest.mark.parametrize("kw,msg", SESSION_REFUSALS, ids=[str(k) for k in range(len(SESSION_REFUSALS))])
def test_session_checks_come_before_any_call(kw, msg):
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd.api import Session
    with pytest.raises(SparseArrayError, match=msg):
        Session(_NoCall()).poissonSparseArray(**kw)


def test_session_matrix_and_rpois_checks_come_before_any_call():
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd.api import Session
    s = Session(_NoCall())
    for kw in (dict(nrow=(1, 2)), dict(ncol="3"), dict(nrow=float("nan")), dict(nrow=None)):
        with pytest.raises(SparseArrayError, match="'nrow' and 'ncol' must be single integers"):
            s.poissonSparseMatrix(**kw)
    with pytest.raises(SparseArrayError, match="only one of 'lambda' and 'density' can be specified"):
        s.poissonSparseMatrix(3, 4, lambda_=1.0, density=0.5)
    with pytest.raises(SparseArrayError, match="'n' cannot be negative"):
        s.simple_rpois(-1, 1.0)
    with pytest.raises(SparseArrayError, match="'n' must be a single integer"):
        s.simple_rpois(1.5, 1.0)
    with pytest.raises(SparseArrayError, match="'lambda' must be a single numeric value"):
        s.simple_rpois(3, "1")
    with pytest.raises(SparseArrayError, match="'lambda' cannot be negative"):
        s.simple_rpois(3, -1.0)
    with pytest.raises(SparseArrayError, match="'seed' must be an integer"):
        s.simple_rpois(3, 1.0, seed=-3)


def test_session_without_the_entry_points_says_so():
    from sparsearray_amd.api import Session, SparseArrayUnsupported

    class Bare:
        def __call__(self, name, *args):
            raise AssertionError(name)
    with pytest.raises(SparseArrayUnsupported, match="C_poissonSparseArray is not offered"):
        Session(Bare()).poissonSparseArray((3, 4))
    with pytest.raises(SparseArrayUnsupported, match="C_simple_rpois is not offered"):
        Session(Bare()).simple_rpois(3, 1.0)


def test_session_hands_over_dim_lambda_and_seed():
    from sparsearray_amd.api import Session
    rec = _Recorder()
    s = Session(rec)
    x = s.poissonSparseArray([3, 4, 2], dimnames=[list("abc"), None, ["u", "v"]], seed=2 ** 64 - 1)
    assert x.type == "integer" and tuple(x.dim) == (3, 4, 2) and x.dimnames == [list("abc"), None, ["u", "v"]]
    s.poissonSparseArray(np.array([3.0, 4.0]), density=0.5)
    s.poissonSparseArray(7, lambda_=0)
    s.poissonSparseMatrix(5, 6, density=0.0, seed=9)
    s.poissonSparseMatrix()
    s.simple_rpois(4, 2, seed=3)
    assert rec.calls == [
        ("C_poissonSparseArray", ((3, 4, 2), -np.log(0.95), 2 ** 64 - 1)),
        ("C_poissonSparseArray", ((3, 4), -np.log(1 - 0.5), 0)),
        ("C_poissonSparseArray", ((7,), 0.0, 0)),
        ("C_poissonSparseArray", ((5, 6), 0.0, 9)),
        ("C_poissonSparseArray", ((1, 1), -np.log(0.95), 0)),
        ("C_simple_rpois", (4, 2.0, 3)),
    ]
