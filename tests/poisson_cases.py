"""The rules of the random count arrays (sparsearray_amd/csrc/svt_random_rules.h) restated in numpy, and the cases the
Poisson tests share.  Nothing here calls the library: Philox4x32-10 vectorised in uint64, the cell -> uniform -> value
rule, and the ticks of compute_cumsum_dpois (src/randomSparseArray.c:19-38 of the reference) in numpy.longdouble."""
import functools
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# counter words, key words -> output words (Salmon et al. 2011; the Random123 known-answer vectors)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# lambda -> number of ticks (-1: 32 are not enough)
TICK_COUNTS = [(0.0, 0), (1e-300, 0), (1e-17, 0), (1e-16, 2), (-np.log(0.95), 9), (1.0, 18), (4.0, 31), (4.5, -1), (5.0, -1),
               (100.0, -1)]
LAMBDAS = [0.0, 1e-17, 1e-16, -np.log(0.95), 1.0, 4.0]
SEEDS = [0, 1, 2 ** 32, 2 ** 64 - 1]
DEFAULT_LAMBDA = -np.log(0.95)

HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant == 63


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of counters c0..c3 (arrays or ints) under the key."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no wrap in uint64
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c1, c3 = p1 & MASK32, p0 & MASK32
        c0, c2 = n0, n2
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def cell_uniform(seed, cells):
    """u of every cell (uint64 array of flat cell indices) under ``seed`` (an int in [0, 2^64))."""
    cells = np.asarray(cells, dtype=np.uint64)
    block = cells >> np.uint64(1)
    w = philox4x32_10(block & MASK32, block >> S32, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    odd = (cells & np.uint64(1)).astype(bool)
    lo, hi = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    x = (hi << S32) | lo
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _ticks(lam):
    lam = np.float64(lam)
    if not lam >= 0 or np.isinf(lam):
        return -1, ()
    # two sums side by side (svt_random_rules.h): `ref`, the reference's own arithmetic (the double exp(), the double
    # quotient lambda / n), says by the reference's tests where the table ends; the tick stored is `acc`, the same sum
    # with both in long double
    LD = np.longdouble
    with np.errstate(all="ignore"):
        ref_dp = ref = LD(math.exp(-float(lam)))     # (libm's exp, as in C: numpy's own may differ by an ulp)
        if ref >= 1.0:
            return 0, ()
        acc_dp = acc = np.exp(-LD(lam))
        ref_last = np.float64(ref)
        t = [np.float64(acc)]
        for n in range(1, 32):
            ref_dp = ref_dp * LD(lam / np.float64(n))
            ref = ref + ref_dp
            if np.float64(ref) == ref_last:
                return n, tuple(t)
            ref_last = np.float64(ref)
            acc_dp = acc_dp * (LD(lam) / LD(n))
            acc = acc + acc_dp
            t.append(np.float64(acc))
    return -1, ()


def ticks(lam):
    """(n, float64 array of n ticks); n == -1: 32 ticks are not enough, or lambda is negative, NaN or infinite."""
    n, t = _ticks(float(lam))
    return n, np.array(t, dtype=np.float64)


def values(seed, cells, lam):
    """The int32 value of every cell: the first k with u < ticks[k], i.e. the number of ticks <= u (they ascend)."""
    n, t = ticks(lam)
    assert n >= 0
    u = cell_uniform(seed, cells)
    return np.searchsorted(t, u, side="right").astype(np.int32)


def dense(seed, lam, nrow, nleaves, first_leaf=0):
    """The leaves [first_leaf, first_leaf + nleaves) as an (nrow, nleaves) int32 array."""
    cells = np.uint64(first_leaf) * np.uint64(nrow) + np.arange(nrow * nleaves, dtype=np.uint64)
    return values(seed, cells, lam).reshape((nrow, nleaves), order="F")


def csc_of(d):
    """(col_ptr int64, row_idx int32, val int32) of a dense (nrow, nleaves) array: the nonzeros in column-major order."""
    nrow, nleaves = d.shape
    flat = d.reshape(-1, order="F")
    pos = np.flatnonzero(flat)
    counts = np.bincount(pos // nrow, minlength=nleaves) if nrow else np.zeros(nleaves, dtype=np.int64)
    col_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row_idx = (pos % nrow if nrow else pos).astype(np.int32)
    return col_ptr, row_idx, flat[pos].astype(np.int32)


@functools.lru_cache(maxsize=None)
def whole(seed, lam, nrow, total):
    """dense() of an array of ``total`` leaves, computed once and read-only: the windows of one array share it."""
    d = dense(seed, lam, nrow, total)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(seed, lam, nrow, nleaves, first_leaf=0, total=None):
    """csc_of() of the leaves [first_leaf, first_leaf + nleaves), computed once per case; the arrays are read-only.
    ``total``: cut them out of whole(seed, lam, nrow, total) (the cell index is global: it is the same thing)."""
    d = dense(seed, lam, nrow, nleaves, first_leaf) if total is None else whole(seed, lam, nrow, total)[:, first_leaf:first_leaf + nleaves]
    out = csc_of(d)
    for a in out:
        a.setflags(write=False)
    return out


def extents(T):
    """The shapes of the extent cases for a tile of T cells, with the lambda of each."""
    return [((0, 5), DEFAULT_LAMBDA), ((7, 0), DEFAULT_LAMBDA), ((1, 1), DEFAULT_LAMBDA), ((T - 1, 1), DEFAULT_LAMBDA),
            ((T, 1), DEFAULT_LAMBDA), ((T + 1, 1), DEFAULT_LAMBDA), ((37, 333), DEFAULT_LAMBDA), ((1, 3 * T + 5), DEFAULT_LAMBDA),
            ((2 * T + 200, 3), DEFAULT_LAMBDA), ((3000001, 3), -np.log(0.99))]


# The law (independent of the ticks): 2^22 cells at lambda = 1 under LAW_SEED; for every k with n p_k >= 25 the count of
# cells equal to k lies within 6 sqrt(n p_k (1 - p_k)) of n p_k.  The restatement passes this under seed 20240607
# (tests/test_zzzzzzzzzzzz_poisson_cpu.py checks that on the CPU).
LAW_SEED, LAW_N, LAW_LAMBDA = 20240607, 2 ** 22, 1.0


def law_violations(vals, lam=LAW_LAMBDA):
    """[(k, count, mean, bound)] of the classes that break the law; [] when it holds.  p_k from math.lgamma, not from
    the ticks."""
    n = int(vals.size)
    counts = np.bincount(vals.astype(np.int64))
    bad = []
    for k in range(0, 64):
        p = math.exp(-lam + k * math.log(lam) - math.lgamma(k + 1)) if lam > 0 else float(k == 0)
        if n * p < 25:
            continue
        c = int(counts[k]) if k < counts.size else 0
        bound = 6.0 * math.sqrt(n * p * (1.0 - p))
        if abs(c - n * p) > bound:
            bad.append((k, c, n * p, bound))
    return bad
