"""Which ``.Call`` entry points ``Session`` issues over the HIP library, and that it hands back what they return.

The Python routing is what is checked here, not a kernel: the order statistics, x[i, j] and the one-call row statistics
each issue exactly one ``.Call`` (a recording dispatcher around hip_dispatcher(), tests/session_calls_cases.py), and each
result equals the oracle session's bit for bit.  The operands are 5 x 4 -- the smallest with an empty leaf, a stored zero
and an NA in different columns -- and hold small integers whose row means are integers, so no sum, mean, centred sum or
interpolated quantile of them rounds: the comparison needs no tolerance.  "Bit for bit" is R's identical(): the same bits
wherever the oracle's value is a number, and a missing value of the same class (NA or NaN) wherever it is not -- the sign
and the payload of a NaN that arithmetic made are whatever the processor's arithmetic leaves there (the variance of the row with the NA comes back with the sign bit
set from the device and clear from the host), not a value."""
import numpy as np
import pytest

import session_calls_cases as sc
from sparsearray_amd import SVT_SparseArray, is_NA_real

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROW_CALLS = [(m, (), {"dims": 1, "na_rm": na_rm}) for m in ("rowMeans", "rowVars", "rowRanges") for na_rm in (False, True)]


def _same_bits(got, want, what):
    if isinstance(want, SVT_SparseArray):
        assert isinstance(got, SVT_SparseArray), what
        assert (got.dim, got.type, got.na_background, got.dimnames) == (want.dim, want.type, want.na_background,
                                                                        want.dimnames), what
        for g, w in zip(got.to_csc(), want.to_csc()):
            _same_bits(g, w, what)
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if want.dtype == np.float64:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(is_NA_real(got), is_NA_real(want)), (what, got, want)
        got, want = got[~nan], want[~nan]
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), (what, got, want)


@pytest.mark.parametrize("key", ["X", "XI"])
def test_one_call_each_and_the_oracles_bits(hip, oracle, key):
    ops = sc.operands()
    for n, (m, args, kw) in enumerate(sc.ORDER_CALLS + ROW_CALLS):
        what = f"{m} {key} #{n}"
        got, calls = sc.run(hip, ops, m, key, args, kw)
        assert not isinstance(got, Exception), (what, got)
        assert calls == [sc.FULL if m in ("rowMeans", "rowVars", "rowRanges") else sc.entry_of(m)], (what, calls)
        _same_bits(got, getattr(oracle, m)(ops[key], *args, **kw), what)
