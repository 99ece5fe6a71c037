"""The case table of tests/transpose_cases.py without a GPU: the reference against numpy, the tracer's exactness, every
case's arithmetic through device.transpose_plan() (svt_dev_transpose_plan needs no device), and negative checks of the
comparison -- what tests/test_hip_transpose_cases.py relies on when it runs the same table on the GPU."""
from math import prod

import numpy as np
import pytest

import transpose_cases as tc
from sparsearray_amd.device import transpose_plan

NAMES = [c["name"] for c in tc.CASES]
T_NAMES = [c["name"] for c in tc.CASES if c["perm"] is None]
A_NAMES = [c["name"] for c in tc.CASES if c["perm"] is not None]
SMALL_NAMES = [c["name"] for c in tc.CASES if prod(c["dim"]) < tc.SMALL]


def test_the_table_covers_every_route_and_every_arena_route():
    routes = set()
    for c in tc.CASES:
        routes |= set(c["route"])
    assert routes == {"t_bucketed", "t_key_sort", tc.LP, tc.SW, tc.SLAB, tc.VIA, tc.GEN, tc.K32, tc.REFUSED}      # all but key_sort_64
    assert {c["arena"] for c in tc.CASES if c["arena"]} >= {
        "bucketed staged", "pass 3 in rounds", "6000 groups", "key sort", "swap01", "slab", "slab refused inside general",
        "via 3-d", "general", "leaf-preserving", "key_sort_32"}
    assert len(SMALL_NAMES) >= 25


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_reference_is_numpy_transpose_of_the_dense_array(name):
    tc.check_reference_against_numpy(name)


@pytest.mark.parametrize("name", NAMES)
def test_tracer_is_exact(name):
    """every value names its old position: doubles hold old linear index + 1 exactly, integers stay off 0 and NA"""
    lin = tc.pattern(name)
    d = tc.values("tracer", "double", lin)
    assert d.dtype == np.float64 and np.array_equal(d.astype(np.int64) - 1, lin) and (lin.size == 0 or d.max() < 2.0 ** 53)
    i = tc.values("tracer", "integer", lin)
    assert i.dtype == np.int32 and np.array_equal(i.astype(np.int64), lin % (2 ** 31 - 2) + 1)
    assert lin.size == 0 or (i.min() >= 1 and i.max() <= 2 ** 31 - 2)
    if lin.size and lin[-1] < 2 ** 31 - 2:
        assert np.unique(i).size == i.size
    assert np.array_equal(tc.values("tracer", "logical", lin), i)


@pytest.mark.parametrize("name", T_NAMES)
def test_t_case_is_on_the_branch_it_claims(name):
    c, lin = tc.BY_NAME[name], tc.pattern(name)
    plan = transpose_plan(c["dim"][0], c["dim"][1], lin.size)
    for k, v in c["plan"].items():
        assert plan[k] == v, (k, plan)
    assert c["route"] == ({} if lin.size == 0 else {"t_bucketed": 1} if plan["bucketed"] else {"t_key_sort": 1})
    if plan["bucketed"]:
        wg, fb, _ = tc.loads(c["dim"], lin, plan)
        assert wg.sum() == lin.size == fb.sum() and plan["ngroups"] <= 6000
        assert plan["nfb"] == -(-c["dim"][0] >> plan["fbits"]) and plan["ngroups"] == -(-c["dim"][1] // tc.T2_NT)
    if c["check"] is not None:
        assert plan["bucketed"]
        c["check"](c["dim"], lin, plan)


@pytest.mark.parametrize("name", A_NAMES)
def test_aperm_case_is_on_the_branch_it_claims(name):
    c, lin = tc.BY_NAME[name], tc.pattern(name)
    assert sorted(c["perm"]) == list(range(1, len(c["dim"]) + 1))
    if c["swap"] is not None:
        (d0, d1, nslab), want = c["swap"]
        assert transpose_plan(d0, d1, lin.size, nslab)["bucketed"] == want
    if c["check"] is not None:
        c["check"](c["dim"], c["perm"], lin)
    if tc.SW in c["route"] or tc.VIA in c["route"]:
        assert c["swap"] is not None and c["swap"][1]
    if tc.REFUSED in c["route"]:
        assert c["check"] is not None


def test_plan_query_answers_without_a_device():
    p = transpose_plan(3000, 700, 21_000)
    assert p["bucketed"] and p["why_not"] == "taken" and (p["nfb"], p["ngroups"]) == (-(-3000 >> p["fbits"]), 3)
    assert p["ncoarse"] == -(-p["nfb"] >> p["cbits"]) and p["key_sort_passes"] == 2
    q = transpose_plan(3000, 700, 0)
    assert not q["bucketed"] and q["why_not"] == "shape"
    assert not transpose_plan(32, 1_536_001, 3_072_002)["bucketed"] and transpose_plan(32, 1_536_000, 3_072_000)["ngroups"] == 6000
    assert transpose_plan(16_384, 1, 4096)["why_not"] == "reserve"
    assert [transpose_plan(n, 10, 5)["key_sort_passes"] for n in (2, 256, 257, 65_536, 65_537, 2 ** 24, 2 ** 24 + 1)] == [1, 1, 2, 2, 3, 3, 4]
    from sparsearray_amd._hip import HipBackendError
    with pytest.raises(HipBackendError, match="svt_dev_transpose_plan"):
        transpose_plan(10, 10, 5, nslab=0)


def test_specials_land_in_first_and_last_slots():
    """each special value is the first and the last entry of some column's run (a pass-2 piece) and of some output
    leaf (a pass-3 bucket's row) of the plain staged case"""
    name = "t_plain_staged"
    lin = tc.pattern(name)
    cp, _ = tc.csc_of(tc.BY_NAME[name]["dim"], lin)
    ocp, _, order = tc.reference(name)
    for dtype, table in (("double", tc.SPECIALS_F64), ("integer", tc.SPECIALS_I32), ("logical", tc.SPECIALS_LGL)):
        v = tc.bits(tc.values("specials", dtype, lin))
        every = set(tc.bits(table).tolist())
        ne, one = np.flatnonzero(np.diff(cp) > 0), np.flatnonzero(np.diff(ocp) > 0)
        assert set(v[cp[ne]].tolist()) == every and set(v[cp[ne + 1] - 1].tolist()) == every
        w = v[order]
        assert set(w[ocp[one]].tolist()) == every and set(w[ocp[one + 1] - 1].tolist()) == every


def _damaged(want, how):
    """a copy of `want` with one defect; None if this palette cannot show it"""
    cp, ri, v, lg = want
    ri, v = ri.copy(), v.copy()
    b = tc.bits(v)
    lens = np.diff(cp)
    if how == "swap":               # two neighbours of one output leaf (equal old rows) change places
        for leaf in np.flatnonzero(lens >= 2):
            for i in range(cp[leaf], cp[leaf + 1] - 1):
                if b[i] != b[i + 1]:
                    ri[[i, i + 1]] = ri[[i + 1, i]]
                    v[[i, i + 1]] = v[[i + 1, i]]
                    return cp, ri, v, lg
        return None
    if how == "swap_values":        # only their values do
        for leaf in np.flatnonzero(lens >= 2):
            for i in range(cp[leaf], cp[leaf + 1] - 1):
                if b[i] != b[i + 1]:
                    v[[i, i + 1]] = v[[i + 1, i]]
                    return cp, ri, v, lg
        return None
    if how == "zero":               # an idle slot's fill instead of a value
        i = np.flatnonzero(b != 0)
        if i.size == 0:
            return None
        v[i[len(i) // 2]] = 0
        return cp, ri, v, lg
    if how == "payload":            # a NaN comes back as another NaN
        if v.dtype != np.float64 or not np.isnan(v).any():
            return None
        i = np.flatnonzero(np.isnan(v))[3]
        v.view(np.uint64)[i] ^= np.uint64(0x10)
        assert np.isnan(v[i])
        return cp, ri, v, lg
    if how == "minus_zero":
        if v.dtype != np.float64:
            return None
        i = np.flatnonzero(b == np.int64(-2 ** 63))
        if i.size == 0:
            return None
        v[i[0]] = 0.0
        return cp, ri, v, lg
    if how == "pointer":
        cp = cp.copy()
        leaf = int(np.flatnonzero(lens >= 1)[0])
        cp[leaf + 1] -= 1
        return cp, ri, v, lg
    if how == "flag":
        return cp, ri, v, not lg
    if how == "dtype":
        with np.errstate(invalid="ignore"):
            return cp, ri, v.astype(np.float64 if v.dtype == np.int32 else np.int32), lg
    raise AssertionError(how)


@pytest.mark.parametrize("how", ["swap", "swap_values", "zero", "payload", "minus_zero", "pointer", "flag", "dtype"])
@pytest.mark.parametrize("palette", tc.PALETTES)
@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("name", ["t_plain_staged", "a_leaf_1423"])
def test_comparison_rejects_a_damaged_result(name, dtype, palette, how):
    want, _ = tc.expected(name, dtype, palette)
    tc.compare(want, want, what="itself")
    bad = _damaged(want, how)
    if bad is None:
        # not every palette holds the value the defect needs; the ones that must are checked here
        assert (how, dtype) not in {("swap", "double"), ("swap_values", "double"), ("zero", "double")}
        assert not (how in ("payload", "minus_zero") and dtype == "double" and palette == "specials")
        assert not (how in ("swap", "swap_values", "zero") and palette == "tracer")
        return
    with pytest.raises(AssertionError):
        tc.compare(bad, want, what=how)
    # what a float comparison would have let through
    if how in ("payload", "minus_zero"):
        assert np.array_equal(bad[2], want[2], equal_nan=True)
