"""The chains of tests/chain_cases.py walked with the dense rules alone, no GPU: every step's rule applied to the rule's
own result of the step before, every consumer's expectation computed and met by a plain numpy answer, and what the
chains claim about their intermediates (an empty one is empty, the stored zeros are still there after the subset, the
integer product overflows, each subset takes the route it names) asserted.  tests/test_hip_chains.py runs the same data
on the device."""
import numpy as np
import pytest

import chain_cases as cc
import subset_cases as sc


@pytest.fixture(scope="module")
def walked():
    """name -> (mats, wants) of the chain, each walked once"""
    done = {}

    def walk(name):
        if name not in done:
            chain = cc.CHAINS[name]
            mats = {n: cc.operand(n) for n in chain.inputs}
            wants = {}
            for step in chain.steps:
                wants[step[0]] = w = cc.rule(step, mats)
                mats[step[0]] = m = w.mat()
                w.check(m, f"{name}: {step[0]}", max_ulps=0)              # the rule's own result passes its own check
            done[name] = (mats, wants)
        return done[name]
    return walk


def test_inputs_are_what_the_chains_need():
    T_subset, T_arith = 4096, 2048                          # (svt_dev_subset_tile / svt_dev_arith_tile: test_abi.py)
    x, m, xs, i, lg = (cc.operand(n) for n in ("x", "m", "xs", "i", "lg"))
    for a in (x, m, xs, i, lg):
        cc.check_invariants(a, *cc.DIM, a.type, "input")
        lens = np.diff(a.col_ptr)
        assert a.nnz > 2 * T_subset and a.nnz > 4 * T_arith and lens.max() == cc.DIM[0] and (lens == 0).sum() >= 17
    assert np.array_equal(np.flatnonzero(np.diff(x.col_ptr) == 0), np.setdiff1d(np.arange(3, 160, 7), [80]))
    assert not np.array_equal(x.dense[1], m.dense[1]) and (x.dense[1] & m.dense[1]).sum() > 500
    special = np.isin(sc.bits(xs.val), sc.bits(sc.SPECIALS_F64))
    assert 0.05 < special.mean() < 0.15 and set(sc.bits(sc.SPECIALS_F64).tolist()) <= set(sc.bits(xs.val).tolist())
    assert (i.val == cc.NA_integer).any() and (i.val == cc.INT_MAX).any() and (i.val == cc.INT_MAX - 1).any()
    assert set(np.unique(lg.val).tolist()) == {int(cc.NA_integer), 0, 1}
    assert cc.operand("a3").ncol == 20 and cc.operand("b3").ncol == 20 and cc.operand("a3").nrow == 9


def test_tile_sizes_assumed_above():
    from sparsearray_amd.device import arith_tile, subset_tile
    assert (subset_tile(), arith_tile()) == (4096, 2048)


@pytest.mark.parametrize("name", cc.NAMES)
def test_chain_walks_and_claims_hold(walked, name):
    chain = cc.CHAINS[name]
    mats, wants = walked(name)
    assert {s[0] for s in chain.steps}.isdisjoint(chain.inputs) and len({s[0] for s in chain.steps}) == len(chain.steps)
    for claim in chain.claims:
        cc.check_claim(claim, mats, wants)
    for target, _ in chain.consumers:
        assert target in wants, f"{name}: {target} is no device-made operand"
    for operand, word in chain.refused:
        assert mats[operand].type == word == "logical"


@pytest.mark.parametrize("name", cc.NAMES)
def test_every_consumer_expectation_is_computable(walked, name):
    mats, _ = walked(name)
    for target, cons in cc.CHAINS[name].consumers:
        m = mats[target]
        if cons == ("crossprod",):
            assert m.type == "double" and np.isfinite(m.val).all(), f"{name}: crossprod of {target} has no exact product"
        cc.check_consumer(cons, m, cc.host_consumer(cons, m), f"{name}: {target}")


def test_subset_steps_take_the_routes_they_name(walked):
    mats, _ = walked("subset_then_everything")
    steps = {s[0]: s for s in cc.CHAINS["subset_then_everything"].steps}
    assert cc.subset_route(steps["w"], mats) == {"column_gather": 1, "row_filter": 1, "general_rows": 0}
    assert cc.subset_route(steps["w2"], mats) == {"column_gather": 1, "row_filter": 0, "general_rows": 1}
    assert cc.subset_route(steps["wts"], mats) == {"column_gather": 2, "row_filter": 0, "general_rows": 1}
    w = steps["w"]
    assert np.all(np.diff(w[3]) > 0) and np.unique(w[4]).size < w[4].size          # rows increase, columns repeat
    assert 3 in w[4] and np.diff(mats["x"].col_ptr)[3] == 0                        # an empty column, repeated
    assert np.unique(steps["w2"][3]).size == cc.DIM[0] < steps["w2"][3].size       # a permutation, with repeats
    assert mats["w"].nnz > 4096 and mats["w2"].nnz > 2 * 4096


def test_a_wrong_link_is_caught(walked):
    """the checks reject what they must: one value off by one ulp, one entry dropped, one stored zero added"""
    mats, wants = walked("normalise_log_centre_consume")
    z = mats["z"]
    v = z.val.copy()
    v[1234] = np.nextafter(v[1234], np.inf)
    with pytest.raises(AssertionError, match="differ as bits"):
        wants["z"].check(cc.Mat(z.nrow, "double", z.col_ptr, z.row_idx, v), "off by an ulp")
    cp = z.col_ptr.copy()
    cp[-1] -= 1
    with pytest.raises(AssertionError):
        wants["z"].check(cc.Mat(z.nrow, "double", cp, z.row_idx[:-1], z.val[:-1]), "an entry dropped")
    with pytest.raises(AssertionError, match="ulps"):
        l = mats["l"]
        v = l.val.copy()
        v[77] = np.nextafter(v[77], np.inf)
        wants["l"].check(cc.Mat(l.nrow, "double", l.col_ptr, l.row_idx, v), "log1p an ulp off", max_ulps=0)
    m = mats["z"]
    med = cc.host_consumer(("colmedians", False), m)
    med[80] = np.nextafter(med[80], np.inf)
    with pytest.raises(AssertionError):
        cc.check_consumer(("colmedians", False), m, med, "median an ulp off")
    s = cc.host_consumer(("colstats", "sum"), m)
    s[80] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="err / bound"):
        cc.check_consumer(("colstats", "sum"), m, s, "sum off by 1e-9")
