"""Operands made on the device as inputs (tests/chain_cases.py): the results of subset, Arith / Math, t() and aperm() go
straight into every consumer -- statistics, medians, quantiles, MADs, ranks, the product, transposition, subset and Arith
again -- on the same stream, with no synchronisation and no download between a producer's return and the launch of what
consumes its result.  Everything is downloaded after the last launch, and every link is then checked on its own against
the dense rule applied to the ACTUAL arrays of the link before: at tolerance 0 (bits), except log1p / expm1 / ^ (the
measured MAX_ULPS of tests/test_hip_arith.py) and the sums and products (the bounds of exact_stats / exact_products).

A consumer that misses its rule is run once more on a copy of the same arrays made by DeviceCSC.from_host; the message
says whether the copy passes -- wrong on this data, or wrong only on a device-made operand."""
import numpy as np
import pytest

import chain_cases as cc
from test_hip_arith import MAX_ULPS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _upload(m: cc.Mat):
    from sparsearray_amd.device import DeviceCSC
    return DeviceCSC(m.nrow, torch.as_tensor(m.col_ptr.copy(), device="cuda"), torch.as_tensor(m.row_idx.copy(), device="cuda"),
                     torch.as_tensor(m.val.copy(), device="cuda"), logical=m.type == "logical")


def _download(A) -> cc.Mat:
    from sparsearray_amd.svt import INTSXP, LGLSXP, REALSXP
    assert (A.val.dtype == torch.float64) == (A.Rtype == REALSXP)
    type = {REALSXP: "double", INTSXP: "integer", LGLSXP: "logical"}[A.Rtype]
    assert A.col_ptr.numel() == A.ncol + 1 and A.row_idx.numel() == A.nnz == A.val.numel()
    return cc.Mat(A.nrow, type, A.col_ptr.cpu().numpy(), A.row_idx.cpu().numpy(), A.val.cpu().numpy())


def _launch_step(step, dev):
    """the producer of ``step`` on the device operands ``dev``; returns the new DeviceCSC.  (A producer reads its own
    count back to size its result: that is inside the producer.)"""
    _, kind, src, *args = step
    A = dev[src]
    if kind == "scalar":
        op, s, st = args
        return A.arith(op, int(s) if st == "integer" else float(s))
    if kind == "merge":
        return A.arith(args[0], dev[args[1]])
    if kind == "neg":
        return A.neg()
    if kind == "math":
        return A.math(args[0])
    if kind == "subset":
        return A.subset(rows=args[0], cols=args[1])
    if kind == "t":
        return A.t()
    if kind == "aperm":
        return A.aperm(args[0], args[1])[0]
    raise KeyError(kind)


def _launch_consumer(cons, A, Y):
    """the consumer on the device operand; returns device tensors, nothing is read back"""
    from sparsearray_amd import device
    kind = cons[0]
    if kind == "colstats":
        return device.colstats(A, cons[1], inner=cons[2] if len(cons) > 2 else 1)[0]
    if kind == "rowsums":
        return device.rowsums(A)
    if kind == "colmedians":
        return device.colmedians(A, na_rm=cons[1])
    if kind == "colquantiles":
        return device.colquantiles(A, cc.PROBS, na_rm=cons[1])
    if kind == "colmads":
        return device.colmads(A, na_rm=cons[1])
    if kind == "colranks":
        # no column of a chain operand is long enough for the form that sorts in the workspace: sized without a look
        # at the column lengths (which would be a read-back); the flag says so if that were wrong
        assert A.nrow <= device.colranks_form_limits()[1]
        ws = torch.empty(device._lib().svt_dev_colranks_ws_bytes(A.ncol, 0), dtype=torch.uint8, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        return device.colranks(A, cons[1], ws=ws, flag=flag) + (flag,)
    if kind == "crossprod":
        return device.crossprod_csc_dense(A, Y[A.nrow])
    raise KeyError(kind)


def _host(out):
    if isinstance(out, tuple):
        rank_nz, zero_rank, flag = (t.cpu().numpy() for t in out)
        assert int(flag[0]) == 0, "colranks: the workspace was made for fewer long nonzeros than the operand holds"
        return rank_nz, zero_rank
    return out.cpu().numpy()


def _check_consumer_or_say_which(cons, A, m, got, Y, what):
    try:
        cc.check_consumer(cons, m, got, what)
    except AssertionError as e:
        copy = _upload(m)                                  # the same arrays, made by hand: DeviceCSC.from_host's layout
        again = _launch_consumer(cons, copy, Y)
        torch.cuda.synchronize()
        try:
            cc.check_consumer(cons, m, _host(again), what + " (hand-built copy)")
            verdict = "a hand-built copy of the same arrays PASSES: wrong only on the device-made operand"
        except AssertionError as e2:
            verdict = f"a hand-built copy of the same arrays fails too ({e2}): wrong on this data"
        raise AssertionError(f"{e}\n{verdict}") from e


@pytest.mark.parametrize("name", cc.NAMES)
def test_chain(hip, name):
    """One chain, every link judged: the message of a failure lists the links that miss their rule, and only those.

    The log1p link of normalise_log_centre_consume is held to MAX_ULPS["log1p"] = 0.  The device library's log1p missed
    it (8698 of this chain's 8747 values at 0 ulps, 49 at 1 ulp); svt_rule_log1p (svt_arith_rules.h) meets it."""
    from sparsearray_amd import SparseArrayError
    from sparsearray_amd.device import subset_route_counts
    chain = cc.CHAINS[name]
    mats = {n: cc.operand(n) for n in chain.inputs}
    dev = {n: _upload(m) for n, m in mats.items()}
    Y = {}                                                 # nrow -> the dense operand of the products, on the device
    torch.cuda.synchronize()

    # ---- launch everything: producers in order, then every consumer; no synchronize, no download ----
    routes = {}
    for step in chain.steps:
        if step[1] == "subset":
            subset_route_counts(reset=True)                # (host counters of the library)
        dev[step[0]] = _launch_step(step, dev)
        if step[1] == "subset":
            routes[step[0]] = subset_route_counts()
    for target, cons in chain.consumers:
        n = dev[target].nrow
        if cons == ("crossprod",) and n not in Y:
            Y[n] = torch.as_tensor(np.ascontiguousarray(cc.crossprod_Y(n).T), device="cuda")     # (an upload)
    outs = [(target, cons, _launch_consumer(cons, dev[target], Y)) for target, cons in chain.consumers]
    ovflow = {s[0]: dev[s[0]].ovflow for s in chain.steps if hasattr(dev[s[0]], "ovflow")}

    # ---- the last launch is behind us: download ----
    torch.cuda.synchronize()
    for step in chain.steps:
        mats[step[0]] = _download(dev[step[0]])
    got = [(target, cons, _host(out)) for target, cons, out in outs]
    ovflow = {k: bool(v.item()) for k, v in ovflow.items()}
    for step in chain.steps:                               # arrays that are no operand end the test here
        cc.check_structure(mats[step[0]], f"{name}: {step[0]} = {step[1]}({step[2]})")

    # ---- every link against the rule on the actual arrays of the link before; a link that misses its rule does not
    # hide the verdict on the others (each expectation is made from actual arrays) ----
    wants, missed = {}, []

    def link(f, *args):
        try:
            return f(*args)
        except AssertionError as e:
            missed.append(str(e))

    def producer(step, w):
        what = f"{name}: {step[0]} = {step[1]}({step[2]})"
        if w.ulps_of:
            print(f"{what}: {w.ulps_of}: {cc.ulps_histogram(mats[step[0]], w)}")
        w.check(mats[step[0]], what, max_ulps=MAX_ULPS.get(w.ulps_of, 0))
        if step[0] in ovflow:
            assert ovflow[step[0]] == w.overflow, f"{what}: the overflow word"
        if step[1] == "subset":
            assert routes[step[0]] == cc.subset_route(step, mats), f"{what}: {routes[step[0]]}"

    for step in chain.steps:
        wants[step[0]] = w = cc.rule(step, mats)
        link(producer, step, w)
    for claim in chain.claims:
        link(cc.check_claim, claim, mats, wants)
    for target, cons, g in got:
        link(_check_consumer_or_say_which, cons, dev[target], mats[target], g, Y, f"{name}: {target}")
    assert not missed, f"{len(missed)} link(s) of {name} miss their rule:\n" + "\n".join(missed)
    for operand, word in chain.refused:
        for f in (lambda: dev[operand].arith("*", 2.0), lambda: dev[operand].neg(), lambda: dev[operand].arith("+", dev[operand])):
            with pytest.raises(SparseArrayError, match=word):
                f()
