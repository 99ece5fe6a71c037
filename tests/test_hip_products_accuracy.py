"""The product kernels against the exact result: the cases of product_cases.py (operands built by hand at the edges of
the panel-blocked layouts, one per launch path, the value palettes) through the device-level entry points and the host
entry points, held to the rules of exact_products.py -- |got - E| <= gamma(n) M on every cell, identity for the integer
tracer -- with the plan each case names asserted through PbcPlan.plan().  test_products_accuracy_cpu.py holds the
reference to the same rules and shows what they reject; the 1e-9 / 1e-11 bar of the oracle-parity tests is a different,
much wider rule."""
import numpy as np
import pytest

import exact_products as xp
import product_cases as pc

pytestmark = pytest.mark.gpu


def _plan_of(name, palette="tracer"):
    """(case, expected, DeviceCSC, PbcPlan) of one of the cases that run in a test of their own."""
    from sparsearray_amd.device import DeviceCSC, PbcPlan
    c = pc.DENSE_CASES[name]
    e = pc.expected(c["structure"], palette, c["K"])
    A = DeviceCSC.from_host(e.st.nrow, e.st.cp, e.st.ri, e.val)
    return c, e, A, PbcPlan(A, c["K"], *c["layout"])


@pytest.mark.parametrize("name", pc.generic_device_cases())
def test_dense_cases(hip, name):
    """Every palette and output layout of one structural case through svt_dev_crossprod_pbc, on the plan it names."""
    pc.run_dense_case_device(name)


def test_spared_cus(hip):
    """set_spare_cus(32).  On the 16384-row operand the split rule of the spared launch (224 / units splits, at least
    16 panels each) gives 128 / 16 = 8 splits as the default rule does, in the packed workgroup order of the spared
    launch.  On 256 panels and 16 (column block, dense tile) units the two rules differ: 16 splits by default, 14 with
    the CUs spared, and the plan must say so."""
    from sparsearray_amd.device import set_spare_cus
    try:
        for palette in pc.STRUCTURAL:
            set_spare_cus(32)
            c, e, A, plan = _plan_of("split16384", palette)
            pc.assert_plan(plan.plan(), dict(c["plan"], nsplit=8, panels_per_split=16), "spared")
            pc.check_dense(pc.device_run(plan, e), e, "spare 32")
            set_spare_cus(0)
            c, e, A, plan = _plan_of("spare256p", palette)
            default = plan.plan()
            pc.assert_plan(default, c["plan"], "256 panels, no CU spared")
            pc.check_dense(pc.device_run(plan, e), e, "256 panels, no CU spared")
            set_spare_cus(32)
            spared = plan.plan()
            pc.assert_plan(spared, pc.SPARED_PLAN, "256 panels, 32 CUs spared")
            assert spared["nsplit"] != default["nsplit"]
            pc.check_dense(pc.device_run(plan, e), e, "256 panels, 32 CUs spared")
    finally:
        set_spare_cus(0)


@pytest.mark.parametrize("palette", pc.STRUCTURAL)
def test_many_column_blocks_rounds_and_cut_last_round(hip, palette):
    """263 column blocks of 80 leaves, no row split, direct write: one launch per round of workgroups, the last round
    cut by rows; the same with the last round whole (2) and in one launch (0).  The tracer makes the three results
    identical to E, hence to each other."""
    from sparsearray_amd.device import set_round_launches
    c, e, A, plan = _plan_of("many_blocks", palette)
    try:
        got = {}
        for mode in (1, 2, 0):
            set_round_launches(mode)
            p = plan.plan()
            pc.assert_plan(p, c["plan"], f"mode {mode}")
            if mode == 1:
                assert p["launches"] > 1 and p["tail_splits"] > 1 and p["tail_blocks"] > 0, p
            elif mode == 2:
                assert p["launches"] > 1 and p["tail_splits"] == 1, p
            else:
                assert p["launches"] == 1 and p["tail_splits"] == 1, p
            got[mode] = pc.device_run(plan, e)
            if palette == "tracer" or mode == 1:
                pc.check_dense(got[mode], e, f"round launches {mode}")
        # rounds do not change a sum: whole rounds and one launch add every cell in the same order
        assert np.array_equal(got[2], got[0])
        pc.check_dense(got[0], e, "round launches 0")
    finally:
        set_round_launches(1)


def test_from_first_col(hip):
    """svt_dev_crossprod_pbc_from on blocks of 80 leaves: first_col at 0, at a block boundary and one past it; the cells
    of leaves before the block of first_col keep the sentinel bit for bit, all others obey the rule."""
    sentinel = -1234.5
    for palette in pc.STRUCTURAL:
        c, e, A, plan = _plan_of("from_first_col", palette)
        for first_col, c_begin in ((0, 0), (80, 80), (81, 80)):
            pc.assert_plan(plan.plan(first_col=first_col), c["plan"], f"first_col {first_col}")
            got = pc.device_run(plan, e, first_col=first_col, sentinel=sentinel)
            assert np.all(got[:c_begin] == sentinel), f"first_col {first_col}: a cell before the block was written"
            full = got.copy()
            full[:c_begin] = pc.device_run(plan, e)[:c_begin]
            assert not np.any(full[c_begin:] == sentinel)
            pc.check_dense(full, e, f"first_col {first_col}")


def test_gather2_on_64_panels_with_pacing_off(hip):
    from sparsearray_amd.device import set_gather_pacing
    try:
        set_gather_pacing(-1, 256)
        for palette in pc.STRUCTURAL:
            c, e, A, plan = _plan_of("gather64p_unpaced", palette)
            pc.assert_plan(plan.plan(), c["plan"], "unpaced")
            pc.check_dense(pc.device_run(plan, e), e, "gather2, 64 panels")
    finally:
        set_gather_pacing()


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("sname", ["gatherx64", "gatherx67"])
def test_gatherx(hip, sname, K):
    """crossprod_pbc_gatherx_kernel on 64 and on 67 panels (the eighth XCD's share is short), the three accumulator
    widths, the default pacing and (0, 1): results never depend on the pacing."""
    from sparsearray_amd.device import DeviceCSC, PbcPlan, set_gather_pacing
    c = pc.DENSE_CASES[f"{sname}_K{K}"]
    try:
        for palette in pc.STRUCTURAL:
            e = pc.expected(sname, palette, K)
            A = DeviceCSC.from_host(e.st.nrow, e.st.cp, e.st.ri, e.val)
            for cbw in (16, 32, 40):
                plan = PbcPlan(A, K, cbw, 4, 9)
                got = []
                for pacing in ((1, 256), (0, 1)):
                    set_gather_pacing(*pacing)
                    pc.assert_plan(plan.plan(), dict(c["plan"], NV=(cbw + 15) // 16), f"cbw {cbw} pacing {pacing}")
                    got.append(pc.device_run(plan, e))
                pc.check_dense(got[0], e, f"cbw {cbw}")
                assert np.array_equal(got[0], got[1]), f"cbw {cbw}: the result depends on the pacing"
    finally:
        set_gather_pacing()


@pytest.mark.parametrize("name", ["chunks_gather", "chunks_gather2"])
def test_several_row_chunks_per_product(hip, name):
    """The second and later row chunks of crossprod_pbc_gather_kernel / crossprod_pbc_gather2_kernel, which add to
    the partial sums of the chunks before: 4096 wavefronts per launch, one split, 514 panels against chunks of 512
    (gather), 322 against 320 (gather2); half of the leaves hold a nonzero in the last chunk's rows.  One split and
    whole dense tiles: the chunks add up in `out` itself (the direct write), and in the partials when the output is
    given by rows (run with the tracer, whose rule is identity)."""
    from sparsearray_amd.device import set_gather_pacing
    try:
        set_gather_pacing(-1, 256)                          # (K = 128 and >= 64 panels would take the paced kernel)
        for palette in pc.STRUCTURAL:
            c, e, A, plan = _plan_of(name, palette)
            for variant in ("cm", "tr") if palette == "tracer" else ("cm",):
                p = plan.plan(**pc.plan_kwargs(e.K, variant))
                pc.assert_plan(p, dict(c["plan"], direct=variant == "cm"), f"{name} {variant}")
                assert p["launches"] >= 2
                pc.check_dense(pc.device_run(plan, e, variant), e, f"{name} {variant}")
            del A, plan
    finally:
        set_gather_pacing()


@pytest.mark.parametrize("K", [1, 24, 65])
def test_general_kernels(hip, K):
    """255 rows: an LDS-DMA layout without records, the general kernels answer; and CrossprodPlan on a double and on
    an integer operand."""
    import torch
    from sparsearray_amd.device import CrossprodPlan, DeviceCSC, PbcPlan
    for palette in pc.PALETTES:
        e = pc.expected("general255", palette, K)
        st = e.st
        A = DeviceCSC.from_host(st.nrow, st.cp, st.ri, e.val)
        plan = PbcPlan(A, K)
        pc.assert_plan(plan.plan(), dict(kind="none", kernel="general", launches=0), "255 rows")
        pc.check_dense(pc.device_run(plan, e), e, "PbcPlan, no records")
        pc.check_dense(pc.device_run(plan, e, "tr"), e, "PbcPlan, no records, by rows")
        Yd = torch.as_tensor(np.ascontiguousarray(e.Y.T), device="cuda")
        out = torch.full((K, st.ncol), 3.0, dtype=torch.float64, device="cuda")
        CrossprodPlan(A, K).run(Yd, st.nrow, out)
        torch.cuda.synchronize()
        pc.check_dense(out.cpu().numpy().T, e, "CrossprodPlan")
    e = pc.expected("general255", "tracer", K)
    Ai = DeviceCSC.from_host(e.st.nrow, e.st.cp, e.st.ri, e.val.astype(np.int32))
    Yi = torch.as_tensor(np.ascontiguousarray(e.Y.T.astype(np.int32)), device="cuda")
    out = torch.full((K, e.st.ncol), 3.0, dtype=torch.float64, device="cuda")
    CrossprodPlan(Ai, K).run(Yi, e.st.nrow, out)
    torch.cuda.synchronize()
    pc.check_dense(out.cpu().numpy().T, e, "CrossprodPlan, integer")


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("name", list(pc.NONFINITE_CASES))
def test_nonfinite_dense_operand(hip, oracle, name, saturated):
    """An Inf, a NaN and an NA in Y (or a saturated dense column): non-finite exactly where the reference is, with its
    class; every other cell obeys the finite rule."""
    import torch
    from sparsearray_amd.device import DeviceCSC, PbcPlan
    c = pc.NONFINITE_CASES[name]
    st, val, Y = pc.nonfinite_operands(name, saturated)
    want = np.asarray(oracle.crossprod(pc.svt_of(st, val), np.asfortranarray(Y)))
    A = DeviceCSC.from_host(st.nrow, st.cp, st.ri, val)
    plan = PbcPlan(A, c["K"], *c["layout"])
    pc.assert_plan(plan.plan(), dict(kind=name, kernel=c["kernel"]), name)
    out = torch.full((c["K"], st.ncol), 3.0, dtype=torch.float64, device="cuda")
    plan.run(torch.as_tensor(np.ascontiguousarray(Y.T), device="cuda"), st.nrow, out)
    torch.cuda.synchronize()
    v = xp.check_with_nonfinite(out.cpu().numpy().T, want, st.cp, st.ri, val, Y, name).require()
    assert v.ncompared == int((np.isfinite(want) & (np.diff(st.cp)[:, None] > 0)).sum())


def _assert_host_layout(sname):
    from sparsearray_amd.device import DeviceCSC, PbcPlan
    st = pc.structure(sname)
    A = DeviceCSC.from_host(st.nrow, st.cp, st.ri, pc.tracer_a(st.ri, st.leaf))
    pc.assert_plan(PbcPlan(A, pc.HOST_K, 0, 0, 0).plan(), dict(kind=pc.HOST_LAYOUT[sname]), f"{sname}, layout by density")


@pytest.mark.parametrize("case", pc.HOST_CASES, ids="-".join)
def test_host_entry_points(hip, case):
    """svt_crossprod2_SVT_mat, svt_crossprod2_mat_SVT and svt_matmul_SVT_mat at 0.5 % and 0.1 % density (the automatic
    layout picks LDS-DMA for the first and gather for the second, asserted on the layout chosen by density), double
    and integer."""
    _assert_host_layout(case[0])
    pc.run_host_case(hip, *case)


def test_host_entry_points_wide_dense_operand(hip):
    """More than 512 dense columns: the host entry point runs the product chunk by chunk; the tracer's integers."""
    _assert_host_layout("host_wide")
    pc.run_host_case(hip, "host_wide", "double", "tracer", K=600)


def _device_matmul(A, B, va, vb):
    import torch
    from sparsearray_amd.device import DeviceCSC, matmul_csc_csc
    out, flag = matmul_csc_csc(DeviceCSC.from_host(A.nrow, A.cp, A.ri, va), DeviceCSC.from_host(B.nrow, B.cp, B.ri, vb))
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return out.cpu().numpy().T


def _device_gram(X, Y, vx, vy, sym):
    import torch
    from sparsearray_amd.device import DeviceCSC, crossprod_csc_csc
    Xd = DeviceCSC.from_host(X.nrow, X.cp, X.ri, vx)
    Yd = Xd if sym else DeviceCSC.from_host(Y.nrow, Y.cp, Y.ri, vy)
    out, flag = crossprod_csc_csc(Xd.t(), Yd, sym=sym)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return out.cpu().numpy().T


@pytest.mark.parametrize("types", pc.TYPE_PAIRS, ids="-".join)
@pytest.mark.parametrize("nrow", pc.MATMUL_ROWS)
def test_sparse_matmul(hip, nrow, types):
    """svt_dev_matmul_csc_csc: result rows on both sides of the 8192-row LDS panel, every type combination."""
    pc.run_matmul_case(_device_matmul, nrow, types)


@pytest.mark.parametrize("panels", [False, True], ids=["one_block", "panels"])
@pytest.mark.parametrize("types", pc.TYPE_PAIRS, ids="-".join)
@pytest.mark.parametrize("name", list(pc.GRAM_ROWS))
def test_sparse_crossprod(hip, name, types, panels):
    """svt_dev_crossprod_csc_csc: the general form for every type combination (the mixed ones included), the
    symmetric form for equal types (bit-symmetric, n = rows where both columns meet); one block of cells and panels
    (of 64 columns, or of 256 where the case is built for the wider lane groups).  The cases put the walk of a lane
    group -- after launch_gram's division by the panels and its halving in the symmetric form -- on the three sides of
    the lane-group widths, in each form and blocking (product_cases.GRAM_ROWS asserts the arithmetic); one has a row
    of 100 means."""
    from sparsearray_amd.device import set_sparse_crossprod_panel
    try:
        set_sparse_crossprod_panel(*pc.gram_panel(name, panels))
        pc.run_gram_case(_device_gram, name, types)
        if types[0] == types[1]:
            pc.run_gram_case(_device_gram, name, types, sym=True)
    finally:
        set_sparse_crossprod_panel(-1, -1)
