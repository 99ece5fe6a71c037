"""Every case of tests/ws_cases.py on the GPU: the device-level entry points of the product and row-statistics
families that take a caller's workspace, held to the contract of include/svt_hip.h ("Workspaces"):

  a. nothing is written outside [ws, ws + the advertised bytes) and the outputs -- the call runs in a 0xA5 arena with
     guard bands, and with one byte less it answers its own "workspace too small" before anything is written;
  b. every output cell is defined -- the outputs start as 0xA5 bytes and end as the expectation, bit for bit;
  c. the result does not depend on what the workspace held -- 0x00, 0xA5, 0xFF, and the workspace another operand of
     the table left behind all give the same output bytes and flag / warn words;
  d. the same for the degenerate operands, and for the not-finite flag: raised by one NaN / Inf / NA wherever it
     sits, and down again for clean operands in the same workspace.

The expectations are plain numpy on exact integers (tolerance 0); tests/test_ws_cases_cpu.py has asserted, without a
GPU, that every case sits on the route it names, and pinned the expectations against the oracle.  Every buffer a call
may write has at least GUARD bytes of the same allocation behind it."""
import contextlib

import numpy as np
import pytest

import ws_cases as wc
from helpers import GUARD, Arena, assert_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)


def _dev(op):
    from sparsearray_amd.device import DeviceCSC
    return DeviceCSC.from_host(op.nrow, op.cp, op.ri, op.val)


def _buf(n, fill=0xA5):
    """n bytes at the start of an allocation of n + GUARD"""
    return torch.full((n + GUARD,), fill, dtype=torch.uint8, device="cuda")[:n]


def _bytes(tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def _assert_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        w = np.ascontiguousarray(w)
        if g == w.tobytes():
            continue
        assert len(g) == w.nbytes, f"{what}: output {i} has {len(g)} bytes, the expectation {w.nbytes}"
        word = np.uint64 if w.dtype.itemsize == 8 else np.uint32
        ga = np.frombuffer(g, dtype=w.dtype)
        bad = np.flatnonzero(ga.view(word) != w.reshape(-1).view(word))
        raise AssertionError(f"{what}: output {i}: {bad.size} of {w.size} cells differ, the first at {bad[0]}: "
                             f"got {ga[bad[0]]!r}, want {w.reshape(-1)[bad[0]]!r}")


# ---------------------------------------------------------------------------
# one runner per entry point: the operands on the device, the advertised bytes, the call on (ws, outputs)
# ---------------------------------------------------------------------------
class Run:
    error = "workspace too small"
    has_prepared = False

    def __init__(self, case, ops=None):
        from sparsearray_amd.device import _check, _lib, _stream
        self.c, self.o = case, ops if ops is not None else wc.operands(case)
        self.lib, self.check, self.stream = _lib(), _check, _stream
        self.setup()

    def settings(self):
        return contextlib.nullcontext()

    def before(self, outs):
        """what the caller owes the call besides the buffers"""


class GramRun(Run):
    def settings(self):
        from sparsearray_amd.device import set_sparse_crossprod_panel

        @contextlib.contextmanager
        def panel():
            try:
                if self.c["panel"] is not None:
                    set_sparse_crossprod_panel(*self.c["panel"])
                yield
            finally:
                set_sparse_crossprod_panel(-1, -1)
        return panel()

    def setup(self):
        self.Xt = _dev(self.o["X"].t())                     # (transposed on the host: t() has tests of its own)
        self.Y = _dev(self.o["Y"])
        with self.settings():                               # sized after the panel setting
            self.ws_bytes = self.lib.svt_dev_crossprod_csc_csc_ws_bytes(self.Xt.handle)

    def call(self, ws, outs):
        out, flag = outs
        with self.settings():
            self.check(self.lib.svt_dev_crossprod_csc_csc(self.Xt.handle, self.Y.handle, int(self.c["sym"]), out.data_ptr(),
                                                          self.Xt.nrow, ws.data_ptr(), ws.numel(), flag.data_ptr(),
                                                          self.stream()))


class SpmmRun(Run):
    def setup(self):
        self.A, self.B = _dev(self.o["A"]), _dev(self.o["B"])
        self.ws_bytes = self.lib.svt_dev_matmul_csc_csc_ws_bytes(self.A.handle)

    def call(self, ws, outs):
        out, flag = outs
        self.check(self.lib.svt_dev_matmul_csc_csc(self.A.handle, self.B.handle, out.data_ptr(), self.A.nrow, ws.data_ptr(),
                                                   ws.numel(), flag.data_ptr(), self.stream()))


class SpmmPreparedRun(SpmmRun):
    has_prepared = True

    def setup(self):
        super().setup()
        self.B2 = _dev(self.o["B2"])

    def prepare(self, ws):
        self.check(self.lib.svt_dev_matmul_csc_csc_prepare(self.A.handle, ws.data_ptr(), ws.numel(), self.stream()))

    def prepared(self, ws, outs):
        for B, out, flag in ((self.B, outs[0], outs[1]), (self.B2, outs[2], outs[3])):
            self.check(self.lib.svt_dev_matmul_csc_csc_prepared(self.A.handle, B.handle, out.data_ptr(), self.A.nrow,
                                                                ws.data_ptr(), ws.numel(), flag.data_ptr(), self.stream()))

    def call(self, ws, outs):
        self.prepare(ws)
        self.prepared(ws, outs)


class RowsumsRun(Run):
    def setup(self):
        from sparsearray_amd.device import rowstats_form
        self.A = _dev(self.o["A"])
        if "row" in self.c:
            assert rowstats_form(self.A, "sum", self.c["inner"]) == wc.ROW_OPERANDS[self.c["row"]]["forms"]["sum"]
        self.ws_bytes = self.lib.svt_dev_rowstats_ws_bytes(self.A.nrow, self.A.ncol)

    def call(self, ws, outs):
        self.check(self.lib.svt_dev_rowsums(self.A.handle, 0, self.c["inner"], outs[0].data_ptr(), ws.data_ptr(), ws.numel(),
                                            self.stream()))


class RowsumsPreparedRun(RowsumsRun):
    has_prepared = True

    def prepare(self, ws):
        self.check(self.lib.svt_dev_rowsums_prepare(self.A.handle, self.c["inner"], ws.data_ptr(), ws.numel(), self.stream()))

    def prepared(self, ws, outs):
        self.check(self.lib.svt_dev_rowsums_prepared(self.A.handle, 0, self.c["inner"], outs[0].data_ptr(), ws.data_ptr(),
                                                     ws.numel(), self.stream()))

    def call(self, ws, outs):
        self.prepare(ws)
        self.prepared(ws, outs)


class RowstatsRun(Run):
    def setup(self):
        from sparsearray_amd.api import OPCODES
        from sparsearray_amd.device import rowstats_form
        self.A, self.oc = _dev(self.o["A"]), OPCODES[self.c["op"]]
        if "row" in self.c:                                 # the form the table states, for the operand as the device sees it
            forms = wc.ROW_OPERANDS[self.c["row"]]["forms"]
            for p in wc.ROW_PASSES[self.c["op"]]:
                assert rowstats_form(self.A, p, self.c["inner"]) == forms[p], f"{self.c['name']}: pass {p}"
        self.ws_bytes = self.lib.svt_dev_rowstats_ws_bytes_op(self.A.handle, self.oc, self.c["inner"])

    def before(self, outs):
        outs[1].zero_()                                     # the warn word is raised, never cleared, by the call

    def call(self, ws, outs):
        self.check(self.lib.svt_dev_rowstats(self.A.handle, self.oc, 0, None, self.c["inner"], outs[0].data_ptr(),
                                             outs[1].data_ptr(), ws.data_ptr(), ws.numel(), self.stream()))


class ColmediansRun(Run):
    def setup(self):
        self.A = _dev(self.o["A"])
        self.ws_bytes = self.lib.svt_dev_colmedians_ws_bytes(self.A.nnz, self.A.ncol)

    def call(self, ws, outs):
        self.check(self.lib.svt_dev_colmedians(self.A.handle, 0, outs[0].data_ptr(), ws.data_ptr(), ws.numel(), self.stream()))


class RowsumIdsRun(Run):
    """svt_dev_rowsum_prepare + _prepared: the workspace is the id buffer, which only the first call is told the size of"""
    error = "id buffer too small"
    has_prepared = True
    prepared_checks_ws = False

    def setup(self):
        self.A = _dev(self.o["A"])
        self.group = torch.as_tensor(wc.group_of(self.A.nrow, self.c["ngroup"])[0], device="cuda")
        self.ws_bytes = self.lib.svt_dev_rowsum_gid_bytes(self.A.handle)

    def prepare(self, ws):
        self.check(self.lib.svt_dev_rowsum_prepare(self.A.handle, self.group.data_ptr(), self.c["ngroup"], ws.data_ptr(),
                                                   ws.numel(), self.stream()))

    def prepared(self, ws, outs):
        self.check(self.lib.svt_dev_rowsum_prepared(self.A.handle, ws.data_ptr(), self.c["ngroup"], 0, outs[0].data_ptr(),
                                                    self.stream()))

    def call(self, ws, outs):
        self.prepare(ws)
        self.prepared(ws, outs)


class CscDenseRun(Run):
    def setup(self):
        self.A = _dev(self.o["A"])
        self.Y = torch.as_tensor(np.ascontiguousarray(self.o["Y"].T), device="cuda")       # (K, nrow): column-major
        self.ws_bytes = self.lib.svt_dev_crossprod_ws_bytes(self.A.nrow, self.A.ncol, self.c["K"])

    def call(self, ws, outs):
        A = self.A
        self.check(self.lib.svt_dev_crossprod_csc_dense(A.handle, self.Y.data_ptr(), A.nrow, self.c["K"], 0, outs[0].data_ptr(),
                                                        1, A.ncol, ws.data_ptr(), ws.numel(), self.stream()))


class PbcRun(CscDenseRun):
    def setup(self):
        from sparsearray_amd.device import PbcPlan
        super().setup()
        self.plan = PbcPlan(self.A, self.c["K"], *self.c["layout"])
        assert self.plan.plan()["kind"] == self.c["kind"], f"{self.c['name']}: {self.plan.plan()}"
        self.ws_bytes = self.lib.svt_dev_crossprod_pbc_ws_bytes(self.plan._p, self.c["K"])

    def call(self, ws, outs):
        A = self.A
        self.check(self.lib.svt_dev_crossprod_pbc(self.plan._p, A.handle, self.Y.data_ptr(), A.nrow, self.c["K"], 0,
                                                  outs[0].data_ptr(), 1, A.ncol, ws.data_ptr(), ws.numel(), self.stream()))


RUNNERS = {"gram": GramRun, "spmm": SpmmRun, "spmm_prepared": SpmmPreparedRun, "rowsums": RowsumsRun,
           "rowsums_prepared": RowsumsPreparedRun, "rowstats": RowstatsRun, "colmedians": ColmediansRun,
           "rowsum_prepared": RowsumIdsRun, "csc_dense": CscDenseRun, "pbc": PbcRun}


def _arena(run, want):
    ar = Arena([run.ws_bytes] + [np.asarray(w).nbytes for w in want])
    return ar, ar.part(0), [ar.part(i + 1) for i in range(len(want))]


def _run_in(run, ws, want):
    """the call on ``ws`` with fresh 0xA5 outputs; returns the output bytes"""
    outs = [_buf(np.asarray(w).nbytes) for w in want]
    run.before(outs)
    run.call(ws, outs)
    return _bytes(outs)


# ---------------------------------------------------------------------------
# a, b, c (and d for the degenerate operands): one test per case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_case(hip, name):
    from sparsearray_amd import SparseArrayError
    c = wc.BY_NAME[name]
    want = wc.expected(c)
    run = RUNNERS[c["entry"]](c)
    n = run.ws_bytes
    assert n > 1
    # a + b: inside the arena, every output cell written with the expected bits
    ar, ws, outs = _arena(run, want)
    run.before(outs)
    run.call(ws, outs)
    got = _bytes(outs)
    _assert_bits(got, want, name)
    assert ar.guards_intact(), f"{name}: a byte outside the workspace and the outputs was written"
    if run.has_prepared:
        # the prepared half alone, again, on the workspace as it stands: the same bytes
        for o in outs:
            o.fill_(0xA5)
        run.before(outs)
        run.prepared(ws, outs)
        assert _bytes(outs) == got, f"{name}: the second run on one prepared workspace differs"
        assert ar.guards_intact()
    # one byte short: the entry point's own error, before anything is written (the prepared half refuses it too)
    if run.has_prepared and getattr(run, "prepared_checks_ws", True):
        for o in outs:
            o.fill_(0xA5)
        keep = ws.clone()
        with pytest.raises(SparseArrayError, match=run.error):
            run.prepared(ws[:n - 1], outs)
        torch.cuda.synchronize()
        assert torch.equal(ws, keep) and all(bool((o == 0xA5).all()) for o in outs) and ar.guards_intact()
    ar.mem.fill_(0xA5)
    with pytest.raises(SparseArrayError, match=run.error):
        run.call(ws[:n - 1], outs)
    torch.cuda.synchronize()
    assert ar.untouched(), f"{name}: the refused call wrote something"
    # c: whatever the workspace held
    for fill in FILLS:
        assert _run_in(run, _buf(n, fill), want) == got, f"{name}: the result depends on a workspace of {fill:#04x} bytes"
    other = wc.other_case(c)
    orun = RUNNERS[other["entry"]](other)
    both = _buf(max(n, orun.ws_bytes))
    _run_in(orun, both[:orun.ws_bytes], wc.expected(other))
    assert _run_in(run, both[:n], want) == got, f"{name}: the result depends on what {other['name']} left in the workspace"


def test_every_case_has_a_runner():
    assert set(RUNNERS) == set(wc.ENTRIES)


# ---------------------------------------------------------------------------
# d: the not-finite flag
# ---------------------------------------------------------------------------
FLAG_RUNS = {"gram_gen": (GramRun, dict(sym=False, panel=None)), "gram_sym": (GramRun, dict(sym=True, panel=None)),
             "spmm": (SpmmRun, {}), "spmm_prepared": (SpmmPreparedRun, {})}


@pytest.mark.parametrize("form,place,value", wc.FLAG_CASES)
def test_flag_goes_up_and_comes_down(hip, form, place, value):
    clean, dirty, _ = wc.flag_operands(form, place, value)
    cls, case = FLAG_RUNS[form]
    case = dict(case, name=f"{form} {place} {value}")
    rd, rc = cls(case, dirty), cls(case, clean)
    assert rd.ws_bytes == rc.ws_bytes
    product, one, zero = wc.flag_expected(form, clean), np.ones(1, np.int32), np.zeros(1, np.int32)
    want = [product, zero] * (2 if form == "spmm_prepared" else 1)
    ar, ws, outs = _arena(rd, want)
    rd.call(ws, outs)
    got = _bytes(outs)
    for i in range(1, len(want), 2):
        assert got[i] == one.tobytes(), f"{case['name']}: flag word {np.frombuffer(got[i], np.int32)}, not 1"
    assert ar.guards_intact()
    # clean operands in the same workspace: the flag is down and the product exact
    for o in outs:
        o.fill_(0xA5)
    rc.call(ws, outs)
    _assert_bits(_bytes(outs), want, case["name"] + ", then clean operands")
    assert ar.guards_intact()


# ---------------------------------------------------------------------------
# the sharded sparse crossprod's local block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("where,value", wc.SHARD_CASES)
def test_sharded_block_is_the_reference_product(hip, oracle, where, value):
    """parallel.device_sparse_crossprod_block on one device, no process group: with a NaN / Inf / NA in either operand
    the kernel leaves its output alone, and the block must come from the dense-buffer route -- the reference's
    dirty-leaf result -- not from whatever the allocator handed out."""
    from sparsearray_amd import parallel
    A, B = wc.shard_operands(where, value)
    lp = parallel.device_sparse_crossprod_block(_dev(A))
    Bd = _dev(B)
    nbytes = A.ncol * B.ncol * 8
    pool = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")     # what torch.empty of the result's size gets next
    torch.cuda.synchronize()
    del pool
    got = lp((Bd.col_ptr, Bd.row_idx, Bd.val))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (A.ncol, B.ncol)
    assert int(lp.flag.item()) == (0 if where == "clean" else 1)
    want = np.asarray(oracle.crossprod(A.svt(), B.svt()))
    assert_equal(got.cpu().numpy(), want, tol=0, strict_na=True, what=f"block, {value} in {where}")
