"""The bits of everything kernels_colstats.hip computes, one line per key: SHA-256 of the result's bytes (and of the
same with every NaN that is not NA as one pattern) plus the warn word.  For a change that must not move any arithmetic: run it over the library before and after, and compare.
  run  [--lib PATH] --out FILE    every (form, palette) case of tests/stats_cases.py, every op of COL_OPS (any / all for
                                  integers; centered_X2_sum, var1, sd1 without and with a given centre), both na_rm, at
                                  three levels: the host entry points (_colStats), the device level (device.colstats:
                                  out and warn), the whole-array summaries; the dgCMatrix column statistics of the
                                  doubles without planted NAs.  --lib: another build of the library (same ABI) under
                                  this tree's Python.  Needs the GPU.
  diff A B                        the keys whose lines differ, the count of keys compared and how many differ in more
                                  than the bits of a NaN; exit status 1 if any differs"""
import argparse
import hashlib
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CENTRED = ("centered_X2_sum", "var1", "sd1")


def digest(res, one_nan=False):
    """``one_nan``: every NaN that is not NA_real_ as one bit pattern first (which NaN an operation on two NaNs gives
    back depends on the operand order the compiler chose)"""
    import numpy as np
    from sparsearray_amd import is_NA_real
    h = hashlib.sha256()
    for a in (res if isinstance(res, (tuple, list)) else (res,)):
        a = np.ascontiguousarray(np.asarray(a))
        if one_nan and a.dtype == np.float64:
            a = np.where(np.isnan(a) & ~is_NA_real(a), np.nan, a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def run(args):
    import numpy as np
    from sparsearray_amd import _hip
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    import sparsearray_amd
    import stats_cases as sc
    from sparsearray_amd import device
    hip = sparsearray_amd.hip_session()
    out = open(args.out, "w")

    def line(key, f):
        """``f() -> (result, warn word or None)``; a session says it by the warning instead"""
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with np.errstate(all="ignore"):
                try:
                    res, warn = f()
                    text = f"bits={digest(res)} one_nan={digest(res, True)}"
                except Exception as e:                           # (an answer too: it must not change either)
                    text, warn = f"{type(e).__name__}: {e}", None
        if warn is None:
            warn = int(any(sc.NO_VALUE in str(m.message) for m in w))
        print(f"{key}\t{text} warn={warn}", file=out, flush=True)

    for name in sc.COLUMN_FORMS:
        for palette in sc.COLUMN_PALETTES[name]:
            c = sc.column_case(name, palette)
            is_int = c.type == "integer"
            A = None if c.na_bg else device.DeviceCSC.from_host(c.nrow, c.col_ptr, c.row_idx, c.val)
            for na_rm in (False, True):
                for op in sc.COL_OPS + (["any", "all"] if is_int else []):
                    if na_rm and op in ("anyNA", "countNAs"):    # (no na.rm there)
                        continue
                    for center in ((None, c.center) if op in CENTRED else (None,)):
                        key = f"{name}/{palette} {op} na_rm={int(na_rm)} center={'none' if center is None else 'given'}"
                        line("host    " + key, lambda: (hip._colStats(op, c.x, na_rm, center, c.dims), None))
                        if A is not None:
                            def dev():
                                res, warn = device.colstats(A, op, na_rm, float("nan") if center is None else center,
                                                            c.inner)
                                return res.cpu().numpy(), int(warn.cpu().numpy().any())
                            line("device  " + key, dev)
                for op in sc.SUMMARY_OPS + (["any", "all"] if is_int else []):
                    if na_rm and op in ("anyNA", "countNAs"):
                        continue
                    kw = {} if op in ("anyNA", "countNAs") else {"na_rm": na_rm}
                    line(f"summary {name}/{palette} {op} na_rm={int(na_rm)}", lambda: (getattr(hip, op)(c.x, **kw), None))
            if c.inner == 1 and c.type == "double" and not c.planted:
                x = ((c.nrow, c.nseg), c.col_ptr.astype(np.int32), c.row_idx, c.val)
                for f in ("colMins_dgCMatrix", "colMaxs_dgCMatrix", "colRanges_dgCMatrix", "colVars_dgCMatrix"):
                    line(f"dgC     {name}/{palette} {f}", lambda: (getattr(hip, f)(x), None))
    out.close()


def diff(args):
    a, b = ({ln.split("\t")[0]: ln for ln in open(p).read().splitlines()} for p in (args.a, args.b))
    keys = sorted(set(a) | set(b))
    differ = [k for k in keys if a.get(k) != b.get(k)]
    one_nan = lambda ln: None if ln is None else ln.split("\t")[1].split(" ", 1)[-1]
    beyond = [k for k in differ if one_nan(a.get(k)) != one_nan(b.get(k))]
    for k in differ:
        print(f"< {a.get(k)}\n> {b.get(k)}")
    print(f"{args.a} vs {args.b}: {len(keys)} keys, {len(differ)} differ, "
          f"{len(beyond)} of them in more than which NaN a NaN result is")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", default=None)
    r.add_argument("--out", required=True)
    d = sub.add_parser("diff")
    d.add_argument("a")
    d.add_argument("b")
    args = ap.parse_args()
    sys.exit(run(args) if args.cmd == "run" else diff(args))


if __name__ == "__main__":
    main()
