"""Worst observed err / bound per (entry point, launch form) of the rowsum / colsum cases (tests/groupsum_cases.py,
tests/exact_stats.py) -- the figures of profiles/groupsum_accuracy.txt.  A record, not a threshold: the tests assert <= 1
(and tolerance 0 on the tracer palette, which shows here as 0.000).
  python tools/debug/groupsum_accuracy_record.py oracle|hip [out.txt]     ("hip" needs the GPU; it also runs the device level)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import groupsum_cases as gc  # noqa: E402

who = sys.argv[1] if len(sys.argv) > 1 else "oracle"
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
if who == "oracle":
    from oracle import oracle_session
    sess, rec, dev = oracle_session(), {}, None
else:
    import sparsearray_amd
    import test_hip_groupsum_cases as dev
    sess, rec = sparsearray_amd.hip_session(), dev.REC
for name, palette in gc.ROWSUM_PARAMS:
    gc.run_rowsum_case(sess, name, palette, rec, who)
    if dev is not None:
        dev.test_device_rowsum(sess, name, palette)
        dev.test_prepared_sums(sess, name, palette)
for name in ("lds_table_g1000", "windowed_2W1"):
    for palette in gc.ALL:
        gc.run_dgc_case(sess, name, palette, rec, who)
for ngroup in gc.COLSUM_NGROUPS:
    for palette in gc.COLSUM_PALETTES:
        gc.run_colsum_case(sess, ngroup, palette, rec, who)
print(f"{'who':18s} {'entry point':26s} {'form':12s} worst err / bound", file=out)
for (w, entry, form), worst in sorted(rec.items()):
    print(f"{w:18s} {entry:26s} {form:12s} {worst:.6f}", file=out)
