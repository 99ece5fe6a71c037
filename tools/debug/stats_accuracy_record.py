"""Worst observed err / bound per (operation, route) of the statistics accuracy cases (tests/stats_cases.py,
tests/exact_stats.py) -- the figures of profiles/stats_accuracy.txt.  A record, not a threshold: the tests assert <= 1.
  python tools/debug/stats_accuracy_record.py oracle|hip [out.txt]     ("hip" needs the GPU; it also runs the device level)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stats_cases as sc  # noqa: E402

who = sys.argv[1] if len(sys.argv) > 1 else "oracle"
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
rec = {}
if who == "oracle":
    from oracle import oracle_session
    sess = oracle_session()
else:
    import sparsearray_amd
    import test_hip_stats_accuracy as dev
    sess = sparsearray_amd.hip_session()
for name in sc.COLUMN_FORMS:
    for palette in sc.COLUMN_PALETTES[name]:
        c = sc.column_case(name, palette)
        sc.run_column_case(sess, c, rec, who)
        sc.run_summary_case(sess, c, rec, who)
        if c.inner == 1 and c.type == "double" and not c.planted and palette != "e":
            sc.run_dgc_case(sess, c, rec, who)
        if who == "hip" and not c.na_bg:
            sc.run_column_case(None, c, rec, "hip device level", colstat=dev.device_colstat(c))
for name in sc.ROW_ROUTES:
    for palette in sc.ROW_PALETTES[name]:
        c = sc.row_case(name, palette)
        sc.run_row_case(sess, c, rec, who)
        if who == "hip":
            sc.run_row_case(None, c, rec, "hip device level", rowstat=dev.device_rowstat(c))
for palette in ("a", "c_up", "c_down", "d"):
    for ngroup in (3, 1000):
        sc.run_groupsum_case(sess, sc.groupsum_case(palette, ngroup), rec, who)
for (w, op, route), worst in sorted(rec.items()):
    print(f"{w:18s} {op:32s} {route:22s} {worst:.3f}", file=out)
