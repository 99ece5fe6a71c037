"""Worst observed err / bound per (kernel, palette) of the product accuracy cases (tests/product_cases.py,
tests/exact_products.py) -- the figures of profiles/products_accuracy.txt.  A record, not a threshold: the tests assert
<= 1 for every cell (and identity for the integer tracer, recorded as 0).
  python tools/debug/products_accuracy_record.py oracle|hip [out.txt]     ("hip" needs the GPU; the chunked-gather
  cases run at their full width there, at K = 2 for the oracle)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import product_cases as pc  # noqa: E402

who = sys.argv[1] if len(sys.argv) > 1 else "oracle"
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
rec = {}
if who == "oracle":
    from oracle import oracle_session
    sess = oracle_session()
    for name in pc.DENSE_CASES:
        pc.run_dense_case_oracle(sess, name, rec)
    matmul, gram = pc.oracle_matmul(sess), pc.oracle_gram(sess)
else:
    import sparsearray_amd
    import test_hip_products_accuracy as dev
    from sparsearray_amd.device import set_gather_pacing, set_round_launches, set_spare_cus
    sess = sparsearray_amd.hip_session()
    # the knob settings the tests run a case under, besides the default ones
    knobs = {"many_blocks": [lambda: set_round_launches(2), lambda: set_round_launches(0)],
             "spare256p": [lambda: set_spare_cus(32)], "split16384": [lambda: set_spare_cus(32)]}
    for name, c in pc.DENSE_CASES.items():
        if not c.get("own"):
            pc.run_dense_case_device(name, rec, who)
            if name not in knobs:
                continue
        unpaced = c["plan"]["kernel"] != "gatherx" and c["plan"]["kind"] == "gather"
        for knob in ([None] if c.get("own") else []) + knobs.get(name, []):
            try:
                if unpaced:
                    set_gather_pacing(-1, 256)
                if knob is not None:
                    knob()
                for palette in c["palettes"]:
                    _, e, A, plan = dev._plan_of(name, palette)
                    pc.check_dense(pc.device_run(plan, e), e, name, rec, who, c["plan"]["kernel"])
            finally:
                set_gather_pacing()
                set_round_launches(1)
                set_spare_cus(0)
    matmul, gram = dev._device_matmul, dev._device_gram
for case in pc.HOST_CASES:
    pc.run_host_case(sess, *case, rec=rec, who=who)
for nrow in pc.MATMUL_ROWS:
    for types in pc.TYPE_PAIRS:
        pc.run_matmul_case(matmul, nrow, types, rec, who)
for name in pc.GRAM_ROWS:
    for types in pc.TYPE_PAIRS:
        pc.run_gram_case(gram, name, types, False, rec, who)
        if types[0] == types[1]:
            pc.run_gram_case(gram, name, types, True, rec, who, kernel="gram symmetric")
for (w, kernel, palette), worst in sorted(rec.items()):
    print(f"{w:18s} {kernel:22s} {palette:12s} {worst:.3f}", file=out)
