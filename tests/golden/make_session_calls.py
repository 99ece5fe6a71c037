#!/usr/bin/env python3
"""Generate tests/golden/session_calls.json: what ``Session`` over the CPU oracle's dispatcher returns for every call of
tests/session_calls_cases.py (order_cases() and row_cases()), and the ``.Call`` names every row statistic issued.

session_calls.json was written by this script on commit 6957427 ("Host-level statistics: one body per family in
svt_hip.cpp"), the last one whose Session held the host statements of the order statistics and of x[i, j] and chose the
route of a row statistic in five places.  tests/test_session_calls_cpu.py requires the same results of every later
Session; its route table is a literal of its own, and the "routes" recorded here are only what that literal was checked
against when it was written.  Running the script on a later commit must reproduce the file byte for byte.

Run:  python tests/golden/make_session_calls.py   (rewrites session_calls.json)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import session_calls_cases as sc                     # noqa: E402
from oracle import oracle_session                    # noqa: E402


def main():
    orc, ops = oracle_session(), sc.operands()
    results, routes = {}, {}
    for cid, m, key, args, kw in sc.order_cases():
        results[cid] = sc.encode(sc.run(orc, ops, m, key, args, kw)[0])
    for cid, m, key, kw, full in sc.row_cases():
        res, calls = sc.run(orc, ops, m, key, (), kw, full)
        results[cid], routes[cid] = sc.encode(res), calls
    with open(os.path.join(HERE, "session_calls.json"), "w") as f:
        json.dump({"commit": "6957427", "results": results, "routes": routes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(results), "results")


if __name__ == "__main__":
    main()
