#!/usr/bin/env python
"""Generate tests/golden/solver_exact_deep.json: positions of 15..17 empties of tests/solver_batch_cases.py's seeded generator
(seed 7100 + empties) with the answers of tests/native/ab_check.c - a plain host negamax with bounds that searches every root child
under the full window, so every root move's exact value is recorded beside the answer (the first maximum in ascending order):
    python tests/golden/make_golden_solver_exact_deep.py
ab_check itself is pinned to the oracle at 1..10 empties and on the 13 / 14 fixture by tests/test_solver_exact_host.py.  Recording
takes minutes on one core (a 17-empties position alone: tens of millions of node visits), which is why these answers
are recorded instead of being computed by the tests."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import solver_exact_cases as X  # noqa: E402


def main():
    out = {"_generator": "tests/golden/make_golden_solver_exact_deep.py", "positions": []}
    for e, (b, w, p) in X.deep2_positions():
        t = time.time()
        ans, values, nodes = X.ab_answer(b, w, p)
        out["positions"].append({"black": "0x%016x" % b, "white": "0x%016x" % w, "next_player": p, "empties": e, "exact": list(ans),
                                 "root_values": {str(s): v for s, v in sorted(values.items())}, "nodes": nodes})
        print(out["positions"][-1], "%.1f s" % (time.time() - t), flush=True)
    path = os.path.join(HERE, "solver_exact_deep.json")
    with open(path, "wt") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, len(out["positions"]), "positions")


if __name__ == "__main__":
    main()
