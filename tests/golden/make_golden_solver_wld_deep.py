#!/usr/bin/env python
"""Generate tests/golden/solver_wld_deep.json: positions of 18..21 empties of tests/solver_batch_cases.py's seeded generator
(seed 7200 + empties; 4 each at 18, 19 and 20, 2 at 21) with the answers of tests/native/wld_check.c - a plain host negamax over
win / draw / loss that searches every root move under the window (-1, +1), so every root move's own outcome is recorded beside the
answer (the best outcome and the lowest-numbered move that has it), with its node visits and its seconds on one core:
    python tests/golden/make_golden_solver_wld_deep.py
wld_check itself is pinned to ab_check's root values at 1..10 empties and to the recorded ones at 15..17 by
tests/test_solver_wld_host.py.  A position takes up to some ten seconds, which is why these answers are recorded instead of being
computed by the tests.  (No 22 empties: one such row took 8 minutes.)"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import solver_wld_cases as W  # noqa: E402


def main():
    out = {"_generator": "tests/golden/make_golden_solver_wld_deep.py", "positions": []}
    for e, (b, w, p) in W.deep3_positions():
        t = time.time()
        ans, outcomes, nodes = W.wld_answer(b, w, p)
        out["positions"].append({"black": "0x%016x" % b, "white": "0x%016x" % w, "next_player": p, "empties": e, "wld": list(ans),
                                 "root_outcomes": {str(s): v for s, v in sorted(outcomes.items())}, "nodes": nodes,
                                 "seconds": round(time.time() - t, 2)})
        print(out["positions"][-1], flush=True)
    path = os.path.join(HERE, "solver_wld_deep.json")
    with open(path, "wt") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, len(out["positions"]), "positions")


if __name__ == "__main__":
    main()
