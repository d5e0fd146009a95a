#!/usr/bin/env python
"""Generate tests/golden/solver_batch_deep.json: the positions of 13 and 14 empties of tests/solver_batch_cases.py's seeded
generator with the answers of the oracle's end-game solver (oracle/orc_solver.c, pinned to the reference's compiled Cython solver
by tests/test_oracle_solver.py) in both modes:
    python tests/golden/make_golden_solver_batch_deep.py
An exact solve takes the oracle about 11 s at 13 empties and 78 s at 14 on one core, which is why these answers are recorded
instead of being computed by the tests."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import solver_batch_cases as C  # noqa: E402


def main():
    out = {"_generator": "tests/golden/make_golden_solver_batch_deep.py", "positions": []}
    for e, count in C.DEEP_COUNTS.items():
        for b, w, p in C.random_positions(e, count, 7000 + e):
            t = time.time()
            ne, ex = C.oracle_answer(b, w, p, 0), C.oracle_answer(b, w, p, 1)
            out["positions"].append({"black": "0x%016x" % b, "white": "0x%016x" % w, "next_player": p, "empties": e,
                                     "exact": list(ex), "non_exact": list(ne)})
            print(out["positions"][-1], "%.1f s" % (time.time() - t), flush=True)
    path = os.path.join(HERE, "solver_batch_deep.json")
    with open(path, "wt") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, len(out["positions"]), "positions")


if __name__ == "__main__":
    main()
