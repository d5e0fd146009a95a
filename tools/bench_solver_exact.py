#!/usr/bin/env python
"""raz_solve_exact by itself and beside raz_solve_batch(exactly = 1) of the same build: positions/s and node visits/s (the counter
in the workspace), HIP-event timed on the caller's stream after one warm-up call, on positions of the tests' seeded generator
(tests/solver_batch_cases.py random_positions, seed 7000 + empties):
    65 536 positions of 10 empties, 4 096 of 12, 64 of 14 (tools/bench_solver_batch.py's sets): both calls, alternating in one
        process, `reps` runs each, medians with ranges; the answers are asserted identical before anything is timed;
    64 positions of 16, 17 and 18 empties (a depth above the build's RAZ_SOLVE_EXACT_MAX_EMPTIES is listed as refused, not run):
        every row as a batch of one (the slowest one `reps` times), the 64 as one batch, and
        4 096 rows (the 64 cycled) - a batch is run only where the smaller ones project it to stay under a minute.
Prints one JSON document.  --cache FILE keeps the generated positions (the playouts are host work: minutes for 65 536)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from bench_solver_batch import positions  # noqa: E402


class Call:
    """One of the two entry points on fixed device arrays; run() = (milliseconds by HIP events, node visits)."""

    def __init__(self, b, w, p, exact, max_empties):
        import torch
        from reversi_alpha_zero_amd._native import lib, check
        self.n, self.exact, self.lib, self.check = b.size, exact, lib, check
        self.d = [torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda()]
        self.mv = torch.empty(self.n, dtype=torch.int8, device="cuda")
        self.sc, self.st = torch.empty_like(self.mv), torch.empty(self.n, dtype=torch.uint8, device="cuda")
        if exact:
            self.nbytes = lib.raz_solve_exact_workspace_bytes(self.n, max_empties) + min(self.n * 65536, 1 << 31)
        else:
            self.nbytes = lib.raz_solve_batch_workspace_bytes(self.n, 14) + min(self.n * 4096, 1 << 31)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def run(self):
        import torch
        s = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ptr = [t.data_ptr() for t in self.d]
        out = [self.mv.data_ptr(), self.sc.data_ptr(), self.st.data_ptr(), self.ws.data_ptr(), self.nbytes, 0, s.cuda_stream]
        e0.record(s)
        if self.exact:
            self.check(self.lib.raz_solve_exact(*ptr, self.n, *out), "raz_solve_exact")
        else:
            self.check(self.lib.raz_solve_batch(*ptr, self.n, 1, *out), "raz_solve_batch")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), int(self.ws[:8].cpu().numpy().view(np.uint64)[0])

    def answers(self):
        return self.mv.cpu().numpy().tobytes() + self.sc.cpu().numpy().tobytes() + self.st.cpu().numpy().tobytes()


def note(*what):
    print(*what, file=sys.stderr, flush=True)   # progress: the document itself goes to stdout at the end


def summary(n, runs):
    ms = [r[0] for r in runs]
    med = statistics.median(ms)
    visits = statistics.median(r[1] for r in runs)
    return {"ms": [round(x, 3) for x in ms], "ms_median": round(med, 3), "ms_range": [round(min(ms), 3), round(max(ms), 3)],
            "positions_per_s": n / med * 1e3, "node_visits": [r[1] for r in runs], "node_visits_per_s": visits / med * 1e3}


def compare(name, b, w, p, empties, reps):
    exact, batch = Call(b, w, p, True, empties), Call(b, w, p, False, empties)
    exact.run(), batch.run()   # warm-up; the answers
    assert exact.answers() == batch.answers(), f"{name}: raz_solve_exact and raz_solve_batch(exactly = 1) differ"
    assert int((exact.st != 0).sum()) == 0
    runs = {"exact": [], "batch": []}
    for _ in range(reps):   # alternating
        runs["exact"].append(exact.run())
        runs["batch"].append(batch.run())
        note(name, "exact / batch ms", runs["exact"][-1][0], runs["batch"][-1][0])
    doc = {"case": name, "positions": int(b.size), "identical_answers": True,
           "raz_solve_exact": summary(b.size, runs["exact"]), "raz_solve_batch_exactly_1": summary(b.size, runs["batch"])}
    doc["speedup_median"] = doc["raz_solve_batch_exactly_1"]["ms_median"] / doc["raz_solve_exact"]["ms_median"]
    doc["ranges_apart"] = doc["raz_solve_exact"]["ms_range"][1] < doc["raz_solve_batch_exactly_1"]["ms_range"][0]
    return doc


def deep(empties, b, w, p, reps, minute_ms=60e3):
    doc = {"case": f"{empties} empties", "rows": int(b.size)}
    singles = []
    Call(b[:1], w[:1], p[:1], True, empties).run()   # warm-up
    for i in range(b.size):
        c = Call(b[i:i + 1], w[i:i + 1], p[i:i + 1], True, empties)
        singles.append(c.run())
        assert int(c.st[0]) == 0, f"row {i} of {empties} empties was not solved: status {int(c.st[0])}"
        note(empties, "empties, row", i, "alone: ms, visits", *singles[-1])
    ms = [s[0] for s in singles]
    worst = int(np.argmax(ms))
    c = Call(b[worst:worst + 1], w[worst:worst + 1], p[worst:worst + 1], True, empties)
    doc["batch_of_1"] = {"every_row_once_ms": [round(x, 1) for x in ms], "ms_median_over_rows": round(statistics.median(ms), 3),
                         "slowest_row": worst, "slowest_row_node_visits": singles[worst][1],
                         "slowest_row_again": summary(1, [c.run() for _ in range(reps)])}
    if sum(ms) < 2 * minute_ms:   # (a batch shares the chip: it takes less than its rows one by one)
        c = Call(b, w, p, True, empties)
        c.run()
        doc["batch_of_64"] = summary(b.size, [c.run() for _ in range(reps)])
        note(empties, "empties, the batch of", b.size, doc["batch_of_64"]["ms"])
    else:
        doc["batch_of_64"] = {"skipped": f"its rows one by one take {sum(ms) / 1e3:.0f} s"}
    k = 4096
    if "ms_median" in doc["batch_of_64"] and doc["batch_of_64"]["ms_median"] * k / b.size < minute_ms:
        idx = np.arange(k) % b.size
        c = Call(b[idx], w[idx], p[idx], True, empties)
        c.run()
        doc["batch_of_4096"] = summary(k, [c.run() for _ in range(reps)])
    else:
        doc["batch_of_4096"] = {"skipped": "projected from the batch of 64 to take a minute or more"}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n10", type=int, default=65536)
    ap.add_argument("--n12", type=int, default=4096)
    ap.add_argument("--n14", type=int, default=64)
    ap.add_argument("--ndeep", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of: e10, e12, e14, e16, e17, e18")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--prepare-only", action="store_true", help="generate (and cache) the positions, run nothing")
    ap.add_argument("--out", default=None, help="also write the document to this file")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    sets = {e: positions(e, n, a.cache) for e, n in ((10, a.n10), (12, a.n12), (14, a.n14), (16, a.ndeep), (17, a.ndeep), (18, a.ndeep)) if f"e{e}" not in skip}
    if a.prepare_only:
        return
    import torch
    import __graft_entry__ as g
    g.build()
    doc = {"tool": "tools/bench_solver_exact.py", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events on the caller's stream after one warm-up call; medians and [min, max] of `reps` runs, the two calls alternating",
           "reps": a.reps, "compared": [], "deep": []}
    for e in (10, 12, 14):
        if e in sets:
            doc["compared"].append(compare(f"{e} empties", *sets[e], e, a.reps))
    from reversi_alpha_zero_amd._native import lib
    for e in (16, 17, 18):
        if e in sets:
            if lib.raz_solve_exact_workspace_bytes(1, e) == 0:   # above this build's RAZ_SOLVE_EXACT_MAX_EMPTIES: every row would be refused
                doc["refused"] = doc.get("refused", []) + [f"{e} empties"]
                continue
            doc["deep"].append(deep(e, *sets[e], a.reps))
            if a.out:   # (kept as it grows: a run that is cut short leaves what it had measured)
                with open(a.out + ".partial", "wt") as f:
                    f.write(json.dumps(doc) + "\n")
    c14 = next((c for c in doc["compared"] if c["case"] == "14 empties"), None)
    if c14:   # every depth measured: its slowest row alone against the exhaustive 64 x 14 call of this session
        doc["limit"] = [{"empties": d["case"], "slowest_row_alone_ms": d["batch_of_1"]["slowest_row_again"]["ms_range"],
                         "raz_solve_batch_64x14_ms": c14["raz_solve_batch_exactly_1"]["ms_range"],
                         "stands": d["batch_of_1"]["slowest_row_again"]["ms_range"][1] <= c14["raz_solve_batch_exactly_1"]["ms_range"][0]}
                        for d in doc["deep"]]
    text = json.dumps(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "wt") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
