#!/usr/bin/env python
"""raz_solve_wld on the fixture rows of tests/golden (solver_exact_deep.json at 15..17 empties, solver_wld_deep.json at 18 and
above), HIP-event timed on the caller's stream after one warm-up call:
    for every fixture depth this build accepts, every row as a batch of one (`reps` runs, median) and the rows as one batch, with
        the node visits of each (the counter in the workspace) - the answers are asserted equal to the fixture's before anything
        is timed;
    at 15..17 empties the same rows through raz_solve_exact, the two calls alternating, and on the 17-empties rows raz_solve_wld
        with record cuts off (tuning bit 26);
    the one-core time of tests/native/wld_check.c on every row: the fixture's at 18 and above, taken here at 15..17;
    raz_solve_batch(exactly = 1) on 64 positions of 14 empties (tools/bench_solver_batch.py's set) in the same process: the bar
        the limit rule of DESIGN.md measures the slowest single row of a depth against.
Prints one JSON document; --out FILE also writes it (and FILE.partial as it grows)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from bench_solver_batch import positions  # noqa: E402
from bench_solver_exact import note  # noqa: E402

NO_CUTS = 1 << 26


class Call:
    """One entry point ("wld", "exact" or "batch") on fixed device arrays; run() = (milliseconds by HIP events, node visits)."""

    def __init__(self, cases, which, tuning=0):
        import torch
        import solver_batch_cases as C
        from reversi_alpha_zero_amd._native import lib, check
        b, w, p = C.arrays(cases)
        self.n, self.which, self.tuning, self.lib, self.check = b.size, which, tuning, lib, check
        deepest = max(64 - bin(int(x) | int(y)).count("1") for x, y in zip(b, w))
        self.d = [torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda()]
        self.mv = torch.empty(self.n, dtype=torch.int8, device="cuda")
        self.sc, self.st = torch.empty_like(self.mv), torch.empty(self.n, dtype=torch.uint8, device="cuda")
        size = {"wld": lib.raz_solve_wld_workspace_bytes, "exact": lib.raz_solve_exact_workspace_bytes,
                "batch": lib.raz_solve_batch_workspace_bytes}[which]
        self.nbytes = size(self.n, deepest) + min(self.n * 65536, 1 << 31)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def run(self):
        import torch
        s = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ptr = [t.data_ptr() for t in self.d]
        out = [self.mv.data_ptr(), self.sc.data_ptr(), self.st.data_ptr(), self.ws.data_ptr(), self.nbytes, self.tuning, s.cuda_stream]
        e0.record(s)
        if self.which == "batch":
            self.check(self.lib.raz_solve_batch(*ptr, self.n, 1, *out), "raz_solve_batch")
        else:
            self.check(getattr(self.lib, "raz_solve_" + self.which)(*ptr, self.n, *out), "raz_solve_" + self.which)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), int(self.ws[:8].cpu().numpy().view(np.uint64)[0])

    def answers(self):
        return list(zip(self.mv.cpu().tolist(), self.sc.cpu().tolist(), self.st.cpu().tolist()))


def summary(runs):
    ms = [r[0] for r in runs]
    return {"ms": [round(x, 3) for x in ms], "ms_median": round(statistics.median(ms), 3), "node_visits": [r[1] for r in runs]}


def timed(cases, which, reps, tuning=0, want=None):
    c = Call(cases, which, tuning)
    c.run()   # warm-up; the answers
    if want is not None:
        assert c.answers() == want, (which, hex(tuning), c.answers(), want)
    return c, summary([c.run() for _ in range(reps)])


def depth(e, cases, cpu_seconds, reps, with_exact, with_cuts_off):
    import solver_wld_cases as W
    want = [(c[4][1][0], c[4][1][1], 0) for c in cases]
    doc = {"empties": e, "rows": len(cases), "wld_check_one_core_s": cpu_seconds, "rows_alone": []}
    for i, c in enumerate(cases):
        row = {"row": i, "raz_solve_wld": timed([c], "wld", reps, want=want[i:i + 1])[1]}
        if with_exact:
            x, row["raz_solve_exact"] = timed([c], "exact", reps)
            assert [W.sign(s) for _, s, _ in x.answers()] == [want[i][1]], "raz_solve_exact's sign differs"
        if with_cuts_off:
            row["raz_solve_wld_cuts_off"] = timed([c], "wld", 1, tuning=NO_CUTS, want=want[i:i + 1])[1]
        doc["rows_alone"].append(row)
        note(e, "empties, row", i, {k: v["ms_median"] for k, v in row.items() if isinstance(v, dict)})
    slow = max(doc["rows_alone"], key=lambda r: r["raz_solve_wld"]["ms_median"])
    doc["slowest_row_alone"] = {"row": slow["row"], "ms_median": slow["raz_solve_wld"]["ms_median"], "ms": slow["raz_solve_wld"]["ms"]}
    # the rows as one batch, the two calls alternating
    wld, exact = Call(cases, "wld"), (Call(cases, "exact") if with_exact else None)
    wld.run()
    assert wld.answers() == want
    runs = {"wld": [], "exact": []}
    if exact:
        exact.run()
    for _ in range(reps):
        runs["wld"].append(wld.run())
        if exact:
            runs["exact"].append(exact.run())
    doc["one_batch"] = {"raz_solve_wld": summary(runs["wld"])}
    if exact:
        doc["one_batch"]["raz_solve_exact"] = summary(runs["exact"])
        a, b = doc["one_batch"]["raz_solve_wld"], doc["one_batch"]["raz_solve_exact"]
        doc["one_batch"]["wld_faster_ranges_apart"] = max(a["ms"]) < min(b["ms"])
        doc["one_batch"]["wld_fewer_visits"] = max(a["node_visits"]) < min(b["node_visits"])
    if with_cuts_off:
        off = timed(cases, "wld", reps, tuning=NO_CUTS, want=want)[1]
        doc["one_batch"]["raz_solve_wld_cuts_off"] = off
        doc["one_batch"]["cuts_save_visits"] = max(doc["one_batch"]["raz_solve_wld"]["node_visits"]) < min(off["node_visits"])
    note(e, "empties, one batch", {k: v["ms"] for k, v in doc["one_batch"].items() if isinstance(v, dict)})
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depths", default="15,16,17,18,19,20,21")
    ap.add_argument("--no-bar", action="store_true", help="skip the 64 x 14 exhaustive call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import solver_wld_cases as W
    from reversi_alpha_zero_amd._native import lib
    doc = {"tool": "tools/bench_solver_wld.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "HIP events on the caller's stream after one warm-up call; medians of `reps` runs", "depths": []}
    rows = {}
    for c in W.deep2_cases():
        t = time.time()
        W.wld_answer(*c[:3])
        rows.setdefault(W.empties_of(c), []).append((c, round(time.time() - t, 2)))
    for c, p in zip(W.deep3_cases(), W.deep3_doc()["positions"]):
        rows.setdefault(p["empties"], []).append((c, p["seconds"]))
    if not a.no_bar:
        bar = timed(list(zip(*[x.tolist() for x in positions(14, 64, None)])), "batch", a.reps)[1]
        doc["raz_solve_batch_exactly_1_64x14"] = bar
        note("64 x 14 exhaustive", bar["ms"])
    for e in [int(x) for x in a.depths.split(",")]:
        if lib.raz_solve_wld_workspace_bytes(1, e) == 0:
            doc["refused"] = doc.get("refused", []) + [e]
            continue
        cases = [c for c, _ in rows[e]]
        doc["depths"].append(depth(e, cases, [s for _, s in rows[e]], a.reps, e <= 17, e == 17))
        if a.out:   # (kept as it grows: a run that is cut short leaves what it had measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out + ".partial", "wt") as f:
                f.write(json.dumps(doc) + "\n")
    if not a.no_bar:   # the limit rule: a depth stands where its slowest row alone (median) takes no longer than the 64 x 14 call
        doc["limit"] = [{"empties": d["empties"], "slowest_row_alone_ms_median": d["slowest_row_alone"]["ms_median"],
                         "raz_solve_batch_64x14_ms_median": bar["ms_median"],
                         "stands": d["slowest_row_alone"]["ms_median"] <= bar["ms_median"]} for d in doc["depths"] if d["empties"] >= 18]
    if a.out:
        with open(a.out, "wt") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
