#!/usr/bin/env python
"""raz_solve_batch by itself: positions/s and node visits/s (the counter in the workspace), HIP-event timed on the caller's
stream after one warm-up call, on positions of the tests' seeded generator (tests/solver_batch_cases.py random_positions):
    65 536 positions of 10 empties, each mode;  4 096 of 12 empties, exact;  64 of 14 empties, exact
and, on the same 10-empties positions, two comparators that are not the code under test:
    (a) the oracle's orc_solver_solve on the host (one core);
    (b) the on-device route that existed before this call: a SelfPlayEngine armed with set_positions(..., one_move=True) under
        use_solver_turn = 50, so that the pool's root solver answers them - positions/s including its rounds.
Prints one JSON document.  --cache FILE keeps the generated positions (the playouts are host work: minutes for 65 536)."""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def positions(empties, count, cache):
    import solver_batch_cases as C
    key = f"e{empties}_n{count}"
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if key + "_b" in z:
            return z[key + "_b"], z[key + "_w"], z[key + "_p"]
    b, w, p = C.arrays(C.random_positions(empties, count, 7000 + empties))
    if cache:
        old = dict(np.load(cache)) if os.path.exists(cache) else {}
        old.update({key + "_b": b, key + "_w": w, key + "_p": p})
        np.savez(cache, **old)
    return b, w, p


def bench_batch(name, b, w, p, exactly, reps):
    import torch
    from reversi_alpha_zero_amd._native import lib, check
    n = b.size
    db, dw, dp = torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda()
    mv = torch.empty(n, dtype=torch.int8, device="cuda")
    sc, st = torch.empty_like(mv), torch.empty(n, dtype=torch.uint8, device="cuda")
    nbytes = lib.raz_solve_batch_workspace_bytes(n, 14) + min(n * 4096, 1 << 31)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()

    def call():
        check(lib.raz_solve_batch(db.data_ptr(), dw.data_ptr(), dp.data_ptr(), n, exactly, mv.data_ptr(), sc.data_ptr(), st.data_ptr(),
                                  ws.data_ptr(), nbytes, 0, stream.cuda_stream), "raz_solve_batch")
    call()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    visits = int(ws[:8].cpu().numpy().view(np.uint64)[0])
    best = min(ms)
    assert int((st != 0).sum()) == 0
    return {"case": name, "positions": n, "exactly": exactly, "ms": ms, "positions_per_s": n / best * 1e3, "node_visits": visits,
            "node_visits_per_s": visits / best * 1e3, "workspace_bytes": nbytes, "first_answers": [[int(m), int(s)] for m, s in zip(mv[:4].cpu(), sc[:4].cpu())]}


def bench_oracle(b, w, p, exactly, count):
    import oracle as O
    lib = O.load_ext()
    mv, sc = ctypes.c_int(), ctypes.c_int()
    t0 = time.perf_counter()
    for i in range(count):
        s = lib.orc_solver_new()
        lib.orc_solver_solve(s, int(b[i]), int(w[i]), int(p[i]), exactly, ctypes.byref(mv), ctypes.byref(sc))
        lib.orc_solver_free(s)
    dt = time.perf_counter() - t0
    return {"comparator": "(a) oracle orc_solver_solve on the host", "cores": 1, "positions": count, "exactly": exactly, "seconds": dt,
            "positions_per_s": count / dt}


def bench_engine(b, w, p, slots):
    """(b): exact root solves by the engine's pool (agent/player.py:100-103,150-161), `slots` positions at a time."""
    import torch
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.engine import DeviceNet, SelfPlayEngine
    play = types.SimpleNamespace(
        simulation_num_per_move=8, share_mtcs_info_in_self_play=True, thinking_loop=1, required_visit_to_decide_action=40,
        start_rethinking_turn=10, c_puct=5, noise_eps=0.25, dirichlet_alpha=0.5, change_tau_turn=10, virtual_loss=3,
        parallel_search_num=1, resign_threshold=None, allowed_resign_turn=10, disable_resignation_rate=0.0,
        use_solver_turn=50, use_solver_turn_in_simulation=0)
    cfg = types.SimpleNamespace(play=play, play_data=types.SimpleNamespace(save_policy_of_tau_1=True))
    n = b.size
    db, dw, dp = torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda()
    eng = SelfPlayEngine(cfg, DeviceNet(ReversiNet(16, 1, 16).keras_init_(0).to_blob(), "cuda:0"), n_games=slots, seed=3, sims_hint=8)
    steps = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r0 in range(0, n, slots):
        r1 = min(n, r0 + slots)
        eng.start(0, 8)
        eng.set_positions(0, db[r0:r1].contiguous(), dw[r0:r1].contiguous(), dp[r0:r1].contiguous(), 8, enable_resign=False, one_move=True)
        for _ in range(100000):
            eng.step(8)
            steps += 8
            if eng.stats()["idle_or_done"] >= slots:
                break
        else:
            raise RuntimeError("the engine did not answer")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    raw = eng.read_raw()
    solved = int(sum(int(raw["headers"][g, 0]["flags"]) & 1 for g in range(min(slots, n - r0))))
    return {"comparator": "(b) SelfPlayEngine root solver (pool kernels), set_positions one_move under use_solver_turn=50", "positions": n,
            "slots": slots, "engine_steps": steps, "seconds": dt, "positions_per_s": n / dt, "exactly": 1, "last_round_rows_marked_solved": solved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n10", type=int, default=65536)
    ap.add_argument("--n12", type=int, default=4096)
    ap.add_argument("--n14", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-positions", type=int, default=256)
    ap.add_argument("--engine-slots", type=int, default=8192)
    ap.add_argument("--skip", default="", help="comma list of: e10, e12, e14, oracle, engine")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--prepare-only", action="store_true", help="generate (and cache) the positions, run nothing")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    sets = {}
    for e, n in ((10, a.n10), (12, a.n12), (14, a.n14)):
        if f"e{e}" not in skip or (e == 10 and not {"oracle", "engine"} <= skip):
            sets[e] = positions(e, n, a.cache)
    if a.prepare_only:
        return
    import torch
    import __graft_entry__ as g
    g.build()
    doc = {"tool": "tools/bench_solver_batch.py", "device": torch.cuda.get_device_name(0), "timing": "HIP events on the caller's stream, best of reps, after one warm-up call",
           "cases": [], "comparators": []}
    if "e10" not in skip:
        doc["cases"].append(bench_batch("10 empties", *sets[10], 0, a.reps))
        doc["cases"].append(bench_batch("10 empties", *sets[10], 1, a.reps))
    if "e12" not in skip:
        doc["cases"].append(bench_batch("12 empties", *sets[12], 1, a.reps))
    if "e14" not in skip:
        doc["cases"].append(bench_batch("14 empties", *sets[14], 1, 1))
    if "oracle" not in skip:
        for ex in (0, 1):
            doc["comparators"].append(bench_oracle(*sets[10], ex, min(a.oracle_positions, a.n10)))
    if "engine" not in skip:
        try:
            doc["comparators"].append(bench_engine(*sets[10], min(a.engine_slots, a.n10)))
        except Exception as ex:   # (reported, not hidden: the document says what did not run)
            doc["comparators"].append({"comparator": "(b) SelfPlayEngine root solver", "error": repr(ex)})
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
