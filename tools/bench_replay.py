"""Time the two routes from a self-play outbox to the trainer's packed rows on the device, in one process on the same games
(DESIGN.md section 4.9):

  (a) the device route: raz_train_rows_count + raz_train_rows_fill (csrc/raz_replay.hip), device events around
      lib/replay.rows_from_outbox - the row count's copy to the host and torch's allocations included - and around the two
      entries alone on preallocated outputs;
  (b) the file route: BatchedSelfPlayWorker.write_raw (the play_*.json text), then what OptimizeWorker.load_play_data does -
      read_game_data_from_file -> pack_game_data per file, one concatenation - and the upload, on the wall clock (the upload ends in
      a device synchronise).  The reading side is reported on its own too: it is what the `opt` worker pays.

  python tools/bench_replay.py [--games 4096] [--file-games 512] [--slots 2048] [--sims 8] [--reps 20] [--out profiles/r12/replay_rows.json]

All --games games go through (a); the first --file-games of them through (b) and, for the ratio, through (a) again on their own.
The rows of the two routes are compared byte for byte before any number is reported."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROW_BYTES = 8 + 8 + 256 + 1


def config_for(root, sims, nb_game_in_file):
    from reversi_alpha_zero_amd.config import Config
    cfg = Config()
    cfg.model.update(dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16))
    rc = cfg.resource
    rc.project_dir = rc.data_dir = root
    rc.model_dir = os.path.join(root, "model")
    rc.next_generation_model_dir = os.path.join(rc.model_dir, "next_generation")
    rc.play_data_dir = os.path.join(root, "play_data")
    rc.self_play_ggf_data_dir = os.path.join(root, "ggf")
    rc.log_dir = os.path.join(root, "logs")
    rc.force_simulation_num_file = os.path.join(root, ".force-sim")
    rc.self_play_game_idx_file = os.path.join(root, ".self-play-game-idx")
    cfg.play.schedule_of_simulation_num_per_move = [(0, sims)]
    cfg.play.update(dict(parallel_search_num=1, use_solver_turn=0, use_solver_turn_in_simulation=0, thinking_loop=1,
                         required_visit_to_decide_action=sims))
    cfg.play_data.update(dict(nb_game_in_file=nb_game_in_file, enable_ggf_data=False, max_file_num=1 << 30))
    rc.create_directories()
    return cfg


def timed(fn, reps, warmup=3):
    """Median and spread, in ms, of fn() between two device events on the synchronised stream."""
    ms = []
    for it in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def device_route(pk, cfg, reps):
    import ctypes
    from reversi_alpha_zero_amd._native import check, current_stream_ptr, lib
    from reversi_alpha_zero_amd.lib.replay import rows_from_outbox
    kw = dict(change_tau_turn=cfg.play.change_tau_turn, save_policy_of_tau_1=cfg.play_data.save_policy_of_tau_1)
    h, rn, sm = pk["headers"], pk["root_n"], pk["summary"]
    rows = rows_from_outbox(h, rn, sm, **kw)
    R, G, plies = len(rows[0]), h.shape[0], h.shape[1]
    whole = timed(lambda: rows_from_outbox(h, rn, sm, **kw), reps)
    own, enemy, policy, z, off = (torch.empty_like(t) for t in rows)

    def kernels():
        check(lib.raz_train_rows_count(h.data_ptr(), sm.data_ptr(), None, G, plies, off.data_ptr(), None, current_stream_ptr()), "count")
        check(lib.raz_train_rows_fill(h.data_ptr(), rn.data_ptr(), sm.data_ptr(), None, G, plies, int(kw["change_tau_turn"]),
                                      int(bool(kw["save_policy_of_tau_1"])), off.data_ptr(), R, own.data_ptr(), enemy.data_ptr(),
                                      policy.data_ptr(), z.data_ptr(), current_stream_ptr()), "fill")
    alone = timed(kernels, reps)
    assert all(torch.equal(a, b) for a, b in zip(rows, (own, enemy, policy, z, off)))
    read_bytes = h.numel() + rn.numel() * 4 + sm.numel()   # (an upper bound: plies beyond a game's end are skipped)
    return rows, {"games": G, "plies": plies, "rows": R, "rows_from_outbox": dict(whole, rows_per_s=R / (whole["median_ms"] * 1e-3)),
                  "count_and_fill_alone": dict(alone, rows_per_s=R / (alone["median_ms"] * 1e-3),
                                               written_GB_per_s=R * ROW_BYTES / (alone["median_ms"] * 1e-3) / 1e9,
                                               outbox_bytes=read_bytes, row_bytes=R * ROW_BYTES)}


def file_route(player, pk, cfg, dev):
    from reversi_alpha_zero_amd.engine import packed_to_host
    from reversi_alpha_zero_amd.lib.data_helper import get_game_data_filenames, pack_game_data, read_game_data_from_file
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    raw = packed_to_host(pk)
    player.write_raw(raw, 1)
    t1 = time.perf_counter()
    files = get_game_data_filenames(cfg.resource)
    parts = [pack_game_data(read_game_data_from_file(f)) for f in files]   # (one Python thread: OptimizeWorker.load_play_data)
    data = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    t2 = time.perf_counter()
    up = tuple(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in data)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    R = len(data[0])
    text = sum(os.path.getsize(f) for f in files)
    return up, {"games": len(raw["n_plies"]), "rows": R, "files": len(files), "text_bytes": text,
                "write_raw_s": t1 - t0, "read_and_pack_s": t2 - t1, "upload_s": t3 - t2, "whole_route_s": t3 - t0,
                "rows_per_s": R / (t3 - t0), "reading_side_rows_per_s": R / (t3 - t1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--file-games", type=int, default=512)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nb-game-in-file", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "replay_rows.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay needs a GPU: there is nothing to time without one")
    if a.file_games > a.games or a.file_games % a.nb_game_in_file:
        raise SystemExit("--file-games must be at most --games and a whole number of files")
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.worker.self_play import BatchedSelfPlayWorker
    dev = "cuda:0"
    root = tempfile.mkdtemp(prefix="bench_replay.")
    try:
        cfg = config_for(root, a.sims, a.nb_game_in_file)
        model = ReversiModel(cfg)
        model.build(seed=5)
        player = BatchedSelfPlayWorker(cfg, model.model.to_blob(), games_in_flight=min(a.slots, a.games), seed=3, device=dev, block_games=a.games)
        t0 = time.perf_counter()
        pk = player.play_block_continuous(0)(None)
        torch.cuda.synchronize()
        play_s = time.perf_counter() - t0
        _, all_games = device_route(pk, cfg, a.reps)
        sub = {k: pk[k][:a.file_games].contiguous() for k in ("headers", "root_n", "summary")}
        rows, same_games = device_route(sub, cfg, a.reps)
        up, files = file_route(player, sub, cfg, dev)
        for name, x, y in zip(("own", "enemy", "policy", "z"), rows, up):   # the two routes give the same bytes, or nothing is reported
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"{name}: the device rows are not the file route's"
        dr, fr = same_games["rows_from_outbox"]["rows_per_s"], files["rows_per_s"]
        result = {"what": "self-play outbox -> the trainer's packed rows on the device: count + fill against the play_*.json route",
                  "net": "16 filters x 1 residual layer, value_fc 16", "sims_per_move": a.sims, "play_s": play_s,
                  "device_route_all_games": all_games, "device_route_file_games": same_games, "file_route_file_games": files,
                  "rows_identical": True,
                  "ratio_device_over_file_route": dr / fr,
                  "ratio_device_over_reading_side": dr / files["reading_side_rows_per_s"],
                  "device": torch.cuda.get_device_name(0)}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
