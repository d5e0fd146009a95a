"""Time a round robin of four models by two routes, in one process, alternating (README / DESIGN.md section 4.12):

  league   worker/league.py LeagueWorker: M = 4 models, games_per_pair = 34 - 204 games, all at once, in one engine.DeviceLeague;
  matches  the same six pairings as six engine.DeviceMatch runs of 34 games, one after the other (EvaluateWorker(handoff="device")), on
           engines configured the same.

  python tools/bench_league.py [--reps 3] [--cases mini,256x10] [--games-per-pair 34] [--out profiles/r17/league_ab.json]

Cases are tools/bench_match.py's.  The two routes play DIFFERENT games (slots, ids and colour draws differ), so nothing is compared across
them; before timing, 8 of the league's games are replayed by a host driver (ReversiEnv objects, one raz_engine_set_position per ply on
the mapped slot) and must be the league's, and the matches' results must be consistent with themselves.  Per route: wall clock (median
and range over --reps runs, after one untimed run each), games and plies per second, engine steps and launching calls (counted as
tools/bench_match.py counts them)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_match import CASES, Calls  # noqa: E402

MODELS = 4
PAIRS = [(i, j) for i in range(MODELS) for j in range(i + 1, MODELS)]
SYNCING = ("SelfPlayEngine.stats", "DeviceMatch.stats", "DeviceMatch.read", "DeviceLeague.stats", "DeviceLeague.read")


class LeagueCalls(Calls):
    def __init__(self):
        from reversi_alpha_zero_amd.engine import DeviceLeague
        super().__init__()
        for name in ("start", "turn", "stats", "read"):
            self._wrap(DeviceLeague, name)


def play_league(cfg, nets, gpp, seed, calls, keep=False):
    from reversi_alpha_zero_amd.worker.league import LeagueWorker
    w = LeagueWorker(cfg, nets, games_per_pair=gpp, seed=seed)
    calls.take()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w.play()
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return t, len(w.last_results), sum(len(g["plies"]) for g in w.last_games), calls.take(), (w if keep else None)


def play_matches(cfg, nets, gpp, seed, calls):
    from reversi_alpha_zero_amd.worker.evaluate import EvaluateWorker
    calls.take()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    games = plies = 0
    for k, (i, j) in enumerate(PAIRS):
        w = EvaluateWorker(cfg, seed=16 * seed + k, device="cuda:0", handoff="device")
        results = w.play_games(nets[i], nets[j], gpp)
        for (ng_win, best_is_black, (blacks, whites)), g in zip(results, w.last_games):   # consistent with themselves
            resigned = g["plies"][-1]["action"] < 0
            assert len(g["plies"]) >= 1 and blacks + whites <= 64 and g["best_is_black"] == best_is_black
            if not resigned:
                won_by_black = None if blacks == whites else blacks > whites
                assert ng_win == (None if won_by_black is None else int(won_by_black != best_is_black)), (k, g["game_id"])
        games += len(results)
        plies += sum(len(g["plies"]) for g in w.last_games)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, games, plies, calls.take()


def check_league_sample(cfg, nets, worker, sample):
    """Replay `sample` games of the league on the host: the same engines (slots, seeds, ids), one set_position per ply on the mapped slot."""
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv, Winner
    from reversi_alpha_zero_amd.worker.evaluate import _Side
    sides = [_Side(cfg, net, worker.slots, 16 * worker.seed + m, 0, "cuda:0") for m, net in enumerate(nets)]
    envs = {g: ReversiEnv().reset() for g in sample}
    plies = {g: [] for g in sample}
    live = list(sample)
    while live:
        asked = [{} for _ in sides]
        for g in live:
            s = worker.schedule[g]
            m, slot = (s.black_model, s.black_slot) if envs[g].next_player == Player.black else (s.white_model, s.white_slot)
            sides[m].ask(slot, *envs[g].get_own_and_enemy())
            asked[m][slot] = g
        for m, side in enumerate(sides):
            if not asked[m]:
                continue
            while True:
                side.engine.step(64)
                if not side.busy():
                    break
            for slot, (action, _) in side.answers().items():
                g = asked[m][slot]
                plies[g].append((m, -1 if action is None else action))
                envs[g].step(action)
        live = [g for g in live if not envs[g].done]
    for g in sample:
        s, env = worker.schedule[g], envs[g]
        got = [(p["who"], p["action"]) for p in worker.last_games[g]["plies"]]
        assert got == plies[g], f"league game {g} is not the host driver's"
        winner = s.black_model if env.winner == Winner.black else s.white_model if env.winner == Winner.white else None
        assert worker.last_results[g] == (winner, s.black_model, s.white_model, tuple(env.observation.number_of_black_and_white)), g


def run_case(name, gpp, reps, seed, calls):
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.config import Config
    case = CASES[name]
    cfg = Config()
    cfg.model.update(case["model"])
    cfg.eval.play_config.simulation_num_per_move = case["sims"]
    m = case["model"]
    nets = [ReversiNet(m["cnn_filter_num"], m["res_layer_num"], m["value_fc_size"]).keras_init_(s).randomize_bn_(s + 1) for s in range(1, MODELS + 1)]
    routes = {"league": lambda keep=False: play_league(cfg, nets, gpp, seed, calls, keep), "matches": lambda keep=False: play_matches(cfg, nets, gpp, seed, calls)}
    runs = {"league": [], "matches": []}
    for rep in range(reps + 1):                         # rep 0: untimed (kernel loading, allocator warm-up), but checked
        for route in ("league", "matches") if rep % 2 == 0 else ("matches", "league"):
            out = routes[route](keep=rep == 0)
            if rep == 0 and route == "league":
                n = len(out[4].schedule)
                check_league_sample(cfg, nets, out[4], sorted({(i * n) // 8 for i in range(8)}))
                calls.take()
            if rep:
                runs[route].append(out[:4])
    res = {"net": f'{m["cnn_filter_num"]} filters x {m["res_layer_num"]} residual layers, value_fc {m["value_fc_size"]}', "models": MODELS,
           "games_per_pair": gpp, "sims_per_move": case["sims"], "parallel_search_num": int(cfg.eval.play_config.parallel_search_num),
           "league_sample_equals_host_driver": True, "match_results_consistent": True}
    for route, rs in runs.items():
        ts = [r[0] for r in rs]
        med = statistics.median(ts)
        games, plies, c = rs[-1][1], rs[-1][2], rs[-1][3]
        res[route] = {"seconds": {"median": med, "min": min(ts), "max": max(ts), "all": ts, "reps": reps}, "games": games, "plies": plies,
                      "games_per_s": games / med, "plies_per_s": plies / med, "engine_steps": c.get("SelfPlayEngine.step", 0),
                      "launching_calls": sum(c.values()), "syncs": sum(v for k, v in c.items() if k in SYNCING), "calls": c}
    res["league_over_matches_speed"] = res["matches"]["seconds"]["median"] / res["league"]["seconds"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="mini,256x10")
    ap.add_argument("--games-per-pair", type=int, default=34)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "league_ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_league needs a GPU: there is nothing to time without one")
    calls = LeagueCalls()
    try:
        result = {"what": "a round robin of four models as one device league and as six device matches one after the other, alternating in one process",
                  "device": torch.cuda.get_device_name(0),
                  "cases": {name: run_case(name, a.games_per_pair, a.reps, a.seed, calls) for name in a.cases.split(",")}}
    finally:
        calls.remove()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
