"""Time the retrograde analysis of a set of games by two routes, in one process, alternating, on the same engine seed
(README / DESIGN.md section 4.11):

  host    a ReversiEnv walk per game, one raz_engine_set_position launch per position, the engine stepped until every slot idles,
          record 0 of every slot copied to the host (headers, 64 counts, 64 f64 sums), numpy per position;
  device  lib/analysis.GameAnalyzer: raz_analysis_start replays and arms in one launch, raz_analysis_collect reduces every decided
          search where it lies, 128 bytes per position come back.

  python tools/bench_analysis.py [--reps 3] [--cases mini,256x10] [--out profiles/r16/analysis_ab.json]

Cases: "mini" - 64 games, the 16x1 net at `eval`'s 400 simulations a move; "256x10" - 16 games, the 256-filter, 10-layer net at 100
simulations a move.  The games are played by a short seeded self-play (8 simulations a move) in the same run.  The two routes'
per-position results are compared before anything is reported.  Per route: wall clock per pass over all games (median and range
over --reps passes, after one untimed pass each), positions per second, and the calls that reach the device per pass -
"launching_calls" counts every call of SelfPlayEngine.start / set_position / gc / stats / pack_records and DeviceAnalysis.start /
collect / stats / results once and SelfPlayEngine.step(n) n times, "syncs" the ones among them that wait for the device (the host
route's copy of the value sums is counted as one more).  Also: the wall clock of one NBoardEngine.go - the single-game latency - at
the initial position (whose move needs no search) and after one move, for both nets."""
import argparse
import copy
import io
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"mini": dict(model=dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16), sims=400, games=64),
         "256x10": dict(model=dict(cnn_filter_num=256, res_layer_num=10, value_fc_size=256), sims=100, games=16)}
SYNCING = ("SelfPlayEngine.stats", "DeviceAnalysis.stats", "DeviceAnalysis.results", "SelfPlayEngine.pack_records", "host.copy_root_w")


class Calls:
    """Counts the device-reaching calls of the two driver classes while it is installed."""

    def __init__(self):
        from reversi_alpha_zero_amd.engine import DeviceAnalysis, SelfPlayEngine
        self.counts, self._undo = {}, []
        for cls, names in ((SelfPlayEngine, ("start", "set_position", "set_positions", "pack_records", "gc", "stats", "step")),
                           (DeviceAnalysis, ("start", "collect", "stats", "results"))):
            for name in names:
                self._wrap(cls, name)

    def _wrap(self, cls, name):
        f, key = getattr(cls, name), f"{cls.__name__}.{name}"

        def counted(obj, *a, **kw):
            self.counts[key] = self.counts.get(key, 0) + (int(a[0] if a else kw.get("n", 1)) if name == "step" else 1)
            return f(obj, *a, **kw)
        setattr(cls, name, counted)
        self._undo.append((cls, name, f))

    def remove(self):
        for cls, name, f in self._undo:
            setattr(cls, name, f)

    def take(self):
        out, self.counts = self.counts, {}
        return out


def self_play_games(cfg, net, n, seed):
    """n move lists from a seeded self-play at 8 simulations a move (the automatic passes are the env's: no pass entries)."""
    from reversi_alpha_zero_amd.agent.player import effective_play_config
    from reversi_alpha_zero_amd.engine import SelfPlayEngine
    pc = copy.copy(effective_play_config(cfg, cfg.play))
    pc.simulation_num_per_move, pc.resign_threshold = 8, None
    e = SelfPlayEngine(SimpleNamespace(play=pc, play_data=cfg.play_data), net, n, seed=seed, sims_hint=8)
    e.start(0, 8)
    e.run()
    return [(0x0000000810000000, 0x0000001008000000, 1, [p["action"] for p in plies if p["action"] >= 0]) for plies, _ in e.records()]


class HostRoute:
    """The loop a caller writes without raz_analysis_*."""

    def __init__(self, analyzer):
        from reversi_alpha_zero_amd.engine import SelfPlayEngine
        a = analyzer
        shim = SimpleNamespace(play=a.play_config, play_data=a.config.play_data)
        self.sims, self.slots = a.sims, a.slots
        self.engine = SelfPlayEngine(shim, a.net, a.slots, seed=a.seed, nodes_per_game=int(a.engine.cfg.nodes_per_game), sims_hint=a.sims,
                                     max_plies=64, record_root_w=True, single_stream=True, parts=1)

    def analyze(self, games, calls):
        from reversi_alpha_zero_amd.engine import ANALYSIS_EVAL, ANALYSIS_POS, ANALYSIS_TOP, PLY_HEADER, lib
        from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
        from reversi_alpha_zero_amd.lib.analysis import positions_of
        eng = self.engine
        mm = max(1, max(len(g[3]) for g in games))
        P = mm + 1
        assert len(games) * P <= self.slots
        eng.start(0, self.sims, n_active=0)
        pos = np.zeros((len(games), P), dtype=ANALYSIS_POS)
        for g, (b, w, p, actions) in enumerate(games):
            env = ReversiEnv().reset().update(b, w, Player(p))
            for j in range(len(actions) + 1):
                a = actions[j] if j < len(actions) else None
                if env.done:
                    pos[g, j] = (env.board.black, env.board.white, env.next_player.value, 3, j, -2, 0)
                    break
                pos[g, j] = (env.board.black, env.board.white, env.next_player.value, 1, j, -2 if a is None else a, 0)
                own, enemy = env.get_own_and_enemy()
                eng.set_position(g * P + j, own, enemy, 1, self.sims, enable_resign=False, one_move=True)
                if a is not None:
                    env.step(a)
        while True:
            eng.step(64)
            st = eng.stats()
            if st["idle_or_done"] >= eng.n_games:
                break
            if eng.pool_nearly_full(st, 64):
                eng.gc(threshold=min(int(eng.cfg.nodes_per_game) // 4, st["max_pool_used"] // 2))
        pk = eng.pack_records(0, eng.n_games, plies=1)
        hdr = pk["headers"].cpu().numpy().view(PLY_HEADER).reshape(-1)
        root_n = pk["root_n"].cpu().numpy().reshape(-1, 64).view(np.uint32)
        off = lib.raz_engine_device_ptr(eng._h, 2) - eng._ws.data_ptr()
        root_w = eng._ws[off:off + eng.n_games * eng.max_plies * 512].view(torch.float64).view(eng.n_games, eng.max_plies, 64)[:, 0].cpu().numpy()
        calls.counts["host.copy_root_w"] = calls.counts.get("host.copy_root_w", 0) + 1
        evals = np.zeros((len(games), P), dtype=ANALYSIS_EVAL)
        for g in range(len(games)):
            for j in range(P):
                if pos[g, j]["state"] != 1:
                    continue
                s, e, played = g * P + j, evals[g, j], int(pos[g, j]["played"])
                action = int(hdr[s]["action"])
                e["action"], e["played"] = action, played
                if int(hdr[s]["flags"]) & 1:
                    n, q = np.uint32(hdr[s]["n"]), hdr[s]["q"]
                    e["state"], e["n_top"], e["sum_n"], e["top_square"][0], e["top_n"][0], e["top_q"][0] = 3, 1, n, action, n, q
                    if played == action:
                        e["played_n"], e["played_q"] = n, q
                    continue
                n = root_n[s]
                q = root_w[s] / (n.astype(np.float64) + 1e-5)
                order = [int(a) for a in np.argsort(-n.astype(np.int64), kind="stable")[:ANALYSIS_TOP] if n[a] > 0]
                e["state"], e["n_top"], e["sum_n"] = 2, len(order), n.sum(dtype=np.uint64)
                e["top_square"][:len(order)], e["top_n"][:len(order)], e["top_q"][:len(order)] = order, n[order], q[order]
                if played >= 0:
                    e["played_n"], e["played_q"] = n[played], q[played]
        return [positions_of(pos[g], evals[g]) for g in range(len(games))]


def go_latency(cfg, net):
    """Wall clock of one NBoardEngine.go (a fresh engine each): at the initial position, and after F5."""
    from reversi_alpha_zero_amd.play_game.nboard import NBoardEngine
    from reversi_alpha_zero_amd.lib.ggf import make_ggf_string
    c = copy.deepcopy(cfg)
    c.play_with_human.update_play_config(c.play)
    out = {}
    for name, moves in (("initial_position", []), ("after_F5", ["F5"])):
        ts = []
        for rep in range(3):   # the first builds the engine's kernels' state; all three are reported
            engine = NBoardEngine(c, stdin=io.StringIO(""), stdout=io.StringIO(), model=net)
            engine.handler.handle_message("set game " + make_ggf_string(moves=moves))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = engine.go()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name] = {"seconds": ts, "action": r.action, "simulation_num_per_move": int(c.play.simulation_num_per_move),
                     "parallel_search_num": int(c.play.parallel_search_num)}
    return out


def run_case(name, reps, seed, calls):
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.engine import DeviceNet
    from reversi_alpha_zero_amd.lib import analysis
    case = CASES[name]
    cfg = Config()
    cfg.model.update(case["model"])
    cfg.eval.play_config.simulation_num_per_move = case["sims"]
    m = case["model"]
    net = ReversiNet(m["cnn_filter_num"], m["res_layer_num"], m["value_fc_size"]).keras_init_(1).randomize_bn_(2)
    dnet = DeviceNet(net.to_blob(), "cuda:0")
    games = self_play_games(cfg, dnet, case["games"], seed)
    P = max(len(g[3]) for g in games) + 1
    device = analysis.GameAnalyzer(cfg, dnet, cfg.eval.play_config, slots=len(games) * P, device="cuda:0", seed=seed)
    host = HostRoute(device)
    routes = {"host": lambda: host.analyze(games, calls), "device": lambda: device.analyze(games)}
    times, counted, first = {"host": [], "device": []}, {}, None
    for rep in range(reps + 1):                         # rep 0: untimed (kernel loading, allocator warm-up), but compared
        for route in ("host", "device") if rep % 2 == 0 else ("device", "host"):
            calls.take()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = routes[route]()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if first is None:
                first = got
            assert got == first, f"{name}: the {route} route's analysis (rep {rep}) is not the first one made"
            counted[route] = calls.take()
            if rep:
                times[route].append(t)
    positions = sum(len(g) for g in first)
    searched = sum(1 for g in first for d in g if d["state"] == "search")
    out = {"net": f'{m["cnn_filter_num"]} filters x {m["res_layer_num"]} residual layers, value_fc {m["value_fc_size"]}', "games": len(games),
           "sims_per_move": case["sims"], "parallel_search_num": int(cfg.eval.play_config.parallel_search_num), "positions": positions,
           "searched": searched, "solved": sum(1 for g in first for d in g if d.get("exact")), "slots": len(games) * P,
           "results_identical": True}
    for route in ("host", "device"):
        ts, c = times[route], counted[route]
        out[route] = {"seconds_per_pass": {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": ts, "reps": reps},
                      "positions_per_s": positions / statistics.median(ts), "launching_calls": sum(c.values()),
                      "syncs": sum(v for k, v in c.items() if k in SYNCING), "calls": c}
    out["device_over_host_speed"] = out["host"]["seconds_per_pass"]["median"] / out["device"]["seconds_per_pass"]["median"]
    out["steps_per_collect"], out["collects_per_stats"] = analysis.STEPS_PER_COLLECT, analysis.COLLECTS_PER_STATS
    del device, host
    out["nboard_go"] = go_latency(cfg, net)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="mini,256x10")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "analysis_ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analysis needs a GPU: there is nothing to time without one")
    calls = Calls()
    try:
        result = {"what": "the retrograde analysis of a set of self-played games by the host and the device route, alternating in one process",
                  "device": torch.cuda.get_device_name(0),
                  "cases": {name: run_case(name, a.reps, a.seed, calls) for name in a.cases.split(",")}}
    finally:
        calls.remove()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
