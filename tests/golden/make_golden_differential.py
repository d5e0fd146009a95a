#!/usr/bin/env python
"""Generate tests/golden/reference_differential.json: what the UNMODIFIED reference answers on the seeded inputs of the
differential tests (tests/test_oracle_bitboard.py, test_oracle_solver.py, test_oracle_mcts.py, test_worker_host.py), so that those tests compare the
oracle with the reference without importing it.  Run where the reference is installed:
    python tests/golden/make_golden_differential.py
Contents: the parsed config/{mini,ch5,alpha_go_zero}.yml and the play / play_data / model values the reference's Config takes from
them; find_correct_moves / calc_flip on 3000 random(7) inputs; the compiled Cython solver's answers in both modes on 40
late-game positions reached by random(777) playouts of the reference env; and whole self-play games of the reference worker
(fixed seeds, game ids and play overrides) - per ply the action, the player and a digest of root N and W (float64 bytes).
Every number is produced by reference code."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)
import ref_harness as rh  # noqa: E402
from oracle_util import ply_digest  # noqa: E402

PLAY_KEYS = ["thinking_loop", "required_visit_to_decide_action", "start_rethinking_turn", "c_puct", "noise_eps", "dirichlet_alpha",
             "change_tau_turn", "virtual_loss", "parallel_search_num", "resign_threshold", "allowed_resign_turn",
             "disable_resignation_rate", "use_solver_turn", "use_solver_turn_in_simulation", "share_mtcs_info_in_self_play",
             "reset_mtcs_info_per_game"]


# (name, yml, play overrides, seed, game id, sims per move, parallel_search_num, virtual-time event loop)
GAMES = [
    ("live_agz", "alpha_go_zero.yml", {"parallel_search_num": 1, "c_puct": 1.5, "noise_eps": 0.4, "dirichlet_alpha": 1.0, "change_tau_turn": 6},
     99, 123456, 15, 1, False),
    ("dirichlet_alpha_2", "alpha_go_zero.yml", {"parallel_search_num": 1, "noise_eps": 0.5, "dirichlet_alpha": 2.0}, 31, 77, 12, 1, False),
    ("par5_mini", "mini.yml", {"parallel_search_num": 5, "reset_mtcs_info_per_game": 1, "use_solver_turn": 0, "use_solver_turn_in_simulation": 0},
     77, 4242, 18, 5, True),
    ("par7_agz", "alpha_go_zero.yml", {"parallel_search_num": 7, "reset_mtcs_info_per_game": 1, "use_solver_turn": 0,
                                       "use_solver_turn_in_simulation": 0}, 78, 4242, 18, 7, True),
]
FROM_POSITION = ("ch5.yml", {"parallel_search_num": 1, "thinking_loop": 1, "use_solver_turn": 0, "use_solver_turn_in_simulation": 0}, 5, 900, 14)


def from_position_starts():
    """The mid-game positions test_game_taken_up_at_a_position_matches_the_reference plays from (oracle env, rng 3)."""
    import ctypes
    import oracle as O
    env, lib = O.OrcEnv(), O.load()
    rng = np.random.default_rng(3)
    starts = []
    for plies_in in (7, 30, 52):
        lib.orc_env_reset(ctypes.byref(env))
        for _ in range(plies_in):
            own, enemy = (env.black, env.white) if env.next_player == 1 else (env.white, env.black)
            legal = lib.orc_find_correct_moves(own, enemy)
            lib.orc_env_step(ctypes.byref(env), int(rng.choice([i for i in range(64) if legal >> i & 1])))
            assert not env.done
        starts.append((int(env.black), int(env.white), int(env.next_player)))
    return starts


def game_record(name, cfg, ref, seed, gid, sims, par, start=None):
    return {"name": name, "seed": seed, "game_id": gid, "sims": sims, "parallel_search_num": par,
            "start": None if start is None else ["0x%016x" % start[0], "0x%016x" % start[1], start[2]],
            "resolved_play": {k: getattr(cfg.play, k) for k in PLAY_KEYS},
            "resolved_play_data": {"save_policy_of_tau_1": cfg.play_data.save_policy_of_tau_1,
                                   "drop_draw_game_rate": cfg.play_data.drop_draw_game_rate},
            "actions": [p["action"] for p in ref["plies"]], "players": [p["player"] for p in ref["plies"]],
            "root_digests": [ply_digest(p["root_n"], p["root_w"]) for p in ref["plies"]],
            "winner": ref["winner"], "nn_positions": ref["nn_positions"]}


def main():
    rh.install()
    out = {"generator": "tests/golden/make_golden_differential.py"}

    from reversi_zero.lib import bitboard as rb
    rng = random.Random(7)
    fcm, flip = [], []
    for _ in range(3000):
        own, enemy, pos = rng.getrandbits(64), rng.getrandbits(64), rng.randrange(64)
        if rng.random() < 0.7:
            enemy &= ~own
        fcm.append("%x" % rb.find_correct_moves(own, enemy))
        flip.append("%x" % rb.calc_flip(pos, own, enemy))
    out["bitboard_random7"] = {"find_correct_moves": fcm, "calc_flip": flip}

    import pyximport
    import tempfile
    pyximport.install(build_dir=tempfile.mkdtemp(prefix="pyxbld_"), language_level=3)
    from reversi_zero.lib.alt.reversi_solver_cython import ReversiSolver
    from reversi_zero.env.reversi_env import ReversiEnv, Player
    from reversi_zero.lib.bitboard import find_correct_moves, bit_count
    rng = random.Random(777)
    positions = []
    while len(positions) < 40:
        env = ReversiEnv().reset()
        stop_at = 64 - rng.randint(2, 9)
        while not env.done and bit_count(env.board.black) + bit_count(env.board.white) < stop_at:
            own, enemy = env.get_own_and_enemy()
            legal = find_correct_moves(own, enemy)
            env.step(rng.choice([i for i in range(64) if legal >> i & 1]))
        if env.done:
            continue
        b, w, pl = env.board.black, env.board.white, env.next_player.value
        ans = {}
        for exactly in (True, False):
            m, s = ReversiSolver().solve(b, w, Player(pl), timeout=300, exactly=exactly)
            ans["exact" if exactly else "non_exact"] = [m, s]
        positions.append(dict(black="0x%016x" % b, white="0x%016x" % w, next_player=pl, **ans))
    out["solver_random777"] = positions

    import yaml
    out["config_overlay"] = {}
    for yml in ("mini.yml", "ch5.yml", "alpha_go_zero.yml"):
        with open(os.path.join(rh.REFERENCE_ROOT, "config", yml), "rt") as f:
            parsed = yaml.safe_load(f)
        ref = rh.load_config(yml)
        out["config_overlay"][yml] = {"yml": parsed, "resolved": {sec: vars(getattr(ref, sec)) for sec in ("play", "play_data", "model")}}

    import ref_selfplay as rs
    from oracle_util import load_mcts_golden, golden_net_blob
    blob = golden_net_blob(load_mcts_golden()["net"])
    out["games"] = []
    for name, yml, over, seed, gid, sims, par, vt in GAMES:
        cfg = rh.load_config(yml, {"play": over})
        ref = rs.run_reference_game(cfg, blob, seed=seed, game_id=gid, sims_per_move=sims, virtual_time=vt)
        out["games"].append(game_record(name, cfg, ref, seed, gid, sims, par))
        print(name, "plies", len(ref["plies"]), "winner", ref["winner"])
    yml, over, seed, gid0, sims = FROM_POSITION
    cfg = rh.load_config(yml, {"play": over})
    for k, st in enumerate(from_position_starts()):
        ref = rs.run_reference_game(cfg, blob, seed=seed, game_id=gid0 + k, sims_per_move=sims, start=st)
        out["games"].append(game_record(f"from_position_{k}", cfg, ref, seed, gid0 + k, sims, 1, start=st))
        print("from position", k, "plies", len(ref["plies"]), "winner", ref["winner"])

    path = os.path.join(HERE, "reference_differential.json")
    with open(path, "wt") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
