"""Helpers shared by the MCTS parity tests: golden-file access and config reconstruction."""
import hashlib
import json
import os
import types

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_mcts_golden(name="mcts_games.json"):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def load_par_golden():
    """Games of the unmodified reference at parallel_search_num > 1 on the exact-virtual-time event
    loop (raz-sched-v1; tests/golden/make_golden_mcts.py PAR_VARIANTS)."""
    return load_mcts_golden("mcts_par_games.json")


def load_differential_golden():
    """What the unmodified reference answered on the seeded inputs of the differential tests (make_golden_differential.py)."""
    return load_mcts_golden("reference_differential.json")


def ply_digest(root_n, root_w):
    """sha256 (16 hex digits) of a ply's root N and root W as float64 bytes, -0.0 read as 0.0 (equal under ==)."""
    import numpy as np
    n = np.asarray(root_n, dtype=np.float64) + 0.0
    w = np.asarray(root_w, dtype=np.float64) + 0.0
    return hashlib.sha256(n.tobytes() + w.tobytes()).hexdigest()[:16]


def orc_cfg_of(game):
    """OrcPlayCfg of a golden game, with the parallel_search_num the reference ran it at."""
    return O.play_cfg_from_config(config_of(game), parallel_search_num=game["resolved_play"]["parallel_search_num"])


def golden_net_blob(meta):
    """Rebuild the golden net (seeded init) and check it is byte-identical to the generator's."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = ReversiNet(meta["filters"], meta["res_layers"], meta["value_fc"]).keras_init_(meta["keras_init_seed"])
    net.randomize_bn_(meta["randomize_bn_seed"])
    blob = net.to_blob()
    assert hashlib.sha256(blob).hexdigest() == meta["blob_sha256"], "seeded net init is not reproducible"
    return blob


def config_of(game):
    """A Config-like namespace from the resolved play settings stored with a golden game."""
    play = types.SimpleNamespace(**game["resolved_play"])
    pd = types.SimpleNamespace(**game["resolved_play_data"])
    return types.SimpleNamespace(play=play, play_data=pd)


def dense(sp):
    v = [0.0] * 64
    for k, x in (sp or {}).items():
        v[int(k)] = x
    return v


def rows_of_game(plies, winner):
    """play_*.json rows exactly as SelfPlayWorker builds them (worker/self_play.py:180-185,219-231):
    black.moves + white.moves, 8 symmetric rows per searched ply (agent/player.py:166-179), z appended.
    Uses numpy for the policy symmetries like the reference; bitboard symmetries from the oracle."""
    import numpy as np
    orc = O.load()
    black_win = 1 if winner == 1 else (-1 if winner == 2 else 0)
    per_player = {1: [], 2: []}
    for p in plies:
        if not p["has_row"]:
            continue
        policy = np.array(p["saved_policy"], dtype=np.float64)
        z = black_win if p["player"] == 1 else -black_win
        for flip in (False, True):
            for rot in range(4):
                o, e, pol = p["own"], p["enemy"], policy.reshape(8, 8)
                if flip:
                    o, e, pol = orc.orc_flip_vertical(o), orc.orc_flip_vertical(e), np.flipud(pol)
                for _ in range(rot):
                    o, e = orc.orc_rotate90(o), orc.orc_rotate90(e)
                if rot:
                    pol = np.rot90(pol, k=-rot)
                per_player[p["player"]].append([[o, e], list(pol.reshape(64)), z])
    return per_player[1] + per_player[2]
