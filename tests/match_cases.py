"""Shared cases of the device hand-off between two engines (include/raz.h raz_match_*, csrc/raz_match.h), run by
tests/test_match_emu.py on the wave emulator and by tests/test_match_gpu.py on the device.

Both drive the PRODUCT's wrappers (engine.SelfPlayEngine, engine.DeviceMatch); a BACKEND - an Adapter below, one instance for the
emulator's host memory and one for the device - gives the cases engines and matches of its kind:
    backend.engine(cfg, blob, n, seed, sims, **kw)   a started engine with every slot idle (as worker/evaluate.py's _Side makes it)
    backend.answers(engine)                          (actions i8 [n], root visit counts [n, 64]) of every slot's record 0
    backend.match(best_engine, challenger_engine)    a MatchHarness: start(best_is_black, positions, sims_best, sims_challenger,
                                                     enable_resign), turn(), stats() -> dict with "error", read() -> (games, plies,
                                                     root_n), workspace(), check_guard()
`cfg` is the namespace an engine is configured from: play = the effective eval play config, play_data.

The EXPECTATION of every case is drive_host: ReversiEnv objects and one set_position call per ply, the loop of
tests/test_engine_emu.py's golden evaluation test (and of worker/evaluate.py's host route), which looks at no match kernel."""
import hashlib
import json
import os
import types
from random import Random

import numpy as np

from conftest import ROOT

GUARD = 4096


# ---- the backend of the cases: the product's wrappers on one device ---------------------------------------------------------------
class Guarded:
    """The workspace of a product wrapper `w` (set by the subclass) inside a tensor of the backend's device, `guard` bytes of 0x55 on
    both sides of it."""

    def __init__(self, backend, need, guard):
        import torch
        self.backend, self.need = backend, need
        self.mem = torch.full((guard + need + 256 + guard,), 0x55, dtype=torch.uint8, device=backend.device)
        self.given = self.mem[guard:guard + need + 256]   # what the wrapper is handed as workspace=

    def _sync(self):
        self.w.backend.synchronize(self.w.device)
        return self.w.workspace_base - self.mem.data_ptr()

    def workspace(self):
        off = self._sync()
        return self.mem[off:off + self.need].clone().cpu().numpy()

    def check_guard(self):
        off = self._sync()
        assert bool((self.mem[off + self.need:] == 0x55).all()) and bool((self.mem[:off] == 0x55).all()), \
            f"{type(self.w).__name__} wrote outside its workspace"

    def stats(self):
        return self.w.stats(raise_on_error=False)


class MatchHarness(Guarded):
    """engine.DeviceMatch behind the interface of the cases, in a guarded workspace."""

    def __init__(self, backend, best, challenger, guard=GUARD):
        from reversi_alpha_zero_amd.engine import DeviceMatch
        super().__init__(backend, best.lib.raz_match_workspace_bytes(best.n_games), guard)
        self.w = DeviceMatch(best, challenger, workspace=self.given)

    def start(self, best_is_black, positions, sims_best, sims_challenger, enable_resign=True):
        bib = self.backend.tensor(np.array([int(b) for b in best_is_black], dtype=np.uint8))
        self.w.start(bib, self.backend.positions(positions), sims_best, sims_challenger, enable_resign)

    def turn(self):
        self.w.turn()

    def read(self):
        return self.w.read()


class Adapter:
    """A backend of the match, league and analysis cases: `device`, and make_engine(cfg, blob, n, **kw) -> a created SelfPlayEngine
    there (one stream, one part, record_root_w)."""

    def __init__(self, device, make_engine):
        self.device, self.make_engine = device, make_engine

    def engine(self, cfg, blob, n, seed, sims, first_game_id=0, **kw):
        e = self.make_engine(cfg, blob, n, seed=seed, sims_hint=sims, max_plies=64, **kw)
        e.start(first_game_id, sims, n_active=0)
        return e

    def tensor(self, a):
        """A host array in the backend's memory (u64 bit patterns travel as int64)."""
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device)

    def positions(self, positions):
        """[(black, white, player)] or None -> what the wrappers' start takes as positions=."""
        if positions is None:
            return None
        return (self.tensor(np.array([p[0] for p in positions], dtype=np.uint64)), self.tensor(np.array([p[1] for p in positions], dtype=np.uint64)),
                self.tensor(np.array([p[2] for p in positions], dtype=np.uint8)))

    @staticmethod
    def answers(e):
        from reversi_alpha_zero_amd.engine import PLY_HEADER
        pk = e.pack_records(0, e.n_games, plies=1)
        return pk["headers"].cpu().numpy().view(PLY_HEADER).reshape(-1)["action"], pk["root_n"].cpu().numpy().reshape(e.n_games, 64)

    @staticmethod
    def raw(e):
        """Record 0 of every slot: action, flags, q, n [slots] and root_n, root_w [slots, 64]."""
        r = e.read_raw()
        h = r["headers"][:, 0]
        return dict(action=h["action"], flags=h["flags"], q=h["q"], n=h["n"], root_n=r["root_n"][:, 0], root_w=r["root_w"][:, 0])

    @staticmethod
    def blocks(e):
        """The control blocks of every slot, uint8 [n_games, 256] (raz_engine_debug_read, which = 3)."""
        out = np.zeros((e.n_games, 256), dtype=np.uint8)
        e.backend.call("raz_engine_debug_read", e._h, 3, 0, out.size, out.ctypes.data)
        return out

    controls = blocks

    def match(self, best, challenger, guard=GUARD):
        return MatchHarness(self, best, challenger, guard=guard)

    def league(self, engines, n_games, guard=GUARD):
        from league_cases import LeagueHarness
        return LeagueHarness(self, engines, n_games, guard=guard)

    def analysis(self, engine, n_games, max_moves, first_slot=0, guard=GUARD):
        from analysis_cases import AnalysisHarness
        return AnalysisHarness(self, engine, n_games, max_moves, first_slot=first_slot, guard=guard)


# ---- nets and configurations ------------------------------------------------------------------------------------------------
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "eval_games.json")) as f:
        return json.load(f)


def golden_blobs(gold):
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    blobs = []
    for meta in gold["nets"]:
        b = ReversiNet(meta["filters"], meta["res_layers"], meta["value_fc"]).keras_init_(meta["keras_init_seed"]).randomize_bn_(meta["randomize_bn_seed"]).to_blob()
        assert hashlib.sha256(b).hexdigest() == meta["blob_sha256"]
        blobs.append(b)
    return blobs


def golden_cfg(m):
    from reversi_alpha_zero_amd.agent.player import effective_play_config
    whole = types.SimpleNamespace(play=types.SimpleNamespace(**m["resolved_config_play"]))
    pc = effective_play_config(whole, types.SimpleNamespace(**m["resolved_play_config"]))
    return types.SimpleNamespace(play=pc, play_data=types.SimpleNamespace(save_policy_of_tau_1=True))


def mini_blobs():
    """Two mini nets (16 filters, 1 residual layer, value_fc 16): the best model and a challenger."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return [ReversiNet(16, 1, 16).keras_init_(s).randomize_bn_(s + 1).to_blob() for s in (1, 2)]


def mini_config(parallel_search_num=1, sims=8, **play):
    """The package's Config with the mini net, `sims` simulations a move and parallel_search_num in both play sections."""
    from reversi_alpha_zero_amd.config import Config
    cfg = Config()
    cfg.model.update(dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16))
    cfg.eval.play_config.simulation_num_per_move = sims
    for section in (cfg.play, cfg.eval.play_config):
        section.parallel_search_num = parallel_search_num
        for k, v in play.items():
            setattr(section, k, v)
    return cfg


def engine_cfg(config):
    """What worker/evaluate.py's _Side configures its engine from."""
    from reversi_alpha_zero_amd.agent.player import effective_play_config
    return types.SimpleNamespace(play=effective_play_config(config, config.eval.play_config), play_data=config.play_data)


# ---- start positions ----------------------------------------------------------------------------------------------------------
def _legal(env):
    from reversi_alpha_zero_amd.lib.bitboard import find_correct_moves
    own, enemy = env.get_own_and_enemy()
    m = find_correct_moves(own, enemy)
    return [a for a in range(64) if (m >> a) & 1]


def _pos(env):
    return (env.board.black, env.board.white, env.next_player.value)


def playout_positions(seed, n, discs):
    """n playable positions with `discs` discs on the board, each from a random legal playout of its own."""
    from reversi_alpha_zero_amd.env.reversi_env import ReversiEnv
    rnd, out = Random(seed), []
    while len(out) < n:
        env = ReversiEnv().reset()
        while not env.done and sum(env.board.number_of_black_and_white) < discs:
            env.step(rnd.choice(_legal(env)))
        if not env.done:
            out.append(_pos(env))
    return out


def special_positions(seed=7):
    """Positions with ONE legal move each, so that what follows does not depend on a search: "pass" - the move leaves the opponent
    without a move and the mover with one; "one_empty" - a single empty square, the game ends on the hand-off; "dead_end" - after
    the move neither side can move although squares are empty; and "white" - any position with white to move."""
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
    rnd, found = Random(seed), {}
    while len(found) < 4:
        env = ReversiEnv().reset()
        while not env.done:
            moves = _legal(env)
            if env.next_player == Player.white and sum(env.board.number_of_black_and_white) == 9:
                found.setdefault("white", _pos(env))
            if len(moves) == 1:
                b, w, p = _pos(env)
                nxt = ReversiEnv().update(b, w, Player(p))
                nxt.step(moves[0])
                discs = sum(nxt.board.number_of_black_and_white)
                if not nxt.done and nxt.next_player.value == p:
                    found.setdefault("pass", (b, w, p))
                elif nxt.done and discs == 64:
                    found.setdefault("one_empty", (b, w, p))
                elif nxt.done and discs < 64:
                    found.setdefault("dead_end", (b, w, p))
            env.step(rnd.choice(moves))
    return found


# ---- the two drivers ------------------------------------------------------------------------------------------------------------
def _engines(backend, cfg, blobs, n, seed, first, sims, **kw):
    return {True: backend.engine(cfg, blobs[0], n, 2 * seed, sims, first_game_id=first, **kw),
            False: backend.engine(cfg, blobs[1], n, 2 * seed + 1, sims, first_game_id=first, **kw)}


def _outcome(env, best_is_black):
    from reversi_alpha_zero_amd.env.reversi_env import Winner
    ng_win = None if env.winner not in (Winner.black, Winner.white) else int((env.winner == Winner.black) != best_is_black)
    return ng_win, bool(best_is_black), tuple(env.observation.number_of_black_and_white)


def drive_host(backend, cfg, blobs, n, seed, first, sims, best_is_black, positions=None, enable_resign=True, step=16):
    """The independent driver: (per game [(who, action, root_n list)], per game (ng_win, best_is_black, (blacks, whites)))."""
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
    sides = _engines(backend, cfg, blobs, n, seed, first, sims)
    envs = [ReversiEnv().reset() if positions is None else ReversiEnv().update(positions[g][0], positions[g][1], Player(positions[g][2]))
            for g in range(n)]
    plies, live = [[] for _ in range(n)], list(range(n))
    while live:
        armed = {True: [], False: []}
        for g in live:
            own, enemy = envs[g].get_own_and_enemy()
            mover_is_best = (envs[g].next_player == Player.black) == bool(best_is_black[g])
            sides[mover_is_best].set_position(g, own, enemy, 1, sims, enable_resign=enable_resign, one_move=True)
            armed[mover_is_best].append(g)
        for is_best, e in sides.items():
            if not armed[is_best]:
                continue
            while e.stats()["idle_or_done"] < n:
                e.step(step)
            actions, root_n = backend.answers(e)
            for g in armed[is_best]:
                a = int(actions[g])
                plies[g].append(("best" if is_best else "ng", a, [int(x) for x in root_n[g]]))
                envs[g].step(a if a >= 0 else None)
        live = [g for g in live if not envs[g].done]
    return plies, [_outcome(envs[g], best_is_black[g]) for g in range(n)]


def drive_match(backend, cfg, blobs, n, seed, first, sims, best_is_black, positions=None, enable_resign=True, step=4, turn_every=1,
                max_iterations=100000, guard=None, after_start=None, error=0):
    """The same match through raz_match_*: step both engines `turn_every` times by `step`, hand off, read the counters.
    after_start(sides, match): called once, behind the start; error: the error word the match is to end with."""
    from reversi_alpha_zero_amd.engine import match_games, match_results
    sides = _engines(backend, cfg, blobs, n, seed, first, sims)
    match = backend.match(sides[True], sides[False], **({"guard": guard} if guard is not None else {}))
    match.start(best_is_black, positions, sims, sims, enable_resign)
    st = match.stats()
    assert st["live"] == n and st["searching_best"] + st["searching_challenger"] == n and st["plies"] == 0 and not st["error"]
    if after_start is not None:
        after_start(sides, match)
    it = 0
    while st["live"]:
        for _ in range(turn_every):
            for e in sides.values():
                e.step(step)
        match.turn()
        for e in sides.values():
            e.stats()   # raises on engine error flags
        st = match.stats()
        assert st["error"] in (0, error), st
        it += 1
        assert it < max_iterations, "the match does not end"
    assert st["error"] == error and st["searching_best"] == st["searching_challenger"] == 0, st
    games, log, root_n = match.read()
    assert st["plies"] == int(games["n_plies"].sum())
    got = match_games(games, log, root_n, first_game_id=first)
    plies = [[(p["who"], p["action"], [int(x) for x in p["root_n"]]) for p in g["plies"]] for g in got]
    assert [g["game_id"] for g in got] == list(range(first, first + n))
    if guard is not None:
        match.check_guard()
    return plies, match_results(games)


def assert_same(tag, got, want):
    (gp, gr), (wp, wr) = got, want
    assert len(gp) == len(wp)
    for g, (a, b) in enumerate(zip(gp, wp)):
        assert [(w, x) for w, x, _ in a] == [(w, x) for w, x, _ in b], (tag, g)
        for i, (p, q) in enumerate(zip(a, b)):
            assert p[2] == q[2], (tag, g, i, "root_n")
    assert gr == wr, (tag, gr, wr)


# ---- case 1: the reference's golden evaluation games ----------------------------------------------------------------------------
def check_against_golden(m, plies, results):
    for g, ref in enumerate(m["games"]):
        where = (m["name"], ref["game_id"])
        assert [(w, a) for w, a, _ in plies[g]] == [(p["who"], p["action"]) for p in ref["plies"]], where
        for i, ((_, _, rn), p) in enumerate(zip(plies[g], ref["plies"])):
            if p["root_n"] is not None:      # (a move the end-game solver decided has no search behind it)
                want = [0] * 64
                for k, v in p["root_n"].items():
                    want[int(k)] = int(v)
                assert rn == want, (where, i)
        assert results[g][0] == ref["ng_win"] and results[g][1] == ref["best_is_black"] and list(results[g][2]) == ref["black_white"], where


def case_golden(backend, m, blobs):
    cfg = golden_cfg(m)
    n, sims = len(m["games"]), int(cfg.play.simulation_num_per_move)
    plies, results = drive_match(backend, cfg, blobs, n, m["seed"], m["first_game_id"], sims, [g["best_is_black"] for g in m["games"]], step=8)
    check_against_golden(m, plies, results)


# ---- case 3: start positions ----------------------------------------------------------------------------------------------------
def case_start_positions(backend, blobs, parallel_search_num=1):
    sp = special_positions()
    names = ["pass", "white", "one_empty", "dead_end", "pass", "one_empty"]
    positions = [sp[k] for k in names]
    bib = [True, False, True, False, False, False]
    cfg = engine_cfg(mini_config(parallel_search_num))
    want = drive_host(backend, cfg, blobs, len(names), 5, 40, 8, bib, positions)
    again = drive_host(backend, cfg, blobs, len(names), 5, 40, 8, bib, positions, step=3)
    assert_same("host driver agrees with itself", again, want)
    wp, wr = want
    for g in (0, 4):   # the pass: the mover of ply 0 moves again
        assert len(wp[g]) >= 2 and wp[g][0][0] == wp[g][1][0], ("no pass", g, wp[g][:2])
    assert positions[1][2] == 2 and wp[1][0][0] == ("ng" if bib[1] else "best")            # white to move, and white is not black's model
    for g in (2, 5):   # one empty square: one ply, a full board
        assert len(wp[g]) == 1 and wp[g][0][1] >= 0 and sum(wr[g][2]) == 64, ("not a last square", g)
    assert len(wp[3]) == 1 and wp[3][0][1] >= 0 and sum(wr[3][2]) < 64, "no early end"    # neither side can move, squares empty
    assert_same("start positions", drive_match(backend, cfg, blobs, len(names), 5, 40, 8, bib, positions), want)
    # a resign threshold no search value reaches: the mover of every game resigns at once (turn >= allowed_resign_turn 0)
    rcfg = engine_cfg(mini_config(parallel_search_num, resign_threshold=2.0, allowed_resign_turn=0))
    rpos = [sp["white"]] + playout_positions(3, 2, 30)   # (before use_solver_turn: the search decides, and resigns)
    want = drive_host(backend, rcfg, blobs, 3, 6, 50, 8, [True, False, True], rpos)
    assert all(len(p) == 1 and p[0][1] == -1 for p in want[0]), ("no resignation", want[0])
    assert [r[0] for r in want[1]] == [int((pos[2] == 1) == b) for pos, b in zip(rpos, [True, False, True])]   # the resigner's opponent wins
    assert_same("resignation", drive_match(backend, rcfg, blobs, 3, 6, 50, 8, [True, False, True], rpos), want)
    off = drive_match(backend, rcfg, blobs, 3, 6, 50, 8, [True, False, True], rpos, enable_resign=False)
    assert all(p[0][1] >= 0 for p in off[0]), "enable_resign = 0 must reach the slots"


# ---- case 7: a searching slot that leaves the one-move protocol -------------------------------------------------------------------
def rearm_outside_one_move(engine, slot, black, white, player, sims):
    """Arm `slot` again for the side to move of (black, white, player) as a hand-off arms it, but NOT for one move: the slot plays its
    game on alone and ends in phase done - what csrc/raz_handoff.h's slot_answer calls ERR_SLOT."""
    own, enemy = (int(black), int(white)) if int(player) == 1 else (int(white), int(black))
    engine.set_position(slot, own, enemy, 1, sims, enable_resign=True, one_move=False)


def case_slot_off_protocol(backend, blobs, parallel_search_num=1):
    """Game 1's searching slot is re-armed outside one-move mode behind the start: the game ends undecided with error word 0x100 exactly,
    no engine reports an error flag, the searching counters end at 0, and games 0 and 2 are the games of the undisturbed match."""
    cfg = engine_cfg(mini_config(parallel_search_num, use_solver_turn=0, use_solver_turn_in_simulation=0))
    args = (backend, cfg, blobs, 3, 7, 60, 8, [True, False, True], playout_positions(11, 3, 50))
    clean = drive_match(*args)
    kept = {}

    def rearm(sides, match):
        g = match.read()[0][1]
        assert g["searching"] in (1, 2) and g["n_plies"] == 0
        rearm_outside_one_move(sides[g["searching"] == 1], 1, g["black"], g["white"], g["player"], 8)
        kept["match"] = match
    got = drive_match(*args, after_start=rearm, error=0x100)   # (asserts the final error word, the counters, and e.stats() of both engines every turn)
    games = kept["match"].read()[0]
    assert (int(games[1]["searching"]), int(games[1]["winner"]), int(games[1]["n_plies"])) == (0, 0, 0), games[1]
    assert got[0][1] == [] and got[1][1][0] is None
    for g in (0, 2):
        assert len(clean[0][g]) > 0 and games[g]["winner"] != 0
        assert_same(("beside a slot off the protocol", g), ([got[0][g]], [got[1][g]]), ([clean[0][g]], [clean[1][g]]))
