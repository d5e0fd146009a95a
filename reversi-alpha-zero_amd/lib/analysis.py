"""Retrograde analysis of whole games on the device: every position of every game searched by a slot of ONE engine at once
(include/raz.h raz_analysis_*, engine.DeviceAnalysis).  The NBoard command the reference leaves as `pass`
(reversi_zero/play_game/nboard.py:321-330), and the annotation of files of games such as data/self_play-ggf/*.ggf."""
from logging import getLogger
from types import SimpleNamespace

import numpy as np

from ..agent.player import effective_play_config
from ..engine import (ANALYSIS_ENTRY_END, ANALYSIS_ENTRY_PASS, ANALYSIS_MAX_MOVES, EVAL_SOLVED, POS_OVER, POS_PASS_ENTRY, POS_SEARCH,
                      DeviceAnalysis, DeviceNet, SelfPlayEngine)
from .ggf import convert_to_bitboard_and_actions, parse_ggf
from .reversi_solver import EXACT_MAX_EMPTIES, WLD_MAX_EMPTIES

logger = getLogger(__name__)

# engine steps between two collects, and collects between two reads of the counters: their product is the horizon of the pool check
# (64 steps), as worker/evaluate.py's device route splits it
STEPS_PER_COLLECT = 8
COLLECTS_PER_STATS = 8


def game_from_ggf(text):
    """(black, white, player, actions) of a GGF string."""
    ggf = parse_ggf(text)
    black, white, actions = convert_to_bitboard_and_actions(ggf)
    return black, white, 1 if ggf.BO.color == "*" else 2, actions


def positions_of(pos, evals):
    """One game's per-position dictionaries from its ANALYSIS_POS / ANALYSIS_EVAL rows (engine.DeviceAnalysis.results)."""
    out = []
    for p, e in zip(pos, evals):
        state = int(p["state"])
        if state == 0:
            break
        d = {"moves_made": int(p["moves_made"]), "player": int(p["player"]), "black": int(p["black"]), "white": int(p["white"]),
             "state": {POS_SEARCH: "search", POS_PASS_ENTRY: "pass_entry", POS_OVER: "over"}[state],
             "played": None if int(p["played"]) < 0 else int(p["played"])}
        if state == POS_SEARCH:
            k = int(e["n_top"])
            d.update(eval=float(e["top_q"][0]) if k else 0.0, best_move=int(e["top_square"][0]) if k else None,
                     visits=int(e["sum_n"]), action=None if int(e["action"]) < 0 else int(e["action"]), exact=int(e["state"]) == EVAL_SOLVED,
                     top=[(int(e["top_square"][i]), int(e["top_n"][i]), float(e["top_q"][i])) for i in range(k)])
            if d["played"] is not None:
                d.update(played_eval=float(e["played_q"]), played_visits=int(e["played_n"]), played_diff=float(e["played_q"]) - d["eval"])
        elif state == POS_OVER:
            nb, nw = bin(d["black"]).count("1"), bin(d["white"]).count("1")
            d.update(discs=(nb, nw), disc_diff=(nb - nw) if d["player"] == 1 else (nw - nb))
        out.append(d)
    for i, d in enumerate(out):   # a pass entry's position is the one after it: it repeats that position's search
        if d["state"] == "pass_entry":
            nxt = next((x for x in out[i + 1:] if x["state"] != "pass_entry"), None)
            if nxt is not None:
                d.update({k: v for k, v in nxt.items() if k in ("eval", "best_move", "visits", "action", "exact", "top", "discs", "disc_diff")})
    return out




def _empties(d):
    return 64 - bin(d["black"] | d["white"]).count("1")


def annotate_exact(games, exact_empties, solver, device="cuda:0"):
    """Adds the exact solver's verdicts to analyze()'s dictionaries, in place: every position of state `search` or `pass_entry` with
    at most `exact_empties` empty squares goes through ONE solver.solve_exact_batch call.  Such a position gets solved_move and
    solved_score (the side to move's view) and, where a move was played, played_score - the exact value of that move: the next
    position's solved_score, negated when the mover changed, or the final disc difference seen from the mover - and
    played_loss = solved_score - played_score >= 0.  A pass entry whose side to move cannot move takes the position's after it."""
    import torch
    if not (isinstance(exact_empties, int) and 1 <= exact_empties <= EXACT_MAX_EMPTIES):
        raise ValueError(f"exact_empties must be 1..{EXACT_MAX_EMPTIES}, not {exact_empties!r}")
    rows = [(g, i) for g, game in enumerate(games) for i, d in enumerate(game)
            if d["state"] in ("search", "pass_entry") and _empties(d) <= exact_empties]
    if not rows:
        return games
    u = lambda xs: torch.from_numpy(np.array(xs, dtype=np.uint64).view(np.int64)).to(device)   # noqa: E731
    move, score, status = solver.solve_exact_batch(u([games[g][i]["black"] for g, i in rows]), u([games[g][i]["white"] for g, i in rows]),
                                                   torch.tensor([games[g][i]["player"] for g, i in rows], dtype=torch.uint8, device=device))
    move, score, status = (np.asarray(t.cpu()) for t in (move, score, status))
    must_pass = set()
    for k, (g, i) in enumerate(rows):
        if status[k] == 0:
            games[g][i].update(solved_move=int(move[k]), solved_score=int(score[k]))
        elif status[k] == 1:
            must_pass.add((g, i))
        else:
            raise ValueError(f"game {g}, position {i}: the exact solver answered status {int(status[k])}")

    def value(game, i, player):
        """The exact value of position i of the game, seen from `player`; None where it is not known."""
        if i >= len(game):
            return None
        d = game[i]
        v = d.get("disc_diff") if d["state"] == "over" else d.get("solved_score")
        return None if v is None else (v if d["player"] == player else -v)

    for g, game in enumerate(games):
        for i in range(len(game) - 1, -1, -1):   # backwards: a position's successor is finished first
            d = game[i]
            if (g, i) in must_pass:
                v = value(game, i + 1, d["player"])
                if v is not None:
                    d.update(solved_move=None, solved_score=v)
            if "solved_score" in d and d["played"] is not None:
                v = value(game, i + 1, d["player"])
                if v is not None:
                    d.update(played_score=v, played_loss=d["solved_score"] - v)
    return games


def annotate_wld(games, wld_empties, solver, exact_empties=None, device="cuda:0"):
    """Adds the win / draw / loss solver's verdicts to analyze()'s dictionaries, in place: every position of state `search` or
    `pass_entry` with at most `wld_empties` empty squares that `exact_empties` does not already cover goes through ONE
    solver.solve_wld_batch call, and the positions after their played moves through one more.  Such a position gets solved_outcome
    (+1 / 0 / -1, the side to move's view), outcome_move (the lowest-numbered move of that outcome) and, where a move was played,
    played_outcome - the outcome of that move: the next position's, negated when the mover changed, or the sign of the final disc
    difference seen from the mover - and outcome_kept = (played_outcome == solved_outcome).  A pass entry whose side to move cannot
    move takes the outcome of the position after it."""
    import torch
    if not (isinstance(wld_empties, int) and 1 <= wld_empties <= WLD_MAX_EMPTIES):
        raise ValueError(f"wld_empties must be 1..{WLD_MAX_EMPTIES}, not {wld_empties!r}")
    covered = exact_empties if exact_empties is not None else 0
    rows = [(g, i) for g, game in enumerate(games) for i, d in enumerate(game)
            if d["state"] in ("search", "pass_entry") and covered < _empties(d) <= wld_empties]
    if not rows:
        return games
    u = lambda xs: torch.from_numpy(np.array(xs, dtype=np.uint64).view(np.int64)).to(device)   # noqa: E731

    def batch(where):
        got = solver.solve_wld_batch(u([games[g][i]["black"] for g, i in where]), u([games[g][i]["white"] for g, i in where]),
                                     torch.tensor([games[g][i]["player"] for g, i in where], dtype=torch.uint8, device=device))
        return [np.asarray(t.cpu()) for t in got]

    sign = lambda v: (v > 0) - (v < 0)   # noqa: E731
    move, outcome, status = batch(rows)
    must_pass = set()
    for k, (g, i) in enumerate(rows):
        if status[k] == 0:
            games[g][i].update(solved_outcome=int(outcome[k]), outcome_move=int(move[k]))
        elif status[k] == 1:
            must_pass.add((g, i))
        else:
            raise ValueError(f"game {g}, position {i}: the win/draw/loss solver answered status {int(status[k])}")
    after = [(g, i + 1) for g, i in rows if games[g][i]["played"] is not None and games[g][i + 1]["state"] != "over"]
    played = {}
    if after:
        _, o2, s2 = batch(after)
        played = {where: int(o2[k]) for k, where in enumerate(after) if s2[k] == 0}

    def known(d, player):
        """The outcome of a position that is finished or annotated already, seen from `player`; None where it is not known."""
        if d["state"] == "over":
            v = d.get("disc_diff")
        else:
            v = d.get("solved_outcome", d.get("solved_score"))
        return None if v is None else (sign(v) if d["player"] == player else -sign(v))

    for g, game in enumerate(games):
        for i in range(len(game) - 1, -1, -1):   # backwards: a position's successor is finished first
            d = game[i]
            if (g, i) in must_pass and i + 1 < len(game):
                v = known(game[i + 1], d["player"])
                if v is not None:
                    d.update(solved_outcome=v, outcome_move=None)
            if "solved_outcome" in d and d["played"] is not None and i + 1 < len(game):
                nxt = game[i + 1]
                if (g, i + 1) in played:
                    v = played[(g, i + 1)] if nxt["player"] == d["player"] else -played[(g, i + 1)]
                else:   # the game is over there, or that side cannot move: what is known of it already
                    v = known(nxt, d["player"])
                if v is not None:
                    d.update(played_outcome=v, outcome_kept=bool(v == d["solved_outcome"]))
    return games


class GameAnalyzer:
    """analyze(games): per game a list of per-position dictionaries - moves_made, player (side to move), eval (the most visited
    move's value, from the side to move's view), best_move, visits, top; played_eval / played_diff for the move that was played;
    exact where the end-game solver answered.  analyze(games, exact_empties=k) adds annotate_exact's fields for the positions of
    at most k empty squares (`solver`: the object whose solve_exact_batch answers them; None = a ReversiSolver, built when first needed).
    analyze(games, wld_empties=m) adds annotate_wld's fields - who wins - for the positions of at most m empty squares that
    exact_empties does not cover (the same solver object's solve_wld_batch)."""

    def __init__(self, config, model, play_config=None, slots=1024, device="cuda:0", seed=0, solver=None):
        self.solver = solver
        self.config, self.device, self.slots, self.seed = config, device, int(slots), seed
        self.play_config = effective_play_config(config, play_config)
        m = getattr(model, "model", model)
        self.net = m if isinstance(m, DeviceNet) else DeviceNet(m.to_blob(), device)
        self.sims = int(self.play_config.simulation_num_per_move)
        shim = SimpleNamespace(play=self.play_config, play_data=config.play_data)
        loops = max(1, int(self.play_config.thinking_loop))
        # a slot searches ONE move: a node and its mirror per simulation, not the 62 plies of a game
        self.engine = SelfPlayEngine(shim, self.net, self.slots, seed=seed, nodes_per_game=(self.sims * loops + 64) * 2 + 128,
                                     sims_hint=self.sims, max_plies=64, record_root_w=True, single_stream=True, parts=1)
        self.engine.start(0, self.sims, n_active=0)
        self.analysis = DeviceAnalysis(self.engine)
        self.passes = 0

    def _busy(self):
        eng = self.engine
        st = eng.stats()   # raises on engine error flags
        if eng.pool_nearly_full(st, STEPS_PER_COLLECT * COLLECTS_PER_STATS):
            eng.gc(threshold=min(int(eng.cfg.nodes_per_game) // 4, st["max_pool_used"] // 2))

    def analyze(self, games, exact_empties=None, wld_empties=None):
        import torch
        if wld_empties is not None and not (isinstance(wld_empties, int) and 1 <= wld_empties <= WLD_MAX_EMPTIES):
            raise ValueError(f"wld_empties must be 1..{WLD_MAX_EMPTIES}, not {wld_empties!r}")
        if exact_empties is not None and not (isinstance(exact_empties, int) and 1 <= exact_empties <= EXACT_MAX_EMPTIES):
            raise ValueError(f"exact_empties must be 1..{EXACT_MAX_EMPTIES}, not {exact_empties!r}")
        games = [game_from_ggf(g) if isinstance(g, str) else tuple(g) for g in games]
        if not games:
            return []
        lists = [[ANALYSIS_ENTRY_PASS if a is None else int(a) for a in g[3]] for g in games]
        mm = max(1, max(len(x) for x in lists))
        if mm > ANALYSIS_MAX_MOVES:
            raise ValueError(f"a game of {mm} entries: at most {ANALYSIS_MAX_MOVES}")
        P = mm + 1
        per_pass = self.slots // P
        if per_pass < 1:
            raise ValueError(f"{self.slots} slots cannot hold the {P} positions of one game")
        out = []
        for lo in range(0, len(games), per_pass):
            chunk = range(lo, min(lo + per_pass, len(games)))
            moves = np.full((len(chunk), mm), ANALYSIS_ENTRY_END, dtype=np.int8)
            for i, g in enumerate(chunk):
                moves[i, :len(lists[g])] = lists[g]
            u = lambda xs: torch.from_numpy(np.array(xs, dtype=np.uint64).view(np.int64)).to(self.device)
            pos = (u([games[g][0] for g in chunk]), u([games[g][1] for g in chunk]),
                   torch.tensor([int(games[g][2]) for g in chunk], dtype=torch.uint8, device=self.device))
            an = self.analysis
            self.engine.start(lo * P, self.sims, n_active=0)   # empty trees, fresh random streams: a pass does not depend on the ones before it
            an.start(torch.from_numpy(moves).to(self.device), pos, self.sims)
            st = an.stats()   # raises on the error word
            while st["pending"]:
                for _ in range(COLLECTS_PER_STATS):
                    self.engine.step(STEPS_PER_COLLECT)
                    an.collect()
                self._busy()
                st = an.stats()
            _, p, e = an.results()
            out += [positions_of(p[i], e[i]) for i in range(len(chunk))]
            self.passes += 1
        if (exact_empties is not None or wld_empties is not None) and self.solver is None:
            from .reversi_solver import ReversiSolver
            self.solver = ReversiSolver(self.device)
        if exact_empties is not None:
            annotate_exact(out, exact_empties, self.solver, self.device)
        if wld_empties is not None:
            annotate_wld(out, wld_empties, self.solver, exact_empties, self.device)
        return out
