"""The `league` worker: a round robin of up to 16 models on the device, and their ratings (no reference counterpart: the reference's
`eval` worker knows two models and keeps neither, worker/evaluate.py:31-42).

Every model gets one engine, configured as worker/evaluate.py's _Side configures it, and engine.DeviceLeague plays all games of a pass
at once with the hand-off on the device.  The schedule is lib/rating.round_robin's: model m's game of round r against the opponent of
rank q among the other models is served by slot k = r (M-1) + q of m's engine and carries the game id k in that engine, so a game is
the same game whether the schedule is played in one pass or, with fewer slots per engine, in several passes of whole rounds - every
pass restarts the engines on the first k of the pass.  Model m is seeded 16 x seed + m.
Not built: games refilled into freed slots inside one pass, a league over several ranks, Swiss or gauntlet pairings."""
import json
import os
from logging import getLogger

import numpy as np

from ..lib.rating import bradley_terry, round_robin, tally
from .evaluate import _Side, play_on_device

logger = getLogger(__name__)


def start(config, model_dirs=None, names=None, games_per_pair=2, seed=0, device="cuda:0", slots=None, out_path=None, keep_games=False):
    """Rate the models in model_dirs (directories holding the next-generation file names), or - model_dirs None - the generations
    self_opt.start(archive_generations=True) archived, in name order, with the current best model appended where its blob differs from
    the last archived one.  Returns LeagueWorker.play's dictionary."""
    models, found = load_models(config, model_dirs)
    worker = LeagueWorker(config, models, names=names or found, games_per_pair=games_per_pair, seed=seed, device=device, slots=slots)
    return worker.play(out_path=out_path, keep_games=keep_games)


def load_models(config, model_dirs=None):
    """(models, names)."""
    from ..agent.model import ReversiModel
    from ..lib.model_helpler import load_best_model_weight
    from .self_opt import archived_generation_dirs
    rc = config.resource
    archive = model_dirs is None
    models, names = [], []
    for d in (archived_generation_dirs(config) if archive else model_dirs):
        m = ReversiModel(config)
        if not m.load(os.path.join(d, rc.next_generation_model_config_filename), os.path.join(d, rc.next_generation_model_weight_filename)):
            raise RuntimeError(f"no model in {d}")
        models.append(m)
        names.append(os.path.basename(os.path.normpath(d)))
    if archive:
        best = ReversiModel(config)
        if load_best_model_weight(best) and (not models or best.model.to_blob() != models[-1].model.to_blob()):
            models.append(best)
            names.append("best")
    return models, names


class LeagueWorker:
    def __init__(self, config, models, names=None, games_per_pair=2, seed=0, device="cuda:0", slots=None):
        """models: 2..16 ReversiModel (or ReversiNet) objects.  slots: slots per engine, a multiple of len(models) - 1 (None:
        everything at once, (len(models) - 1) x games_per_pair)."""
        from ..engine import LEAGUE_MAX_MODELS
        self.config, self.models, self.seed, self.device = config, list(models), int(seed), device
        M = len(self.models)
        if not 2 <= M <= LEAGUE_MAX_MODELS:
            raise ValueError(f"a league has 2..{LEAGUE_MAX_MODELS} models, not {M}")
        self.names = list(names) if names is not None else [f"model_{m}" for m in range(M)]
        if len(self.names) != M:
            raise ValueError("names: one per model")
        self.games_per_pair = int(games_per_pair)
        self.schedule, self.slot_map = round_robin(M, self.games_per_pair)
        self.slots = (M - 1) * self.games_per_pair if slots is None else int(slots)
        if self.slots < M - 1 or self.slots % (M - 1):
            raise ValueError(f"slots: whole rounds of {M - 1} games per engine")
        self.last_games = None

    def play_pass(self, first_round, rounds):
        """Rounds first_round .. first_round + rounds - 1, all at once.  Returns (LEAGUE_GAME records, per-game dictionaries) of the
        pass's games in schedule order."""
        import torch
        from ..engine import DeviceLeague, league_games, league_pairings
        M = len(self.models)
        first_k, n_slots = first_round * (M - 1), rounds * (M - 1)
        sides = [_Side(self.config, model, n_slots, 16 * self.seed + m, first_k, self.device) for m, model in enumerate(self.models)]
        games = [g for g in self.schedule if first_round <= g.round < first_round + rounds]
        pairings = league_pairings([(g.black_model, g.black_slot - first_k, g.white_model, g.white_slot - first_k) for g in games])
        league = DeviceLeague([s.engine for s in sides])
        league.start(torch.from_numpy(pairings.view(np.uint8).reshape(len(games), -1)).to(self.device), sims=[s.sims for s in sides],
                     enable_resign=True)
        records, _, plies, root_n = play_on_device(league, sides)
        return records, league_games(records, plies, root_n)

    def play(self, out_path=None, keep_games=False):
        """Play the whole schedule in passes of self.slots / (M - 1) rounds and rate the models.  Returns - and, with out_path, writes
        as JSON with sorted keys and fixed float formatting - names, the wins / draws / losses matrices, per-model score and Elo
        (model 0 the anchor at 0), per-pair score, and per-game results (with the move lists where keep_games)."""
        from ..engine import league_results
        M = len(self.models)
        per_pass = self.slots // (M - 1)
        results, games = [], []
        for first_round in range(0, self.games_per_pair, per_pass):
            records, played = self.play_pass(first_round, min(per_pass, self.games_per_pair - first_round))
            results += league_results(records)
            games += played
        self.last_results, self.last_games = results, games
        wins, draws, losses = tally(results, M)
        elo = bradley_terry(wins, draws)
        score = wins + draws / 2
        out = {"names": self.names, "games_per_pair": self.games_per_pair, "seed": self.seed,
               "wins": wins.astype(int).tolist(), "draws": draws.astype(int).tolist(), "losses": losses.astype(int).tolist(),
               "score": [float(x) for x in score.sum(axis=1)], "elo": [round(float(x), 3) for x in elo],
               "pair_score": [[float(x) for x in row] for row in score],
               "games": [dict({"round": g.round, "black_model": g.black_model, "white_model": g.white_model, "black_slot": g.black_slot,
                               "white_slot": g.white_slot, "winner": r[0], "blacks": r[3][0], "whites": r[3][1]},
                              **({"moves": [p["action"] for p in played["plies"]], "movers": [p["who"] for p in played["plies"]]} if keep_games else {}))
                         for g, r, played in zip(self.schedule, results, games)]}
        if out_path:
            with open(out_path, "wt") as f:
                f.write(dump(out))
        return out


def dump(result):
    """The result as JSON text: sorted keys, floats with three decimals."""
    def text(x):
        if isinstance(x, float):
            return f"{x:.3f}"
        if isinstance(x, dict):
            return "{" + ", ".join(f"{json.dumps(str(k))}: {text(x[k])}" for k in sorted(x)) + "}"
        if isinstance(x, (list, tuple)):
            return "[" + ", ".join(text(v) for v in x) + "]"
        return json.dumps(x)
    return text(result) + "\n"
