"""Schedules and ratings of a league of models (worker/league.py): host only, numpy f64, no device work.

round_robin   every pair of models meets games_per_pair times with colours alternating; game slots per model
tally         wins / draws / losses matrices from per-game results
bradley_terry maximum-likelihood Bradley-Terry strengths as Elo differences to model 0
"""
from collections import namedtuple

import numpy as np

Game = namedtuple("Game", "round black_model black_slot white_model white_slot")


def opponent_rank(m, o):
    """The rank of model o among the models other than m."""
    return o if o < m else o - 1


def round_robin(n_models, games_per_pair):
    """(games, slot_map).  games: rounds in order and, inside a round, the pairs (i < j) in lexicographic order; in round r of a pair
    model i is black when r is even.  Model m's game of round r against the opponent of rank q among the other models has index
    k = r * (n_models - 1) + q: slot k of m's engine serves it, and k is the game's id in that engine.  slot_map[m][k] is the index
    in `games` of the game model m plays in its slot k: every model's k values are exactly 0 .. (n_models - 1) * games_per_pair - 1,
    contiguous per round."""
    M, G = int(n_models), int(games_per_pair)
    if M < 2 or G < 1:
        raise ValueError("round_robin: at least two models and one game a pair")
    games, slot_map = [], [[None] * ((M - 1) * G) for _ in range(M)]
    for r in range(G):
        for i in range(M):
            for j in range(i + 1, M):
                ki, kj = r * (M - 1) + opponent_rank(i, j), r * (M - 1) + opponent_rank(j, i)
                black, white = ((i, ki), (j, kj)) if r % 2 == 0 else ((j, kj), (i, ki))
                slot_map[i][ki] = slot_map[j][kj] = len(games)
                games.append(Game(r, black[0], black[1], white[0], white[1]))
    return games, slot_map


def tally(results, n_models):
    """(wins, draws, losses) [n_models, n_models] f64 from per-game (winner model or None, black_model, white_model, ...):
    wins[i, j] games i won against j, draws[i, j] = draws[j, i], losses = wins transposed."""
    wins, draws = np.zeros((n_models, n_models)), np.zeros((n_models, n_models))
    for winner, black, white, *_ in results:
        if winner is None:
            draws[black, white] += 1
            draws[white, black] += 1
        else:
            wins[winner, white if winner == black else black] += 1
    return wins, draws, wins.T.copy()


def bradley_terry(wins, draws, max_sweeps=100000, tol=1e-12):
    """Elo [n] of the maximum-likelihood Bradley-Terry model, model 0 the anchor at 0.  Scores s_ij = wins_ij + draws_ij / 2 plus a
    PRIOR of one drawn game between every pair (+0.5 to s_ij and s_ji), so that an unbeaten model keeps a finite rating.  Solved by
    the MM iteration gamma_i <- sum_j s_ij / sum_j (n_ij / (gamma_i + gamma_j)), n_ij = s_ij + s_ji, from all ones, the models updated
    in index order within a sweep, until the largest relative change of a sweep is below `tol` or max_sweeps sweeps have passed."""
    wins, draws = np.asarray(wins, dtype=np.float64), np.asarray(draws, dtype=np.float64)
    n = wins.shape[0]
    if wins.shape != (n, n) or draws.shape != (n, n) or n < 2:
        raise ValueError("bradley_terry: square matrices of at least two models")
    s = wins + draws / 2 + 0.5
    np.fill_diagonal(s, 0.0)
    games = s + s.T
    won = s.sum(axis=1)
    gamma = np.ones(n)
    for _ in range(max_sweeps):
        change = 0.0
        for i in range(n):
            new = won[i] / (games[i] / (gamma[i] + gamma)).sum()   # (games[i, i] = 0)
            change = max(change, abs(new - gamma[i]) / gamma[i])
            gamma[i] = new
        if change < tol:
            break
    return 400.0 * np.log10(gamma / gamma[0])
