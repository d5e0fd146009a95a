"""CPU: lib/rating.py - the round-robin schedule with its slot map, the tally, and Bradley-Terry ratings against closed forms."""
import math

import numpy as np
import pytest


@pytest.mark.parametrize("M,G", [(2, 1), (3, 2), (4, 34), (5, 3), (16, 2)])
def test_round_robin_schedule_and_slot_map(M, G):
    from reversi_alpha_zero_amd.lib.rating import round_robin
    games, slot_map = round_robin(M, G)
    assert len(games) == M * (M - 1) // 2 * G
    met = {}
    for g in games:
        met.setdefault((min(g.black_model, g.white_model), max(g.black_model, g.white_model)), []).append(g)
    assert sorted(met) == [(i, j) for i in range(M) for j in range(i + 1, M)]
    for (i, j), gs in met.items():   # games_per_pair meetings, colours alternating, model i black in the even rounds
        assert [g.round for g in gs] == list(range(G))
        assert [g.black_model for g in gs] == [i if r % 2 == 0 else j for r in range(G)]
    assert [g.round for g in games] == sorted(g.round for g in games)   # whole rounds lie together
    in_round = [(min(g.black_model, g.white_model), max(g.black_model, g.white_model)) for g in games if g.round == 0]
    assert in_round == sorted(in_round)                                  # pairs in lexicographic order
    for m in range(M):
        ks = sorted((g.black_slot if g.black_model == m else g.white_slot, g.round, g.white_model if g.black_model == m else g.black_model)
                    for g in games if m in (g.black_model, g.white_model))
        assert [k for k, _, _ in ks] == list(range((M - 1) * G))         # exactly 0 .. (M-1)G - 1
        assert [r for _, r, _ in ks] == [k // (M - 1) for k in range((M - 1) * G)]   # contiguous per round
        others = [o for o in range(M) if o != m]
        assert [o for _, _, o in ks] == others * G                       # k = r (M-1) + the opponent's rank
        for k in range((M - 1) * G):
            g = games[slot_map[m][k]]
            assert (g.black_model, g.black_slot) == (m, k) or (g.white_model, g.white_slot) == (m, k)
    with pytest.raises(ValueError):
        round_robin(1, 2)


def test_tally():
    from reversi_alpha_zero_amd.lib.rating import tally
    results = [(0, 0, 1, (40, 24)), (0, 1, 0, (20, 44)), (None, 0, 2, (32, 32)), (2, 1, 2, (10, 54)), (1, 1, 2, (33, 31))]
    wins, draws, losses = tally(results, 3)
    assert wins.tolist() == [[0, 2, 0], [0, 0, 1], [0, 1, 0]]
    assert draws.tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]
    assert (losses == wins.T).all() and wins.dtype == np.float64


@pytest.mark.parametrize("w,d,l", [(3, 0, 0), (0, 0, 5), (7, 2, 4), (1, 9, 1), (120, 13, 71), (0, 0, 0)])
def test_bradley_terry_two_models_closed_form(w, d, l):
    from reversi_alpha_zero_amd.lib.rating import bradley_terry
    elo = bradley_terry(np.array([[0, w], [l, 0]]), np.array([[0, d], [d, 0]]))
    assert elo[0] == 0.0
    assert abs((elo[0] - elo[1]) - 400 * math.log10((w + d / 2 + 0.5) / (l + d / 2 + 0.5))) <= 1e-9


def test_bradley_terry_cycle_relabelling_and_unbeaten():
    from reversi_alpha_zero_amd.lib.rating import bradley_terry
    cycle = np.array([[0, 3, 0], [0, 0, 3], [3, 0, 0]], dtype=float)   # 0 beats 1 beats 2 beats 0: equal scores
    assert np.abs(bradley_terry(cycle, np.zeros((3, 3)))).max() <= 1e-9
    rng = np.random.default_rng(5)
    n = 6
    wins = rng.integers(0, 9, size=(n, n)).astype(float)
    np.fill_diagonal(wins, 0)
    draws = rng.integers(0, 4, size=(n, n)).astype(float)
    draws = draws + draws.T
    np.fill_diagonal(draws, 0)
    elo = bradley_terry(wins, draws)
    perm = rng.permutation(n)
    again = bradley_terry(wins[np.ix_(perm, perm)], draws[np.ix_(perm, perm)])   # model perm[a] carries the label a
    assert np.abs((again - again[list(perm).index(0)]) - elo[perm]).max() <= 1e-9   # re-anchored on the old model 0
    wins[2, :] = 5                                                      # model 2 never loses, never draws
    wins[:, 2] = 0
    draws[2, :] = draws[:, 2] = 0
    wins[2, 2] = 0
    top = bradley_terry(wins, draws)
    assert np.isfinite(top).all() and top[2] == top.max()
    # the stationary point: every model's score equals its expected score
    s = wins + draws / 2 + 0.5
    np.fill_diagonal(s, 0)
    g = 10 ** (top / 400)
    expect = ((s + s.T) * g[:, None] / (g[:, None] + g[None, :])).sum(axis=1)
    assert np.abs(expect - s.sum(axis=1)).max() <= 1e-8
