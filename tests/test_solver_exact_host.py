"""CPU: the yardstick of tests/solver_exact_cases.py - tests/native/ab_check.c, a plain host negamax with bounds - against the
oracle's full scan, the recorded fixture beyond 14 empties against its own root values, and the size query of raz_solve_exact on
the real library (it needs no device)."""
import pytest

import solver_exact_cases as X


def test_ab_check_equals_the_oracle_at_1_to_10_empties():
    for e in range(1, 11):
        for c in X.random_cases(e, 16):
            assert X.ab_answer(*c[:3])[0] == c[4][1], (e, hex(c[0]), hex(c[1]), c[2])


def test_ab_check_equals_the_recorded_13_and_14_fixture():
    for c in X.deep_cases():
        assert X.ab_answer(*c[:3])[0] == c[4][1], (hex(c[0]), hex(c[1]), c[2])


def test_the_fixture_beyond_14_empties_is_the_generators():
    cases = X.deep2_cases()
    assert [64 - bin(c[0] | c[1]).count("1") for c in cases] == [15] * 8 + [16] * 4 + [17] * 2
    b, w, p, _, ans = cases[1]
    assert X.ab_answer(b, w, p)[0] == ans[1]   # (the cheapest row, recomputed: a fifth of a second)


def test_status_rows_and_coverage():
    assert len(X.status_cases()) == 9
    got = X.assert_exact_coverage()
    assert got["tied maximum"] >= 10, got


def test_size_query_on_the_real_library():
    from reversi_alpha_zero_amd import _native as N
    size = N.lib.raz_solve_exact_workspace_bytes
    assert size(100, 18) == 0 and size((1 << 31) + 1, 17) == 0
    assert 0 < size(100, 0) < size(100, 14) < size(100, 17) < size(100000, 17)
    assert [size(7, e) for e in range(18)] == sorted(size(7, e) for e in range(18))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a machine without a GPU")
def test_without_a_gpu_the_call_is_a_device_error():
    from reversi_alpha_zero_amd import _native as N
    need = N.lib.raz_solve_exact_workspace_bytes(100, 17)
    fake = 1 << 20   # (never dereferenced: the first HIP call fails)
    assert N.lib.raz_solve_exact(fake, fake, fake, 100, fake, fake, fake, fake, need, 0, None) == X.RAZ_EDEVICE, N.last_error()
    assert N.lib.raz_solve_exact(None, None, None, 0, None, None, None, None, 0, 0, None) == X.RAZ_OK


# ---- the analysis glue (lib/analysis.py annotate_exact) with a stub solver -------------------------------------------------------
class StubSolver:
    """solve_exact_batch on CPU tensors, answered by ab_check; counts its calls."""

    def __init__(self):
        self.calls = 0

    def solve_exact_batch(self, black, white, player):
        import numpy as np
        import torch
        self.calls += 1
        mv, sc, st = [], [], []
        for b, w, p in zip(black.numpy().view(np.uint64).tolist(), white.numpy().view(np.uint64).tolist(), player.tolist()):
            ans = X.ab_answer(b, w, p)[0]
            mv.append(ans[0]), sc.append(ans[1]), st.append(0 if ans != X.NO_MOVE else 1)
        return torch.tensor(mv, dtype=torch.int8), torch.tensor(sc, dtype=torch.int8), torch.tensor(st, dtype=torch.uint8)


def _game(black, white, player, rng, pass_entries):
    """A random playout as analyze() lists it: a `search` dictionary per move, a `pass_entry` (the side that cannot move) where
    pass_entries is set, and the `over` position at the end."""
    out, made = [], 0
    while True:
        own, enemy = (black, white) if player == 1 else (white, black)
        legal = X.moves_of(own, enemy)
        if not legal:
            if not X.moves_of(enemy, own):
                nb, nw = bin(black).count("1"), bin(white).count("1")
                out.append({"moves_made": made, "player": player, "black": black, "white": white, "state": "over", "played": None,
                            "discs": (nb, nw), "disc_diff": nb - nw if player == 1 else nw - nb})
                return out
            if pass_entries:
                out.append({"moves_made": made, "player": player, "black": black, "white": white, "state": "pass_entry", "played": None})
            player = 3 - player
            continue
        a = rng.choice(X.squares(legal))
        out.append({"moves_made": made, "player": player, "black": black, "white": white, "state": "search", "played": a, "eval": 0.0})
        own, enemy = X.play(a, own, enemy)
        black, white = (own, enemy) if player == 1 else (enemy, own)
        player, made = 3 - player, made + 1


@pytest.fixture(scope="module")
def games():
    """Playouts from 7-empties positions until the list holds a pass, a mover change and (always) a game that ends."""
    import random
    rng, out = random.Random(5), []
    for k, (b, w, p) in enumerate(X.random_positions(7, 60, 9207)):
        g = _game(b, w, p, rng, pass_entries=k % 2 == 0)
        passes = any(x["state"] == "pass_entry" for x in g) or any(a["player"] == b_["player"] for a, b_ in zip(g, g[1:]) if a["state"] == "search")
        if passes or len(out) < 2:
            out.append(g)
        if len(out) >= 6 and sum(any(x["state"] == "pass_entry" for x in g) for g in out) >= 2:
            break
    assert sum(any(x["state"] == "pass_entry" for x in g) for g in out) >= 2
    assert any(a["state"] == b_["state"] == "search" and a["player"] == b_["player"] for g in out for a, b_ in zip(g, g[1:])), "no silent pass"
    assert any(a["player"] != b_["player"] for g in out for a, b_ in zip(g, g[1:]))
    return out


def test_the_analysis_glue_with_a_stub_solver(games):
    import copy
    from reversi_alpha_zero_amd.lib.analysis import annotate_exact
    stub, mine = StubSolver(), copy.deepcopy(games)
    annotate_exact(mine, 6, stub, device="cpu")
    assert stub.calls == 1
    seen = {"played": 0, "pass_entry": 0, "lost": 0, "end": 0}
    for g, before in zip(mine, games):
        for i, (d, old) in enumerate(zip(g, before)):
            e = 64 - bin(d["black"] | d["white"]).count("1")
            added = {k: v for k, v in d.items() if k not in old}
            assert {k: d[k] for k in old} == old
            if d["state"] == "over" or e > 6:
                assert not added
                continue
            if d["state"] == "pass_entry":   # the side to move cannot move: the value of the position after it, from its view
                nxt = g[i + 1]
                want = X.ab_answer(nxt["black"], nxt["white"], nxt["player"])[0][1] if nxt["state"] != "over" else nxt["disc_diff"]
                assert added == {"solved_move": None, "solved_score": want if nxt["player"] == d["player"] else -want}
                seen["pass_entry"] += 1
                continue
            ans, values, _ = X.ab_answer(d["black"], d["white"], d["player"])
            assert (d["solved_move"], d["solved_score"]) == ans
            assert d["played_score"] == values[d["played"]], (i, d)   # (every root move's exact value: ab_check records them all)
            assert d["played_loss"] == ans[1] - values[d["played"]] >= 0
            assert (d["played_loss"] == 0) == (values[d["played"]] == ans[1])
            seen["played"] += 1
            seen["lost"] += d["played_loss"] > 0
            seen["end"] += g[i + 1]["state"] == "over"
    assert all(v > 0 for v in seen.values()), seen


def test_the_analysis_glue_refuses_and_leaves_alone(games):
    import copy
    from reversi_alpha_zero_amd.lib.analysis import annotate_exact
    for bad in (0, 18, -1, 2.5, "6"):
        with pytest.raises(ValueError):
            annotate_exact(copy.deepcopy(games), bad, StubSolver(), device="cpu")
    stub, mine = StubSolver(), copy.deepcopy(games)
    annotate_exact(mine, 1, stub, device="cpu")   # (only positions of one empty square: everything above stays as it was)
    assert all(d == old for g, before in zip(mine, games) for d, old in zip(g, before) if 64 - bin(d["black"] | d["white"]).count("1") > 1)
