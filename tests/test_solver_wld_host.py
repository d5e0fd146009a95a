"""CPU: the yardstick of tests/solver_wld_cases.py - tests/native/wld_check.c, a plain host negamax over win / draw / loss - against
the signs of ab_check's exact root values and of the recorded ones at 15..17 empties, the recorded fixture at 18..21 empties against
its generator, the coverage conditions of the lists, the size query of raz_solve_wld on the real library (it needs no device), and
the analysis glue with a stub solver."""
import pytest

import solver_exact_cases as X
import solver_wld_cases as W


def _signs(values):
    return {s: W.sign(v) for s, v in values.items()}


def test_wld_check_equals_the_signs_of_ab_check_at_1_to_10_empties():
    for e in range(1, 11):
        for c in X.random_cases(e, 16):
            _, values, _ = X.ab_answer(*c[:3])
            ans, outcomes, _ = W.wld_answer(*c[:3])
            assert outcomes == _signs(values) and ans == W.from_values(values), (e, hex(c[0]), hex(c[1]), c[2])


def test_wld_check_equals_the_recorded_root_values_at_15_to_17():
    import json
    import os
    with open(os.path.join(W.GOLDEN, "solver_exact_deep.json")) as f:
        doc = json.load(f)
    assert sorted({p["empties"] for p in doc["positions"]}) == [15, 16, 17]
    for p, case in zip(doc["positions"], W.deep2_cases()):
        values = {int(s): v for s, v in p["root_values"].items()}
        ans, outcomes, _ = W.wld_answer(*case[:3])
        assert outcomes == _signs(values) and ans == case[4][1], p["black"]


def test_the_fixture_beyond_17_empties_is_the_generators():
    cases = W.deep3_cases()
    assert [W.empties_of(c) for c in cases] == [18] * 4 + [19] * 4 + [20] * 4 + [21] * 2
    doc = W.deep3_doc()["positions"]
    assert all(p["nodes"] > 0 and 0 <= p["seconds"] < 60 for p in doc)
    upto20 = [p for p in doc if p["empties"] <= 20]
    assert {p["wld"][1] for p in upto20} >= {1, -1} and any(0 in p["root_outcomes"].values() for p in upto20)
    b, w, p, _, ans = cases[3]
    got, outcomes, nodes = W.wld_answer(b, w, p)   # (the cheapest row, recomputed: a twentieth of a second)
    assert got == ans[1] and outcomes == {int(s): v for s, v in doc[3]["root_outcomes"].items()} and nodes == doc[3]["nodes"]


def test_status_rows_and_coverage():
    rows = W.status_cases()
    assert sorted({r[3] for r in rows}) == [0, 1, 2, 3]
    assert W.empties_of(rows[-1]) == W.MAX_EMPTIES + 1 and rows[-1][3] == 2
    got = W.assert_wld_coverage()
    assert all(v >= 10 for v in got.values()), got
    emu = W.assert_wld_coverage(emu=True)
    assert emu["differs from the exact move"] >= 10 and emu["draw"] >= 3 and emu["win, first move does not win"] >= 10, emu


def test_size_query_on_the_real_library():
    from reversi_alpha_zero_amd import _native as N
    from reversi_alpha_zero_amd.lib.reversi_solver import WLD_MAX_EMPTIES
    assert WLD_MAX_EMPTIES == W.MAX_EMPTIES
    size, m = N.lib.raz_solve_wld_workspace_bytes, W.MAX_EMPTIES
    assert size(100, m + 1) == 0 and size((1 << 31) + 1, m) == 0
    assert 0 < size(100, 0) < size(100, 14) < size(100, m) < size(100000, m)
    assert [size(7, e) for e in range(m + 1)] == sorted(size(7, e) for e in range(m + 1))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a machine without a GPU")
def test_without_a_gpu_the_call_is_a_device_error():
    from reversi_alpha_zero_amd import _native as N
    need = N.lib.raz_solve_wld_workspace_bytes(100, 17)
    fake = 1 << 20   # (never dereferenced: the first HIP call fails)
    assert N.lib.raz_solve_wld(fake, fake, fake, 100, fake, fake, fake, fake, need, 0, None) == W.RAZ_EDEVICE, N.last_error()
    assert N.lib.raz_solve_wld(None, None, None, 0, None, None, None, None, 0, 0, None) == W.RAZ_OK


# ---- the analysis glue (lib/analysis.py annotate_wld) with a stub solver ---------------------------------------------------------
class StubSolver:
    """solve_exact_batch by ab_check and solve_wld_batch by wld_check, on CPU tensors; counts the calls."""

    def __init__(self):
        self.exact_calls = self.wld_calls = 0

    @staticmethod
    def _answer(answer, black, white, player):
        import numpy as np
        import torch
        mv, sc, st = [], [], []
        for b, w, p in zip(black.numpy().view(np.uint64).tolist(), white.numpy().view(np.uint64).tolist(), player.tolist()):
            ans = answer(b, w, p)[0]
            mv.append(ans[0]), sc.append(ans[1]), st.append(0 if ans != W.NO_MOVE else 1)
        return torch.tensor(mv, dtype=torch.int8), torch.tensor(sc, dtype=torch.int8), torch.tensor(st, dtype=torch.uint8)

    def solve_exact_batch(self, black, white, player):
        self.exact_calls += 1
        return self._answer(X.ab_answer, black, white, player)

    def solve_wld_batch(self, black, white, player):
        self.wld_calls += 1
        return self._answer(W.wld_answer, black, white, player)


@pytest.fixture(scope="module")
def games():
    """Playouts from 8-empties positions, with and without pass entries, as test_solver_exact_host.py lists them."""
    import random
    from test_solver_exact_host import _game
    rng, out = random.Random(6), []
    for k, (b, w, p) in enumerate(X.random_positions(8, 80, 9208)):
        g = _game(b, w, p, rng, pass_entries=k % 2 == 0)
        if any(x["state"] == "pass_entry" for x in g) or len(out) < 3:
            out.append(g)
        if len(out) >= 7:
            break
    assert sum(any(x["state"] == "pass_entry" for x in g) for g in out) >= 2
    return out


@pytest.mark.parametrize("exact_empties", [None, 5])
def test_the_analysis_glue_with_a_stub_solver(games, exact_empties):
    import copy
    from reversi_alpha_zero_amd.lib.analysis import annotate_exact, annotate_wld
    stub, mine = StubSolver(), copy.deepcopy(games)
    if exact_empties:
        annotate_exact(mine, exact_empties, stub, device="cpu")
    before = copy.deepcopy(mine)
    annotate_wld(mine, 8, stub, exact_empties, device="cpu")
    assert stub.wld_calls == 2   # (one for the positions, one for the positions after the played moves)
    fields = {"solved_outcome", "outcome_move", "played_outcome", "outcome_kept"}
    seen = {"played": 0, "pass_entry": 0, "not kept": 0, "end": 0, "left to the exact solver": 0}
    for g, olds in zip(mine, before):
        for i, (d, old) in enumerate(zip(g, olds)):
            e = 64 - bin(d["black"] | d["white"]).count("1")
            added = {k: v for k, v in d.items() if k not in old}
            assert {k: d[k] for k in old} == old
            if d["state"] == "over" or e <= (exact_empties or 0):
                assert not added
                seen["left to the exact solver"] += d["state"] != "over"
                continue
            assert set(added) <= fields
            if d["state"] == "pass_entry":   # the side to move cannot move: the outcome of the position after it, from its view
                nxt = g[i + 1]
                want = W.wld_answer(nxt["black"], nxt["white"], nxt["player"])[0][1] if nxt["state"] != "over" else W.sign(nxt["disc_diff"])
                assert added == {"outcome_move": None, "solved_outcome": want if nxt["player"] == d["player"] else -want}
                seen["pass_entry"] += 1
                continue
            ans, outcomes, _ = W.wld_answer(d["black"], d["white"], d["player"])
            assert (d["outcome_move"], d["solved_outcome"]) == ans
            assert d["played_outcome"] == outcomes[d["played"]], (i, d)   # (wld_check records every root move's own outcome)
            assert d["outcome_kept"] is (outcomes[d["played"]] == ans[1])
            seen["played"] += 1
            seen["not kept"] += not d["outcome_kept"]
            seen["end"] += g[i + 1]["state"] == "over"
    if exact_empties:   # (the games' last plies - their passes and ends among them - are the exact solver's then)
        assert seen["played"] > 0 and seen["left to the exact solver"] > 0, seen
    else:
        assert all(v > 0 for k, v in seen.items() if k != "left to the exact solver") and seen["left to the exact solver"] == 0, seen


def test_the_analysis_glue_refuses_and_leaves_alone(games):
    import copy
    from reversi_alpha_zero_amd.lib.analysis import annotate_wld
    for bad in (0, W.MAX_EMPTIES + 1, -1, 2.5, "6"):
        with pytest.raises(ValueError):
            annotate_wld(copy.deepcopy(games), bad, StubSolver(), device="cpu")
    stub, mine = StubSolver(), copy.deepcopy(games)
    annotate_wld(mine, 8, stub, exact_empties=8, device="cpu")   # (everything is the exact solver's: nothing is asked, nothing added)
    assert stub.wld_calls == 0 and mine == games
