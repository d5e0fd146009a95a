"""GPU: the retrograde analysis on the device (include/raz.h raz_analysis_*, engine.DeviceAnalysis) and what is built on it -
lib/analysis.GameAnalyzer, the NBoard engine's `analyze` - against an independent walk of the lists and a second engine armed slot
by slot with raz_engine_set_position.  The cases and the guarded harness around DeviceAnalysis are tests/analysis_cases.py's; the
wave emulator runs them through the same product wrappers in tests/test_analysis_emu.py.  Mini net 16x1 at 8 simulations a move unless stated."""
import ctypes
import io

import numpy as np
import pytest
import torch

import analysis_cases as C
import match_cases as M
from test_match_gpu import DEV, Gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blob():
    return M.mini_blobs()[0]


@pytest.fixture(scope="module")
def special():
    sp = C.special_games()
    C.assert_special_set(sp)
    return sp


@pytest.fixture(scope="module")
def small_engine(blob):
    return Gpu.engine(M.engine_cfg(M.mini_config(1)), blob, 257 * 2, 3, 8, nodes_per_game=40)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_replay_of_one_entry_lists(small_engine, n):
    """Case 1 at max_moves = 1, either side of the 256 threads of a one-thread-per-game block."""
    C.check_replay(Gpu, small_engine, C.one_entry_games(n), 1)


def test_replay_of_the_special_set(blob, special):
    """Case 1 at max_moves = 64 (the set is asserted by the fixture)."""
    names = sorted(special)
    C.check_walk_against_facade([special[k] for k in names], 64)
    e = Gpu.engine(M.engine_cfg(M.mini_config(1)), blob, len(names) * 65 + 3, 3, 8, nodes_per_game=40)
    C.check_replay(Gpu, e, [special[k] for k in names], 64, first_slot=3)


def _mid(seed, discs=20):
    return M.playout_positions(seed, 1, discs)[0]


def _from(start, k, seed=1):
    return (start, C.playout(C.Random(seed), start)[0][:k])


SEARCH_CASES = {   # 1 searched position of 2, then 3, 4, 5 and 65 positions: either side of the 4 waves of a workgroup
    "one": lambda sp: ([(_mid(1), [])], 1),
    "three": lambda sp: ([_from(_mid(2), 2)], 2),
    "four": lambda sp: ([_from(_mid(3), 1), _from(None, 1)], 1),
    "five": lambda sp: ([_from(_mid(4, 30), 4)], 4),
    "sixty_five": lambda sp: ([sp["full60"]], 64),
}


@pytest.mark.parametrize("psn", [1, 4])
@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_collect_equals_set_position_and_numpy(blob, special, name, psn):
    """Case 2: the evals are, byte for byte, what numpy makes of record 0 of a second engine armed slot by slot."""
    games, mm = SEARCH_CASES[name](special)
    got, exp, want = C.case_search(Gpu, blob, games, mm, psn)
    assert (exp["state"] >= 2).sum() == sum(sm["searched"] for _, sm in want)
    if name == "sixty_five":   # use_solver_turn 50 as shipped: the late positions are the root solver's
        assert (exp["state"][0, 50:60] == 3).all() and (exp["state"][0, :46] == 2).all() and exp["state"][0, 60] == 0
        assert exp[0, 55]["n_top"] == 1 and exp[0, 55]["top_n"][0] == 999
    if name == "five":
        s = exp[exp["state"] == 2]
        assert ((s["n_top"] > 0) & (s["n_top"] < 8)).any()                                           # fewer than 8 visited squares
        assert any(len(set(r["top_n"][:r["n_top"]].tolist())) < r["n_top"] for r in s)               # ties in n


def test_collect_cuts_at_eight_squares(blob):
    """Case 2 at 64 simulations on a position of 12 legal moves or more: more than RAZ_ANALYSIS_TOP squares are visited."""
    wide = next(p for p in M.playout_positions(9, 40, 24) if len(C.py_legal(*(p[:2] if p[2] == 1 else p[1::-1]))) >= 12)
    got, exp, _ = C.case_search(Gpu, blob, [(wide, [])], 1, 1, sims=64)
    assert exp[0, 0]["n_top"] == 8 and exp[0, 0]["sum_n"] > exp[0, 0]["top_n"].sum()


@pytest.mark.parametrize("psn", [1, 4])
def test_collect_is_independent_and_idempotent(blob, psn):
    """Case 3."""
    cfg = M.engine_cfg(M.mini_config(psn))
    games = [_from(_mid(10 + g, 16 + 4 * g), 3, seed=g) for g in range(5)]
    mm, n_slots = 3, 5 * 4
    want = [C.py_walk(s, e, mm) for s, e in games]

    def run(gs, step, collect_every, first_slot=0):
        e = Gpu.engine(cfg, blob, n_slots, 21, 8, first_game_id=500)
        an = Gpu.analysis(e, len(gs), mm, first_slot=first_slot)
        an.start(*C.pack(gs, mm), 8)
        C.run_device(Gpu, e, an, step=step, collect_every=collect_every)
        return e, an

    e, every = run(games, 1, 1)
    ws = every.workspace()
    every.collect()   # a second collect changes no byte
    e.step(4)
    every.collect()
    assert (every.workspace() == ws).all()
    _, once = run(games, 1, 64)
    C.assert_same_evals("collect once", once.read()[2], every.read()[2])
    C.assert_same_evals("host", every.read()[2], C.host_route(Gpu, cfg, blob, n_slots, 21, 500, 8, want, mm))
    for g in (0, 3):   # game g alone on the same slots
        _, an = run([games[g]], 3, 1, first_slot=g * 4)
        C.assert_same_evals(("alone", g), an.read()[2], every.read()[2][g:g + 1])
        an.check_guard()
    every.check_guard()
    once.check_guard()


def test_collect_before_any_step_changes_nothing(blob):
    e = Gpu.engine(M.engine_cfg(M.mini_config(4)), blob, 10, 1, 8)
    an = Gpu.analysis(e, 2, 4)
    an.start(*C.pack([_from(_mid(8), 4), _from(_mid(7), 2)], 4), 8)
    before = an.workspace()
    for _ in range(3):
        an.collect()
    assert (an.workspace() == before).all()
    evals = an.read()[2]
    assert set(evals["state"].reshape(-1).tolist()) == {0, 1} and (evals["state"] == 1).sum() == an.stats()["pending"] == 8
    an.check_guard()


def test_analysis_refusals_and_engine_error(blob):
    """Case 4 through engine.DeviceAnalysis: refusals name their reason, CPU tensors are refused, and a 40-node pool at 64
    simulations ends with the error word set and nothing pending."""
    from reversi_alpha_zero_amd._native import lib
    from reversi_alpha_zero_amd.engine import DeviceAnalysis, DeviceNet, SelfPlayEngine, analysis_error_text
    cfg = M.engine_cfg(M.mini_config(1, sims=64))
    moves = torch.full((2, 2), -2, dtype=torch.int8, device=DEV)
    no_w = SelfPlayEngine(cfg, DeviceNet(blob, DEV), 6, seed=0, sims_hint=8, max_plies=64, parts=1, single_stream=True)
    no_w.start(0, 8, n_active=0)
    with pytest.raises(RuntimeError, match="record_root_w"):
        DeviceAnalysis(no_w).start(moves, None, 8)
    e = Gpu.engine(cfg, blob, 6, 0, 64, nodes_per_game=40)
    with pytest.raises(RuntimeError, match="beyond the engine's slots"):
        DeviceAnalysis(e, first_slot=1).start(moves, None, 8)
    a = DeviceAnalysis(e)
    with pytest.raises(ValueError, match="device tensor"):
        a.start(moves.cpu(), None, 8)
    with pytest.raises(ValueError, match="sims"):
        a.start(moves, None, 0)
    with pytest.raises(ValueError, match="max_moves"):
        a.start(torch.zeros((1, 128), dtype=torch.int8, device=DEV), None, 8)
    assert lib.raz_analysis_collect(None, None) == -1
    an = Gpu.analysis(e, 2, 2)
    an.start(*C.pack([_from(_mid(5, 24), 2), _from(_mid(6, 24), 1)], 2), 64)
    for _ in range(400):
        e.step(2)
        an.collect()
        st = an.stats()
        if not st["pending"]:
            break
    assert st["pending"] == 0 and st["failed"] >= 1 and st["failed"] + st["searched"] + st["solved"] == st["armed"] == 5, st
    assert st["error"] & 1 and "node pool full" in analysis_error_text(st["error"])
    with pytest.raises(RuntimeError, match="analysis error word"):
        an.w.stats()
    an.check_guard()


# ---- case 5: Python on the device ---------------------------------------------------------------------------------------------
def _python_config(psn=4):
    cfg = M.mini_config(psn)
    cfg.play.simulation_num_per_move = 8
    cfg.play_with_human.parallel_search_num = psn
    cfg.play_with_human.update_play_config(cfg.play)   # as play_game.nboard.start does
    return cfg


def test_game_analyzer_equals_the_host_route_over_two_passes(blob):
    """GameAnalyzer.analyze on 3 GGF strings, 2 games a pass, against slots armed one by one with raz_engine_set_position."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.agent.player import effective_play_config
    from reversi_alpha_zero_amd.engine import ANALYSIS_POS
    from reversi_alpha_zero_amd.lib.analysis import GameAnalyzer, positions_of
    from reversi_alpha_zero_amd.lib.ggf import convert_action_to_move, make_ggf_string
    import types
    cfg = _python_config()
    lists = [C.playout(C.Random(40 + g))[0][:k] for g, k in enumerate((14, 11, 9))]
    texts = [make_ggf_string("b", "w", moves=[convert_action_to_move(a) for a in x]) for x in lists]
    mm = 14
    P = mm + 1
    net = ReversiNet(16, 1, 16).keras_init_(1).randomize_bn_(2)
    assert net.to_blob() == blob
    ga = GameAnalyzer(cfg, net, cfg.play, slots=2 * P + 3, device=DEV)
    got = ga.analyze(texts)
    assert ga.passes == 2 and [len(g) for g in got] == [15, 12, 10]
    ecfg = types.SimpleNamespace(play=effective_play_config(cfg, cfg.play), play_data=cfg.play_data)
    for lo, chunk in ((0, [0, 1]), (2, [2])):
        want = [C.py_walk(None, lists[g], mm) for g in chunk]
        exp = C.host_route(Gpu, ecfg, blob, 2 * P + 3, 0, lo * P, 8, want, mm)
        for i, g in enumerate(chunk):
            pos = np.zeros(P, dtype=ANALYSIS_POS)
            for j, p in enumerate(want[i][0]):
                pos[j] = (p[0], p[1], p[2], p[3], p[4], p[5], 0)
            assert got[g] == positions_of(pos, exp[i]), g
    d = got[0][3]
    assert d["moves_made"] == 3 and d["player"] in (1, 2) and d["played"] == lists[0][3] and d["visits"] >= 1 and not d["exact"]
    assert d["eval"] == d["top"][0][2] and d["best_move"] == d["top"][0][0] and d["played_diff"] == d["played_eval"] - d["eval"]


@pytest.mark.parametrize("psn", [1, 4])
def test_collect_fails_a_position_whose_slot_left_the_one_move_protocol(blob, psn):
    """Case 7: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    C.case_slot_off_protocol(Gpu, blob, psn)


def test_nboard_engine_session_on_the_device(blob):
    """A scripted NBoardEngine session on in-memory streams: go is a fresh ReversiPlayer's move, hint ranks by visits with the best
    last, ping is answered, analyze sends one line per position."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.agent.player import ReversiPlayer
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
    from reversi_alpha_zero_amd.lib.ggf import convert_action_to_move, make_ggf_string
    from reversi_alpha_zero_amd.play_game.nboard import NBoardEngine
    cfg = _python_config()
    cfg.nboard.read_stdin_timeout = 0.01
    net = ReversiNet(16, 1, 16).keras_init_(1).randomize_bn_(2)
    opening = C.playout(C.Random(3))[0][:4]
    env = ReversiEnv().reset()
    for a in opening:
        env.step(a)
    fresh = ReversiPlayer(cfg, net, cfg.play, enable_resign=False)
    move = convert_action_to_move(fresh.action(*env.get_own_and_enemy()))
    script = ["nboard 2", "set game " + make_ggf_string("b", "w", moves=[convert_action_to_move(a) for a in opening]), "go", f"move {move}",
              "hint 3", "ping 7", "analyze", "learn"]
    out = io.StringIO()
    engine = NBoardEngine(cfg, stdin=io.StringIO("\n".join(script) + "\n"), stdout=out, model=net, device=DEV)
    engine.start()
    lines = out.getvalue().splitlines()
    go = next(x for x in lines if x.startswith("==="))
    assert go.split()[1].split("/")[0] == move
    waiting = [i for i, x in enumerate(lines) if x == "status waiting"]
    h = lines.index("status thinkng hint...")
    item = engine.player.ask_thought_about(*engine.env.get_own_and_enemy())
    top3 = [a for a, v in sorted(enumerate(item.visit), key=lambda x: -x[1])[:3] if v > 0]   # (8 simulations may visit fewer than 3 squares)
    end = next(i for i in waiting if i > h)
    last3 = lines[end - len(top3):end]
    assert len(top3) >= 1 and [x.split()[1] for x in last3] == [convert_action_to_move(a) for a in reversed(top3)]
    assert all(x.startswith("search ") for x in lines[h + 1:end])
    assert [int(x.split()[4]) for x in last3] == sorted(int(x.split()[4]) for x in last3)   # the last one is the best
    assert "pong 7" in lines and lines[-1] == "learned" and lines.index("pong 7") > h
    analysis = [x.split() for x in lines if x.startswith("analysis ")]
    assert [int(x[1]) for x in analysis] == list(range(len(opening) + 2)) and all(abs(float(x[2])) <= 10.0 for x in analysis)
    assert engine.env.next_player in (Player.black, Player.white)
