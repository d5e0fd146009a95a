"""CPU: the retrograde analysis on the device (include/raz.h raz_analysis_*, csrc/raz_analysis.h: k_analysis_start,
k_analysis_collect) on the WAVE EMULATOR - the kernels as they stand, on host memory, driven through the product's own wrappers
(engine.SelfPlayEngine and engine.DeviceAnalysis on tests/emu_util.py's backend) - against an independent walk of the lists and a second engine armed slot by slot with raz_engine_set_position.
The cases are tests/analysis_cases.py's; the device runs them in tests/test_analysis_gpu.py."""
import ctypes

import numpy as np
import pytest

import analysis_cases as C
import match_cases as M
from emu_util import EmuEngine, aligned, load
from test_match_emu import Emu


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
    """257 x 2 slots with a node pool kept small: the replay arms slots, nothing steps them."""
    return Emu.engine(M.engine_cfg(M.mini_config(1)), blob, 257 * 2, 3, 8, nodes_per_game=40)


def test_independent_walk_agrees_with_the_facade(special):
    """Case 1's expectation, checked once against the package's ReversiEnv on the lists the kernels get."""
    C.check_walk_against_facade(list(special.values()), 64)
    C.check_walk_against_facade(C.one_entry_games(257), 1)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_emulated_replay_of_one_entry_lists(small_engine, n):
    """Case 1 at max_moves = 1, either side of the 256 threads of a one-thread-per-game block."""
    games = C.one_entry_games(n)
    if n >= 7:
        kinds = {(tuple(e), s is None) for s, e in games}
        assert any(e == (C.PA,) for e, _ in kinds) and any(e == () for e, _ in kinds) and any(e and not -2 <= e[0] <= 63 for e, _ in kinds)
        assert any(s is not None and s[2] == 2 for s, _ in games)
    C.check_replay(Emu, small_engine, games, 1)


def test_emulated_replay_of_the_special_set(blob, special):
    """Case 1 at max_moves = 64: a full game, an automatic pass, a pass entry, white to move, an early end, an illegal move, entries
    after the end, an empty list, a list without terminator, a bad code."""
    names = sorted(special)
    e = Emu.engine(M.engine_cfg(M.mini_config(1)), blob, len(names) * 65 + 3, 3, 8, nodes_per_game=40)
    C.check_replay(Emu, e, [special[k] for k in names], 64, first_slot=3)


def _mid(seed, discs=20):
    return M.playout_positions(seed, 1, discs)[0]


def _from(start, k, seed=1):
    return (start, C.playout(C.Random(seed), start)[0][:k])


SEARCH_CASES = {   # name: (games, max_moves): 1 searched position of 2, then 3, 4, 5 and 65 positions - either side of 4 waves a block
    "one": lambda sp: ([(_mid(1), [])], 1),
    "three": lambda sp: ([_from(_mid(2), 2)], 2),
    "four": lambda sp: ([_from(_mid(3), 1), _from(None, 1)], 1),
    "five": lambda sp: ([_from(_mid(4, 30), 4)], 4),
    "sixty_five": lambda sp: ([sp["full60"]], 64),
}
_searched = {}


def searched(blob, special, name, psn):
    if (name, psn) not in _searched:
        games, mm = SEARCH_CASES[name](special)
        _searched[(name, psn)] = C.case_search(Emu, blob, games, mm, psn)
    return _searched[(name, psn)]


@pytest.mark.parametrize("psn", [1, 4])
@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_emulated_collect_equals_set_position_and_numpy(blob, special, name, psn):
    """Case 2: the evals of raz_analysis_* are, byte for byte, what numpy makes of record 0 of a second engine armed slot by slot."""
    got, exp, want = searched(blob, special, name, psn)
    assert (exp["state"] >= 2).sum() == sum(sm["searched"] for _, sm in want)
    if name == "sixty_five":   # use_solver_turn 50 as shipped: the late positions are the root solver's
        assert (exp["state"][0, 50:60] == 3).all() and (exp["state"][0, :46] == 2).all() and exp["state"][0, 60] == 0
        s = exp[0, 55]
        assert s["n_top"] == 1 and s["top_n"][0] == 999 and abs(s["top_q"][0]) <= 1.0 and s["top_square"][0] == s["action"]


def test_expectation_holds_few_squares_ties_and_a_cut(blob, special):
    """Case 2: a position with fewer than 8 visited squares, one with ties in n, and - at 64 simulations on a position of 12 legal moves or more - one with more than 8
    visited squares (the cut at RAZ_ANALYSIS_TOP), each present in the expectation before the device's bytes are compared."""
    exp = searched(blob, special, "five", 1)[1]
    s = exp[exp["state"] == 2]
    assert ((s["n_top"] > 0) & (s["n_top"] < 8)).any()
    assert any(len(set(r["top_n"][:r["n_top"]].tolist())) < r["n_top"] for r in s)
    wide = next(p for p in M.playout_positions(9, 40, 24) if len(C.py_legal(*(p[:2] if p[2] == 1 else p[1::-1]))) >= 12)
    got, exp, _ = C.case_search(Emu, blob, [(wide, [])], 1, 1, sims=64)
    assert exp[0, 0]["n_top"] == 8 and exp[0, 0]["sum_n"] > exp[0, 0]["top_n"].sum()


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_collect_is_independent_and_idempotent(blob, special, psn):
    """Case 3."""
    cfg = M.engine_cfg(M.mini_config(psn))
    games = [_from(_mid(10 + g, 16 + 4 * g), 3, seed=g) for g in range(5)]
    mm, n_slots = 3, 5 * 4
    want = [C.py_walk(s, e, mm) for s, e in games]

    def run(gs, first_id, step, collect_every, n=None):
        e = Emu.engine(cfg, blob, n_slots, 21, 8, first_game_id=first_id)
        an = Emu.analysis(e, len(gs), mm)
        an.start(*C.pack(gs, mm), 8)
        C.run_device(Emu, e, an, step=step, collect_every=collect_every)
        return e, an

    e, every = run(games, 500, 1, 1)
    ws = every.workspace()
    every.collect()   # a second collect changes no byte
    assert (every.workspace() == ws).all()
    e.step(4)
    every.collect()
    assert (every.workspace() == ws).all()
    _, once = run(games, 500, 1, 64)   # one collect after 64 steps
    C.assert_same_evals("collect once", once.read()[2], every.read()[2])
    C.assert_same_evals("host", every.read()[2], C.host_route(Emu, cfg, blob, n_slots, 21, 500, 8, want, mm))
    for g in (0, 3):   # game g alone on the SAME slots (the engine's ids shifted so that slot g * P + j has the id it had)
        e1 = Emu.engine(cfg, blob, n_slots, 21, 8, first_game_id=500)
        an = Emu.analysis(e1, 1, mm, first_slot=g * 4)
        an.start(*C.pack([games[g]], mm), 8)
        C.run_device(Emu, e1, an, step=3)
        C.assert_same_evals(("alone", g), an.read()[2], every.read()[2][g:g + 1])
        an.check_guard()
    every.check_guard()
    once.check_guard()


def test_emulated_collect_before_any_step_changes_nothing(blob):
    e = Emu.engine(M.engine_cfg(M.mini_config(4)), blob, 10, 1, 8)
    games = [_from(_mid(8), 4), _from(_mid(7), 2)]   # (not the initial position: its move is decided without a search)
    an = Emu.analysis(e, 2, 4)
    an.start(*C.pack(games, 4), 8)
    before = an.workspace()
    for _ in range(3):
        an.collect()
    assert (an.workspace() == before).all()
    evals = an.read()[2]
    assert set(evals["state"].reshape(-1).tolist()) == {0, 1} and (evals["state"] == 1).sum() == an.stats()["pending"] == 8
    e.step(1)   # mid-search slots (8 simulations take more than one step) are left alone too
    an.collect()
    assert (an.workspace() == before).all()
    an.check_guard()


def test_emulated_analysis_refusals(blob):
    """Case 4: every refusal gives its code and a recognisable message, and launches nothing."""
    lib = load()
    cfg = M.engine_cfg(M.mini_config(1))
    e = Emu.engine(cfg, blob, 10, 0, 8)
    idle = EmuEngine(cfg, blob, 10, seed=1, sims_hint=8, max_plies=64)   # created, not started
    no_w = EmuEngine(cfg, blob, 10, seed=1, sims_hint=8, max_plies=64, record_root_w=False)
    no_w.start(0, 8, n_active=0)
    need = lib.raz_analysis_workspace_bytes(2, 4)
    assert need >= 256 * 4 and need % 256 == 0
    assert lib.raz_analysis_workspace_bytes(0, 4) == 0
    assert lib.raz_analysis_workspace_bytes(2, 0) == 0 and b"max_moves" in lib.raz_last_error()
    assert lib.raz_analysis_workspace_bytes(2, 128) == 0 and b"max_moves" in lib.raz_last_error()
    assert lib.raz_analysis_workspace_bytes(1, 127) >= 128 * (24 + 128)
    mem, base = aligned(need + 64)
    view = np.ctypeslib.as_array((ctypes.c_uint8 * (need + 64)).from_address(base))
    view[:] = 0x55
    h = ctypes.c_void_p()
    controls = Emu.controls(e)

    def create(code, text, engine=e, first=0, ws=base, nbytes=need, n=2, mm=4, out=h):
        assert lib.raz_analysis_create(engine._h if engine else None, first, ws, nbytes, n, mm, ctypes.byref(out) if out is not None else None) == code
        assert text in lib.raz_last_error(), lib.raz_last_error()
    create(-1, b"NULL", engine=None)
    create(-1, b"NULL", ws=None)
    create(-1, b"NULL", out=None)
    create(-4, b"raz_engine_start", engine=idle)
    create(-4, b"record_root_w", engine=no_w)
    create(-1, b"beyond the engine's slots", first=1)
    create(-1, b"beyond the engine's slots", n=3, nbytes=lib.raz_analysis_workspace_bytes(3, 4))
    create(-1, b"aligned", ws=base + 64)
    create(-1, b"smaller than raz_analysis_workspace_bytes", nbytes=need - 1)
    create(-1, b"max_moves", mm=0)
    create(-1, b"max_moves", mm=128)
    create(-1, b"n_games", n=0)
    from reversi_alpha_zero_amd import _native as N
    assert lib.raz_analysis_create(e._h, 0, base, need, 2, 4, ctypes.byref(h)) == 0   # created, not started
    st = N.RazAnalysisStats()
    assert lib.raz_analysis_collect(h, None) == -4 and b"raz_analysis_start" in lib.raz_last_error()
    assert lib.raz_analysis_read(h, None, None, None, None) == -4 and b"raz_analysis_start" in lib.raz_last_error()
    assert lib.raz_analysis_stats_sync(h, ctypes.byref(st), None) == -4 and b"raz_analysis_start" in lib.raz_last_error()
    assert lib.raz_analysis_collect(None, None) == -1 and b"NULL" in lib.raz_last_error()
    moves = np.full((2, 4), -2, dtype=np.int8)
    one = np.zeros(2, dtype=np.uint64)
    assert lib.raz_analysis_start(h, None, None, None, None, 8, None) == -1 and b"NULL" in lib.raz_last_error()
    assert lib.raz_analysis_start(None, None, None, None, moves.ctypes.data, 8, None) == -1 and b"NULL" in lib.raz_last_error()
    assert lib.raz_analysis_start(h, one.ctypes.data, None, None, moves.ctypes.data, 8, None) == -1 and b"all or none" in lib.raz_last_error()
    assert lib.raz_analysis_start(h, one.ctypes.data, one.ctypes.data, None, moves.ctypes.data, 8, None) == -1 and b"all or none" in lib.raz_last_error()
    assert lib.raz_analysis_start(h, None, None, None, moves.ctypes.data, 0, None) == -1 and b"sims" in lib.raz_last_error()
    assert (view == 0x55).all(), "a refused call wrote into the workspace"
    assert (Emu.controls(e) == controls).all(), "a refused call touched the engine"
    lib.raz_analysis_destroy(h)


def test_emulated_analysis_ends_on_an_engine_error(blob):
    """Case 4: slots that end on an engine error (a node pool of 40 nodes that is never pruned) surface as the error word, their
    positions in state ERROR, and nothing stays pending: no loop spins."""
    from reversi_alpha_zero_amd.engine import analysis_error_text
    e = Emu.engine(M.engine_cfg(M.mini_config(1, sims=64)), blob, 6, 0, 64, nodes_per_game=40)
    an = Emu.analysis(e, 2, 2)
    an.start(*C.pack([_from(_mid(5, 24), 2), _from(_mid(6, 24), 1)], 2), 64)
    for _ in range(400):
        e.step(2)
        an.collect()
        st = an.stats()
        if not st["pending"]:
            break
    assert st["pending"] == 0 and st["failed"] >= 1 and st["failed"] + st["searched"] + st["solved"] == st["armed"] == 5, st
    assert st["error"] & 1 and "node pool full" in analysis_error_text(st["error"])
    evals = an.read()[2]
    bad = evals[evals["state"] == 4]
    assert len(bad) == st["failed"] and (bad["flags"] & 1).all() and (bad["n_top"] == 0).all()
    with pytest.raises(RuntimeError, match="error flags"):
        e.stats()
    an.check_guard()


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_collect_fails_a_position_whose_slot_left_the_one_move_protocol(blob, psn):
    """Case 7: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    C.case_slot_off_protocol(Emu, blob, psn)
