"""CPU: the device hand-off between two engines (include/raz.h raz_match_*, csrc/raz_match.h: k_match_start, k_match_turn, their
bodies in csrc/raz_handoff.h) on the
WAVE EMULATOR - the kernels as they stand, on host memory, driven through the product's own wrappers (engine.SelfPlayEngine and
engine.DeviceMatch on tests/emu_util.py's backend) - against an independent host driver (ReversiEnv objects and one set_position call per ply) and the golden games of the unmodified reference's
evaluator.  The cases are tests/match_cases.py's; the device runs them in tests/test_match_gpu.py."""
import ctypes

import numpy as np
import pytest

import match_cases as C
from emu_util import EmuEngine, aligned, load


Emu = C.Adapter("cpu", EmuEngine)   # the emulator's instance of the cases' backend: the product's wrappers on host memory


@pytest.fixture(scope="module")
def blobs():
    return C.mini_blobs()


@pytest.fixture(scope="module")
def late_positions():
    """65 positions 14 plies from a full board, a playout each: a whole match of 65 in the seconds a CPU has."""
    return C.playout_positions(11, 65, 50)


_runs = {}


def match_of_65(blobs, late_positions, psn):
    """The host driver's and the match's 65 games at parallel_search_num `psn`, played once for the tests that look at them."""
    if psn not in _runs:
        cfg = C.engine_cfg(C.mini_config(psn, use_solver_turn=0, use_solver_turn_in_simulation=0))
        bib = [(g * 7 // 3) % 2 == 0 for g in range(65)]
        args = (Emu, cfg, blobs, 65, 9, 300, 8, bib, late_positions)
        _runs[psn] = (cfg, bib, C.drive_host(*args), C.drive_match(*args, guard=4096))
    return _runs[psn]


@pytest.mark.parametrize("name", ["eval_as_shipped", "eval_par1_resign_nosolver", "eval_par4_sections_disagree"])
def test_emulated_match_replays_the_reference_evaluate_games(name):
    """Case 1: the three matches of tests/golden/eval_games.json through raz_match_*: movers, actions (resignations included), root
    visit counts where the fixture has them, ng_win and the final disc counts are the unmodified reference's."""
    gold = C.golden()
    C.case_golden(Emu, next(m for m in gold["matches"] if m["name"] == name), C.golden_blobs(gold))


@pytest.mark.parametrize("psn", [1, 4])
@pytest.mark.parametrize("n", [1, 2])
def test_emulated_match_equals_the_host_driver_whole_games(blobs, n, psn):
    """Case 2, 1 and 2 games from the initial position at 8 simulations a move (end-game solver at the root and in the simulations
    as the eval section ships it)."""
    cfg = C.engine_cfg(C.mini_config(psn))
    args = (Emu, cfg, blobs, n, 4, 20, 8, [False, True][:n])
    C.assert_same((n, psn), C.drive_match(*args), C.drive_host(*args))


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_match_of_65_equals_the_host_driver(blobs, late_positions, psn):
    """Case 2, 65 games (a second wave of one-thread-per-game kernels), from positions 14 plies before a full board."""
    _, _, want, got = match_of_65(blobs, late_positions, psn)
    C.assert_same(("65", psn), got, want)


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_match_start_positions(blobs, psn):
    """Case 3: a pass (the same slot is armed again), white to move, a single empty square, an end with empty squares, and a
    resignation at once - each asserted present in the host driver's logs before a match kernel is looked at."""
    C.case_start_positions(Emu, blobs, psn)


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_match_games_are_independent(blobs, late_positions, psn):
    """Case 4: game g's log is the same played alone as it is as game g of 65, and the same with a hand-off after every engine step
    as with one after every 16."""
    cfg, bib, want, _ = match_of_65(blobs, late_positions, psn)
    for g in (0, 37, 64):
        alone = C.drive_match(Emu, cfg, blobs, 1, 9, 300 + g, 8, [bib[g]], [late_positions[g]], step=1, turn_every=1)
        C.assert_same(("alone", g), alone, ([want[0][g]], [want[1][g]]))
    five = list(range(30, 35))
    args = (Emu, cfg, blobs, 5, 9, 330, 8, [bib[g] for g in five], [late_positions[g] for g in five])
    sparse = C.drive_match(*args, step=1, turn_every=16)
    C.assert_same("a hand-off every 16 steps", sparse, ([want[0][g] for g in five], [want[1][g] for g in five]))


def test_emulated_match_refusals_and_edges(blobs):
    """Case 5."""
    lib = load()
    cfg = C.engine_cfg(C.mini_config(1))
    a, b, c = Emu.engine(cfg, blobs[0], 2, 0, 8), Emu.engine(cfg, blobs[1], 2, 1, 8), Emu.engine(cfg, blobs[1], 3, 1, 8)
    idle = EmuEngine(cfg, blobs[1], 2, seed=1, sims_hint=8, max_plies=64)   # created, not started

    h = ctypes.c_void_p()
    mem, base = aligned(lib.raz_match_workspace_bytes(2) + 64)

    def refused(code, text, x, y, workspace_bytes=lib.raz_match_workspace_bytes(2)):
        assert lib.raz_match_create(x._h, y._h, base, workspace_bytes, ctypes.byref(h)) == code and text in lib.raz_last_error(), lib.raz_last_error()
    refused(-1, b"differ in n_games", a, c)
    refused(-4, b"raz_engine_start", a, idle)
    refused(-1, b"smaller than raz_match_workspace_bytes", a, b, workspace_bytes=lib.raz_match_workspace_bytes(2) - 1)
    assert lib.raz_match_create(a._h, b._h, base + 64, lib.raz_match_workspace_bytes(2), ctypes.byref(h)) == -1 and b"aligned" in lib.raz_last_error()
    assert lib.raz_match_create(a._h, None, base, lib.raz_match_workspace_bytes(2), ctypes.byref(h)) == -1 and b"NULL" in lib.raz_last_error()
    assert lib.raz_match_workspace_bytes(0) == 0
    assert lib.raz_match_workspace_bytes(65) - lib.raz_match_workspace_bytes(1) >= 64 * (32 + 64 * 4 + 64 * 256)
    m = Emu.match(a, b)
    assert lib.raz_match_turn(m.w._h, None) == -4 and b"raz_match_start" in lib.raz_last_error()
    bib = np.array([1, 0], dtype=np.uint8)
    one = np.zeros(2, dtype=np.uint64)
    assert lib.raz_match_start(m.w._h, bib.ctypes.data, one.ctypes.data, None, None, 8, 8, 1, None) == -1 and b"all or none" in lib.raz_last_error()
    assert lib.raz_match_start(m.w._h, bib.ctypes.data, None, None, None, 0, 8, 1, None) == -1 and b"sims" in lib.raz_last_error()
    # no decided slot: a hand-off changes no byte of the workspace (nor of the engines' control blocks)
    m.start([1, 0], None, 8, 8)
    before = m.workspace()
    st = m.stats()
    assert (st["live"], st["searching_best"], st["searching_challenger"], st["plies"], st["error"]) == (2, 1, 1, 0, 0)
    m.turn()
    assert (before == m.workspace()).all()
    m.check_guard()


def test_emulated_match_turn_without_a_decided_slot_changes_nothing(blobs):
    """Case 5: raz_match_turn before any engine step - every armed slot is in phase NEW_MOVE - leaves the workspace as it was,
    byte for byte, and writes nothing behind it."""
    cfg = C.engine_cfg(C.mini_config(4))
    a, b = Emu.engine(cfg, blobs[0], 65, 0, 8), Emu.engine(cfg, blobs[1], 65, 1, 8)
    m = Emu.match(a, b)
    m.start([g % 2 for g in range(65)], C.playout_positions(2, 65, 20), 8, 8)
    before = m.workspace()
    games = m.read()[0]
    assert (games["searching"] == [1 + int((p == 1) != bool(g % 2)) for g, p in enumerate(games["player"])]).all()
    for _ in range(3):
        m.turn()
    assert (m.workspace() == before).all()
    a.step(1)   # mid-search slots (8 simulations take more than one step) are left alone too
    b.step(1)
    m.turn()
    assert (m.workspace() == before).all() and m.stats()["plies"] == 0
    m.check_guard()


def test_emulated_match_ends_on_an_engine_error(blobs):
    """Case 5: a slot that ends on an engine error surfaces as the match's error word, and the match ENDS instead of waiting for a
    move that never comes.  The engine error here is POOL_FULL (a node pool of 40 nodes that is never pruned): RECORDS_FULL cannot be produced in a match -
    raz_engine_create refuses max_plies below 64 (asserted), and arming a slot for one move resets its record count."""
    from reversi_alpha_zero_amd.engine import match_error_text
    cfg = C.engine_cfg(C.mini_config(1))
    with pytest.raises(ValueError, match="max_plies"):
        EmuEngine(cfg, blobs[0], 2, seed=0, sims_hint=8, max_plies=1)
    a = Emu.engine(cfg, blobs[0], 3, 0, 8, nodes_per_game=40)
    b = Emu.engine(cfg, blobs[1], 3, 1, 8)
    m = Emu.match(a, b)
    m.start([1, 0, 1], C.playout_positions(5, 3, 24), 8, 8)
    for it in range(400):
        a.step(2)
        b.step(2)
        m.turn()
        st = m.stats()
        if not st["live"]:
            break
    assert st["live"] == 0 and st["searching_best"] == 0 and st["searching_challenger"] == 0, st
    assert st["error"] & 1 and "node pool full" in match_error_text(st["error"])
    games = m.read()[0]
    assert (games["searching"] == 0).all() and (games["winner"] == 0).any()   # ended, some of them undecided
    with pytest.raises(RuntimeError, match="error flags"):
        a.stats()
    m.check_guard()


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_match_ends_a_game_whose_slot_left_the_one_move_protocol(blobs, psn):
    """Case 7: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    C.case_slot_off_protocol(Emu, blobs, psn)
