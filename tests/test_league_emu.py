"""CPU: the device league (include/raz.h raz_league_*, csrc/raz_league.h: k_league_claim, k_league_start, k_league_turn,
the bodies of the last two in csrc/raz_handoff.h) on the WAVE EMULATOR - the kernels as they stand, on host memory, driven through the
product's own wrappers (engine.SelfPlayEngine and engine.DeviceLeague on tests/emu_util.py's backend) - against an independent host driver (ReversiEnv objects and one set_position
call per ply on the mapped slot) and against raz_match_*.  The cases are tests/league_cases.py's; the device runs them in
tests/test_league_gpu.py."""
import ctypes

import numpy as np
import pytest

import league_cases as L
import match_cases as C
from emu_util import EmuEngine, aligned, load
from test_match_emu import Emu, match_of_65


@pytest.fixture(scope="module")
def blobs():
    return C.mini_blobs()


@pytest.fixture(scope="module")
def blobs3():
    return L.mini_blobs3()


@pytest.fixture(scope="module")
def late_positions():
    return C.playout_positions(11, 65, 50)   # test_match_emu.py's


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_of_two_models_equals_the_match_one_game(blobs, psn):
    """Case 1, n = 1."""
    L.case_equals_match(Emu, blobs, 1, psn, C.playout_positions(12, 1, 50))


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_of_two_models_equals_the_match_65_games(blobs, late_positions, psn):
    """Case 1, n = 65 (a second wave of the one-thread-per-game kernels): the logs (who, action, all 64 root visit counts per ply) and
    results of a two-model league with identity slots are raz_match_*'s and the host driver's."""
    _, _, want_host, want_match = match_of_65(blobs, late_positions, psn)
    L.case_equals_match(Emu, blobs, 65, psn, late_positions, want_match=want_match, want_host=want_host)


_runs = {}


def three_models(blobs3, psn):
    if psn not in _runs:
        _runs[psn] = L.case_three_models(Emu, blobs3, psn)
    return _runs[psn]


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_of_three_models_on_scattered_slots(blobs3, psn):
    """Case 2: engines of 5, 7 and 9 slots, 9 games on slots out of order, a pass, white to move, a last square, an end with empty
    squares and a resignation at once - each asserted present in the host driver's logs first; unused slots byte-identical."""
    three_models(blobs3, psn)


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_games_are_independent(blobs3, psn):
    """Case 3: a game alone, a hand-off every 16 steps, the pairing array permuted."""
    L.case_independence(Emu, blobs3, *three_models(blobs3, psn))


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_bad_pairings(blobs3, psn):
    """Case 4."""
    L.case_bad_pairings(Emu, blobs3, psn)


def test_emulated_league_refusals(blobs3):
    """Case 5: every refusal by return code and message, with no byte of the workspace written."""
    lib = load()
    cfg = C.engine_cfg(C.mini_config(1))
    a, b, c = (Emu.engine(cfg, blobs3[m], n, m, 8) for m, n in enumerate((2, 3, 4)))
    idle = EmuEngine(cfg, blobs3[1], 2, seed=1, sims_hint=8, max_plies=64)   # created, not started
    slots = (ctypes.c_uint32 * 16)(*([2, 3, 4] + [1] * 13))
    need = lib.raz_league_workspace_bytes(3, slots, 5)
    assert need > 0 and need % 256 == 0
    for bad_m in (0, 1, 17):
        assert lib.raz_league_workspace_bytes(bad_m, slots, 5) == 0 and b"n_models" in lib.raz_last_error()
    assert lib.raz_league_workspace_bytes(3, slots, 0) == 0 and b"n_games" in lib.raz_last_error()
    assert lib.raz_league_workspace_bytes(16, slots, 1) > 0
    # the sections: stats, 3 descriptors, 5 pairings, 5 games, the log, 9 claim words, the visit counts
    assert need >= 128 + 5 * (16 + 32 + 64 * 4 + 64 * 256) + 9 * 4
    mem, base = aligned(need + 512)
    view = np.ctypeslib.as_array((ctypes.c_uint8 * (need + 512)).from_address(base))
    view[:] = 0x55
    h = ctypes.c_void_p()

    def create(engines, n_models=None, ws=base, nbytes=need, n_games=5, out=True):
        arr = (ctypes.c_void_p * 17)(*[e._h.value if e is not None else None for e in engines]) if engines is not None else None
        return lib.raz_league_create(arr, len(engines) if n_models is None else n_models, ws, nbytes, n_games, ctypes.byref(h) if out else None)
    for rc, text, kw in [(-1, b"NULL", dict(engines=None, n_models=3)), (-1, b"NULL", dict(engines=[a, b, c], ws=None)),
                         (-1, b"NULL", dict(engines=[a, b, c], out=False)), (-1, b"NULL", dict(engines=[a, None, c])),
                         (-1, b"n_models", dict(engines=[a])), (-1, b"n_models", dict(engines=[a, b, c], n_models=17)),
                         (-1, b"n_games", dict(engines=[a, b, c], n_games=0)), (-1, b"twice", dict(engines=[a, b, a])),
                         (-4, b"raz_engine_start", dict(engines=[a, idle, c])), (-1, b"aligned", dict(engines=[a, b, c], ws=base + 64)),
                         (-1, b"smaller than raz_league_workspace_bytes", dict(engines=[a, b, c], nbytes=need - 1))]:
        assert create(**kw) == rc and text in lib.raz_last_error(), (kw, lib.raz_last_error())
    assert create([a, b, c]) == 0
    from reversi_alpha_zero_amd import _native as N
    st = N.RazLeagueStats()
    assert lib.raz_league_turn(h, None) == -4 and b"raz_league_start" in lib.raz_last_error()
    assert lib.raz_league_stats_sync(h, ctypes.byref(st), None) == -4 and b"raz_league_start" in lib.raz_last_error()
    assert lib.raz_league_read(h, None, None, None, None, None) == -4 and b"raz_league_start" in lib.raz_last_error()
    assert lib.raz_league_turn(None, None) == -1 and b"NULL" in lib.raz_last_error()
    from reversi_alpha_zero_amd.engine import league_pairings
    pr = league_pairings([(0, 0, 1, 0), (1, 1, 2, 0), (2, 1, 0, 1), (1, 2, 2, 2), (2, 3, 1, 0)])
    sims, zero = (ctypes.c_uint32 * 3)(8, 8, 8), (ctypes.c_uint32 * 3)(8, 0, 8)
    one = np.zeros(6, dtype=np.uint64)
    pl = np.ones(5, dtype=np.uint8)
    P, O = pr.ctypes.data, one.ctypes.data
    for rc, text, args in [(-1, b"NULL", (None, P, None, None, None, sims, 1, None)), (-1, b"NULL", (h, None, None, None, None, sims, 1, None)),
                           (-1, b"NULL", (h, P, None, None, None, None, 1, None)), (-1, b"sims", (h, P, None, None, None, zero, 1, None)),
                           (-1, b"all or none", (h, P, O, None, None, sims, 1, None)), (-1, b"all or none", (h, P, O, O, None, sims, 1, None)),
                           (-1, b"8-byte aligned", (h, P, O + 4, O, pl.ctypes.data, sims, 1, None))]:
        assert lib.raz_league_start(*args) == rc and text in lib.raz_last_error(), (args, lib.raz_last_error())
    assert (view == 0x55).all(), "a refused call wrote to the workspace"
    assert lib.raz_league_start(h, P, None, None, None, sims, 1, None) == 0
    assert not (view[:need] == 0x55).all() and (view[need:] == 0x55).all()
    lib.raz_league_destroy(h)


def test_emulated_league_turn_without_a_decided_slot_changes_nothing(blobs3):
    """Case 5: raz_league_turn before any engine step, and with every search under way, leaves the workspace as it was, byte for byte."""
    cfg = C.engine_cfg(C.mini_config(4))
    engines = L.three_engines(Emu, cfg, blobs3)()
    lg = Emu.league(engines, len(L.PAIRINGS))
    lg.start(L.PAIRINGS, C.playout_positions(2, len(L.PAIRINGS), 20), 8)
    before = lg.workspace()
    games = lg.read()[0]
    assert (games["searching"] == games["player"]).all() and lg.stats()["live"] == len(L.PAIRINGS)
    for _ in range(3):
        lg.turn()
    assert (lg.workspace() == before).all()
    for e in engines:
        e.step(1)   # mid-search slots (8 simulations take more than one step) are left alone too
    lg.turn()
    assert (lg.workspace() == before).all() and lg.stats()["plies"] == 0
    lg.check_guard()


def test_emulated_league_ends_on_an_engine_error(blobs3):
    """Case 5: a node pool of 40 nodes that is never pruned (test_match_emu.py's device): the slot's POOL_FULL flag becomes the
    league's error word and the league reaches live == 0."""
    from reversi_alpha_zero_amd.engine import league_error_text
    cfg = C.engine_cfg(C.mini_config(1))
    engines = [Emu.engine(cfg, blobs3[0], 3, 0, 8, nodes_per_game=40), Emu.engine(cfg, blobs3[1], 2, 1, 8), Emu.engine(cfg, blobs3[2], 2, 2, 8)]
    lg = Emu.league(engines, 3)
    lg.start([(0, 2, 1, 0), (2, 1, 0, 0), (0, 1, 2, 0)], C.playout_positions(5, 3, 24), 8)
    for it in range(400):
        for e in engines:
            e.step(2)
        lg.turn()
        st = lg.stats()
        if not st["live"]:
            break
    assert st["live"] == 0 and sum(st["searching"]) == 0, st
    assert st["error"] & 1 and "node pool full" in league_error_text(st["error"])
    games = lg.read()[0]
    assert (games["searching"] == 0).all() and (games["winner"] == 0).any()
    lg.check_guard()


def test_emulated_league_uploads_a_changed_descriptor_again(blobs3):
    """Case 6 on the emulator.  raz_engine_set_parts changes no field of an engine's descriptor here (it changes how the host steps
    the batch), so the logs of a league with that call in its middle equal the logs without it - and the re-upload itself is
    asserted with the one call that does change a descriptor field, raz_engine_set_solver_pool_every: after it, and only after it,
    a hand-off that finds no decided slot changes bytes of the workspace, and all of them lie in the descriptor table."""
    cfg = C.engine_cfg(C.mini_config(1))
    make = L.three_engines(Emu, cfg, blobs3)
    positions = L.case2_positions()

    def set_parts(engines, league):
        engines[1].backend.call("raz_engine_set_parts", engines[1]._h, 4)
    L.assert_same("set_parts between two turns", L.drive_league(Emu, make, L.PAIRINGS, positions, between=set_parts),
                  L.drive_league(Emu, make, L.PAIRINGS, positions))
    engines = make()
    lg = Emu.league(engines, len(L.PAIRINGS))
    lg.start(L.PAIRINGS, positions, 8)
    lg.turn()
    before = lg.workspace()
    lib, changed = engines[2].lib, None
    for every in (1, 2):   # one of the two differs from the engine's present setting
        assert lib.raz_engine_set_solver_pool_every(engines[2]._h, every) == 0
        lg.turn()
        now = lg.workspace()
        if (now != before).any():
            changed = np.flatnonzero(now != before)
            break
    assert changed is not None, "the descriptor table was not uploaded again"
    # the table lies between the 256-byte stats section and the pairings
    from reversi_alpha_zero_amd.engine import league_pairings
    kept = before.tobytes().find(league_pairings(L.PAIRINGS).tobytes())
    assert kept > 256 and 256 <= changed.min() and changed.max() < kept
    lg.turn()
    assert (lg.workspace() == now).all()   # uploaded once, not on every turn
    lg.check_guard()


@pytest.mark.parametrize("psn", [1, 4])
def test_emulated_league_ends_a_game_whose_slot_left_the_one_move_protocol(blobs3, psn):
    """Case 5: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    L.case_slot_off_protocol(Emu, blobs3, psn)
