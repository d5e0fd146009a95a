"""GPU: the device league (include/raz.h raz_league_*, engine.DeviceLeague) and what is built on it - worker/league.py's LeagueWorker,
self_opt.start(archive_generations=True) - against an independent host driver and raz_match_*.  The cases and the guarded harness
around DeviceLeague are tests/league_cases.py's; the wave emulator runs them through the same product wrappers in
tests/test_league_emu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import league_cases as L
import match_cases as C
from test_match_gpu import DEV, Gpu, _self_opt_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blobs():
    return C.mini_blobs()


@pytest.fixture(scope="module")
def blobs3():
    return L.mini_blobs3()


@pytest.fixture(scope="module")
def positions257():
    return C.playout_positions(11, 257, 50)


@pytest.mark.parametrize("psn", [1, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_league_of_two_models_equals_the_match(blobs, positions257, n, psn):
    """Case 1: a two-model league with identity slots gives raz_match_*'s and the host driver's logs (who, action, all 64 root visit
    counts per ply) and results, on either side of a wave and of the 256-thread block."""
    L.case_equals_match(Gpu, blobs, n, psn, positions257[:n])


_runs = {}


def three_models(blobs3, psn):
    if psn not in _runs:
        _runs[psn] = L.case_three_models(Gpu, blobs3, psn)
    return _runs[psn]


@pytest.mark.parametrize("psn", [1, 4])
def test_league_of_three_models_on_scattered_slots(blobs3, psn):
    """Case 2."""
    three_models(blobs3, psn)


@pytest.mark.parametrize("psn", [1, 4])
def test_league_games_are_independent(blobs3, psn):
    """Case 3."""
    L.case_independence(Gpu, blobs3, *three_models(blobs3, psn))


@pytest.mark.parametrize("psn", [1, 4])
def test_league_bad_pairings(blobs3, psn):
    """Case 4."""
    L.case_bad_pairings(Gpu, blobs3, psn)


def test_league_refusals_and_edges(blobs3):
    """Case 5 on the device: the library's refusals by return code and message with no byte of the workspace written, DeviceLeague's
    own, and hand-offs that find no decided slot."""
    from reversi_alpha_zero_amd._native import lib
    from reversi_alpha_zero_amd.engine import DeviceLeague, DeviceNet, SelfPlayEngine, league_pairings
    cfg = C.engine_cfg(C.mini_config(4))
    engines = L.three_engines(Gpu, cfg, blobs3)()
    idle = SelfPlayEngine(cfg, DeviceNet(blobs3[1], DEV), 7, seed=1, sims_hint=8, max_plies=64, parts=1, single_stream=True)
    n = len(L.PAIRINGS)
    slots = (ctypes.c_uint32 * 3)(*L.SIZES)
    need = lib.raz_league_workspace_bytes(3, slots, n)
    assert need and lib.raz_league_workspace_bytes(1, slots, n) == 0 and lib.raz_league_workspace_bytes(17, slots, n) == 0
    assert lib.raz_league_workspace_bytes(3, slots, 0) == 0 and b"n_games" in lib.raz_last_error()
    mem = torch.full((need + 512,), 0x55, dtype=torch.uint8, device=DEV)
    base = (mem.data_ptr() + 255) // 256 * 256
    h = ctypes.c_void_p()

    def create(es, ws=base, nbytes=need, n_games=n, n_models=None):
        arr = (ctypes.c_void_p * 17)(*[e._h.value if e is not None else None for e in es])
        return lib.raz_league_create(arr, len(es) if n_models is None else n_models, ws, nbytes, n_games, ctypes.byref(h))
    a, b, c = engines
    for rc, text, args, kw in [(-1, b"NULL", ([a, None, c],), {}), (-1, b"NULL", ([a, b, c],), dict(ws=None)), (-1, b"n_models", ([a],), {}),
                               (-1, b"n_models", ([a, b, c],), dict(n_models=17)), (-1, b"n_games", ([a, b, c],), dict(n_games=0)),
                               (-1, b"twice", ([a, b, a],), {}), (-4, b"raz_engine_start", ([a, idle, c],), {}),
                               (-1, b"aligned", ([a, b, c],), dict(ws=base + 64)), (-1, b"smaller than", ([a, b, c],), dict(nbytes=need - 1))]:
        assert create(*args, **kw) == rc and text in lib.raz_last_error(), (kw, lib.raz_last_error())
    assert create([a, b, c]) == 0
    pr = torch.from_numpy(league_pairings(L.PAIRINGS).view(np.uint8).reshape(n, 16)).to(DEV)
    pos = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    pl = torch.ones(n, dtype=torch.uint8, device=DEV)
    sims, zero = (ctypes.c_uint32 * 3)(8, 8, 8), (ctypes.c_uint32 * 3)(8, 8, 0)
    assert lib.raz_league_turn(h, None) == -4 and b"raz_league_start" in lib.raz_last_error()
    assert lib.raz_league_read(h, None, None, None, None, None) == -4 and b"raz_league_start" in lib.raz_last_error()
    P, O = pr.data_ptr(), pos.data_ptr()
    for rc, text, args in [(-1, b"NULL", (h, None, None, None, None, sims, 1, None)), (-1, b"NULL", (h, P, None, None, None, None, 1, None)),
                           (-1, b"sims", (h, P, None, None, None, zero, 1, None)), (-1, b"all or none", (h, P, O, O, None, sims, 1, None)),
                           (-1, b"8-byte aligned", (h, P, O + 4, O, pl.data_ptr(), sims, 1, None))]:
        assert lib.raz_league_start(*args) == rc and text in lib.raz_last_error(), (args, lib.raz_last_error())
    torch.cuda.synchronize()
    assert bool((mem == 0x55).all()), "a refused call wrote to the workspace"
    lib.raz_league_destroy(h)
    # DeviceLeague's own refusals
    with pytest.raises(ValueError, match="engine of its own"):
        DeviceLeague([a, b, a])
    with pytest.raises(ValueError, match="2..16"):
        DeviceLeague([a])
    lg = Gpu.league(engines, n)
    with pytest.raises(RuntimeError, match="raz_league_start"):
        lg.w.turn()
    with pytest.raises(ValueError, match="CPU"):
        lg.w.start(pr.cpu(), sims=8)
    with pytest.raises(ValueError, match="CPU"):
        lg.w.start(pr, positions=(torch.zeros(n, dtype=torch.int64),) * 2 + (torch.ones(n, dtype=torch.uint8),), sims=8)
    with pytest.raises(ValueError, match="workspace"):
        DeviceLeague(engines, workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV)).start(pr, sims=8)
    with pytest.raises(RuntimeError, match="raz_engine_start"):
        DeviceLeague([a, idle, c]).start(pr, sims=8)
    # no decided slot: hand-offs change no byte of the workspace, before any step and with every search under way
    lg.start(L.PAIRINGS, C.playout_positions(2, n, 20), 8)
    before = lg.workspace()
    st = lg.stats()
    assert (st["live"], sum(st["searching"]), st["plies"], st["error"]) == (n, n, 0, 0)
    lg.turn()
    lg.turn()
    assert (lg.workspace() == before).all()
    for e in engines:
        e.step(1)
    lg.turn()
    assert (lg.workspace() == before).all() and lg.stats()["plies"] == 0
    lg.check_guard()


def test_league_ends_on_an_engine_error(blobs3):
    """Case 5: a slot's engine error (POOL_FULL: 40 nodes, never pruned - test_match_ends_on_an_engine_error's device, an engine error
    flag) becomes the league's error word, DeviceLeague.stats() raises with league_error_text, and the league has ended."""
    from reversi_alpha_zero_amd.engine import league_error_text
    cfg = C.engine_cfg(C.mini_config(1))
    engines = [Gpu.engine(cfg, blobs3[0], 3, 0, 8, nodes_per_game=40), Gpu.engine(cfg, blobs3[1], 2, 1, 8), Gpu.engine(cfg, blobs3[2], 2, 2, 8)]
    lg = Gpu.league(engines, 3)
    lg.start([(0, 2, 1, 0), (2, 1, 0, 0), (0, 1, 2, 0)], C.playout_positions(5, 3, 24), 8)
    for it in range(400):
        for e in engines:
            e.step(2)
        lg.turn()
        st = lg.stats()
        if not st["live"]:
            break
    assert st["live"] == 0 and sum(st["searching"]) == 0 and st["error"] & 1, st
    with pytest.raises(RuntimeError, match="node pool full") as err:
        lg.w.stats()
    assert str(err.value) == league_error_text(st["error"])
    games = lg.read()[0]
    assert (games["searching"] == 0).all() and (games["winner"] == 0).any()
    lg.check_guard()


@pytest.mark.parametrize("psn", [1, 4])
def test_league_ends_a_game_whose_slot_left_the_one_move_protocol(blobs3, psn):
    """Case 5: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    L.case_slot_off_protocol(Gpu, blobs3, psn)


def test_league_survives_set_parts_between_two_turns(blobs3):
    """Case 6: raz_engine_set_parts on one engine, through the engine wrapper, between two turns: the logs equal the run without it.
    (The descriptor does not change with that call; the re-upload itself is asserted on the emulator.)"""
    cfg = C.engine_cfg(C.mini_config(1))
    make = L.three_engines(Gpu, cfg, blobs3)
    positions = L.case2_positions()
    want = L.drive_league(Gpu, make, L.PAIRINGS, positions)
    got = L.drive_league(Gpu, make, L.PAIRINGS, positions, between=lambda engines, league: engines[1].set_parts(4))
    L.assert_same("set_parts between two turns", got, want)


# ---- worker level -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets3():
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return [ReversiNet(16, 1, 16).keras_init_(s).randomize_bn_(s + 1) for s in (1, 2, 3)]


def test_league_worker_equals_the_host_driver_and_is_reproducible(nets3, blobs3, tmp_path):
    """LeagueWorker on three mini models, games_per_pair 2: per-game results equal drive_host_league on the same schedule; the same
    seed twice writes identical JSON bytes; slots forcing two passes give the same per-game results as one pass."""
    from reversi_alpha_zero_amd.lib.rating import round_robin
    from reversi_alpha_zero_amd.worker.league import LeagueWorker
    config = C.mini_config(4)
    cfg, seed = C.engine_cfg(config), 3
    schedule, _ = round_robin(3, 2)
    pairings = [(g.black_model, g.black_slot, g.white_model, g.white_slot) for g in schedule]
    make = lambda: [Gpu.engine(cfg, blobs3[m], 4, 16 * seed + m, 8, first_game_id=0) for m in range(3)]
    want = L.drive_host_league(Gpu, make, pairings)
    a, b = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    w = LeagueWorker(config, nets3, games_per_pair=2, seed=seed, device=DEV)
    out = w.play(out_path=a, keep_games=True)
    assert w.last_results == want[1]
    assert [[(p["who"], p["action"]) for p in g["plies"]] for g in w.last_games] == [[(m, x) for m, x, _ in g] for g in want[0]]
    assert len(out["games"]) == 6 and out["elo"][0] == 0.0 and out["names"] == ["model_0", "model_1", "model_2"]
    assert np.array(out["wins"]).sum() + np.array(out["draws"]).sum() // 2 == 6 and out["games"][0]["moves"] == [x for _, x, _ in want[0][0]]
    LeagueWorker(config, nets3, games_per_pair=2, seed=seed, device=DEV).play(out_path=b, keep_games=True)
    assert open(a, "rb").read() == open(b, "rb").read()
    two = LeagueWorker(config, nets3, games_per_pair=2, seed=seed, device=DEV, slots=2)
    two.play()
    assert two.last_results == want[1]
    with pytest.raises(ValueError, match="whole rounds"):
        LeagueWorker(config, nets3, games_per_pair=2, slots=3)


def test_self_opt_archives_its_generations_and_the_league_rates_them(tmp_path, caplog, monkeypatch):
    """self_opt.start(evaluate=True, archive_generations=True) leaves generations/ holding the starting model and one directory per
    promotion, each loading to the blob that was promoted; league.start(cfg) rates them; archive_generations=False writes nothing."""
    import logging
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.data_helper import get_next_generation_model_dirs
    from reversi_alpha_zero_amd.worker import evaluate, league, optimize, self_opt
    cfg, best = _self_opt_config(tmp_path / "archived")
    rc = cfg.resource
    saved = {}   # challenger directory -> the blob the trainer saved there

    def remember(self, _f=optimize.OptimizeWorker.save_current_model):
        out = _f(self)
        r = self.config.resource
        d = get_next_generation_model_dirs(r)[-1]
        m = ReversiModel(self.config)
        assert m.load(os.path.join(d, r.next_generation_model_config_filename), os.path.join(d, r.next_generation_model_weight_filename))
        saved[os.path.basename(d)] = m.model.to_blob()
        return out
    monkeypatch.setattr(optimize.OptimizeWorker, "save_current_model", remember)
    monkeypatch.setattr(evaluate, "sleep", lambda s: pytest.fail("the in-process evaluation polls"))
    with caplog.at_level(logging.INFO, logger=self_opt.logger.name):
        self_opt.start(cfg, games_in_flight=16, backend="hip", total_blocks=2, seed=3, block_games=32, evaluate=True, archive_generations=True)
    decisions = [(r.getMessage()[len("evaluated "):].rsplit(": ", 1)) for r in caplog.records if r.getMessage().startswith("evaluated ")]
    promoted = [os.path.basename(d) for d, what in decisions if what == "new best model"]
    assert len(decisions) == len(saved) >= 1
    gen = os.path.join(rc.model_dir, "generations")
    assert sorted(os.listdir(gen)) == ["model_00000000-000000.000000"] + sorted(promoted)
    want = {"model_00000000-000000.000000": best.model.to_blob(), **{d: saved[d] for d in promoted}}
    for d, blob in want.items():
        m = ReversiModel(cfg)
        assert m.load(os.path.join(gen, d, rc.next_generation_model_config_filename), os.path.join(gen, d, rc.next_generation_model_weight_filename))
        assert m.model.to_blob() == blob, d
    # the league over the archive, in name order; the current best model - the LAST promotion by time, which with
    # eval.evaluate_latest_first need not be the last by name - is appended where it differs from the last archived one
    kept = saved[promoted[-1]] if promoted else best.model.to_blob()
    extra = [("best", kept)] if kept != want[sorted(want)[-1]] else []
    models, names = league.load_models(cfg)
    assert names == sorted(want) + [n for n, _ in extra]
    assert [m.model.to_blob() for m in models] == [want[d] for d in sorted(want)] + [b for _, b in extra]
    if len(models) < 2:   # (no promotion in this run: rate the starting model against a challenger saved by hand)
        other = ReversiModel(cfg)
        other.build(seed=9)
        self_opt.archive_generation(cfg, other, "model_20990101-000000.000000")
    out = league.start(cfg, games_per_pair=2, seed=1, device=DEV)
    assert len(out["elo"]) == len(out["names"]) >= 2 and out["elo"][0] == 0.0 and all(np.isfinite(out["elo"]))
    assert len(out["games"]) == len(out["names"]) * (len(out["names"]) - 1) and all(g["blacks"] + g["whites"] > 0 for g in out["games"])
    # archive_generations=False (the default): the directory does not exist
    saved.clear()
    cfg2, _ = _self_opt_config(tmp_path / "plain")
    self_opt.start(cfg2, games_in_flight=16, backend="hip", total_blocks=2, seed=3, block_games=32, evaluate=True)
    assert not os.path.exists(os.path.join(cfg2.resource.model_dir, "generations"))
