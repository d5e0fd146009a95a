"""GPU: the device hand-off between two engines (include/raz.h raz_match_*, engine.DeviceMatch) and what is built on it -
EvaluateWorker(handoff="device"), self_opt.start(evaluate=True) - against the host route, an independent host driver and the golden
games of the unmodified reference's evaluator.  The cases and the guarded harness around DeviceMatch are tests/match_cases.py's; the
wave emulator runs them through the same product wrappers in tests/test_match_emu.py."""
import hashlib
import logging
import os

import numpy as np
import pytest
import torch

import match_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = C.GUARD


def _engine(cfg, blob, n, **kw):
    from reversi_alpha_zero_amd.engine import DeviceNet, SelfPlayEngine
    return SelfPlayEngine(cfg, DeviceNet(blob, DEV), n, parts=1, single_stream=True, record_root_w=True, **kw)


Gpu = C.Adapter(DEV, _engine)   # the device's instance of the cases' backend


@pytest.fixture(scope="module")
def blobs():
    return C.mini_blobs()


@pytest.fixture(scope="module")
def nets():
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return [ReversiNet(16, 1, 16).keras_init_(s).randomize_bn_(s + 1) for s in (1, 2)]


def _same_games(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["game_id"], x["best_is_black"]) == (y["game_id"], y["best_is_black"])
        assert [(p["who"], p["action"]) for p in x["plies"]] == [(p["who"], p["action"]) for p in y["plies"]], x["game_id"]
        for i, (p, q) in enumerate(zip(x["plies"], y["plies"])):
            assert np.array_equal(np.asarray(p["root_n"]).astype(np.int64), np.asarray(q["root_n"]).astype(np.int64)), (x["game_id"], i)


def test_evaluate_worker_device_handoff_equals_the_reference_evaluate_games():
    """Case 1: tests/golden/eval_games.json through EvaluateWorker(handoff="device") - the comparison of
    test_evaluate_worker_matches_equal_the_reference_evaluate_games (tests/test_engine_gpu.py) on the other route."""
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.worker.evaluate import EvaluateWorker
    gold = C.golden()
    nets = []
    for meta in gold["nets"]:
        net = ReversiNet(meta["filters"], meta["res_layers"], meta["value_fc"]).keras_init_(meta["keras_init_seed"]).randomize_bn_(meta["randomize_bn_seed"])
        assert hashlib.sha256(net.to_blob()).hexdigest() == meta["blob_sha256"], "seeded net init is not reproducible"
        nets.append(net)
    for m in gold["matches"]:
        cfg = Config()
        cfg.eval.play_config.update(m["resolved_play_config"])
        cfg.play.update(m["resolved_config_play"])
        w = EvaluateWorker(cfg, seed=m["seed"], device=DEV, handoff="device")
        w.games_played = m["first_game_id"]
        results = w.play_games(nets[0], nets[1], len(m["games"]))
        assert [g["game_id"] for g in w.last_games] == [g["game_id"] for g in m["games"]]
        plies = [[(p["who"], p["action"], [int(x) for x in p["root_n"]]) for p in g["plies"]] for g in w.last_games]
        C.check_against_golden(m, plies, results)


@pytest.mark.parametrize("psn", [1, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_handoff_equals_host_handoff(nets, n, psn):
    """Case 2: the same match by both routes of EvaluateWorker on the mini net at 8 simulations a move: identical last_games and
    results, on either side of a wave (64) and of a 256-thread workgroup."""
    from reversi_alpha_zero_amd.worker.evaluate import EvaluateWorker
    cfg = C.mini_config(psn)
    out = {}
    for route in ("host", "device"):
        w = EvaluateWorker(cfg, seed=13, device=DEV, handoff=route)
        w.games_played = 1000
        out[route] = (w.play_games(nets[0], nets[1], n), w.last_games)
    assert [tuple(r) for r in out["device"][0]] == [tuple(r) for r in out["host"][0]]
    assert n == 1 or {r[1] for r in out["host"][0]} == {True, False}
    _same_games(out["device"][1], out["host"][1])
    assert all(len(g["plies"]) >= 9 for g in out["host"][1])


@pytest.mark.parametrize("psn", [1, 4])
def test_match_start_positions(blobs, psn):
    """Case 3 (a pass, white to move, a last square, an end with empty squares, a resignation at once) through DeviceMatch's
    positions=."""
    C.case_start_positions(Gpu, blobs, psn)


@pytest.mark.parametrize("psn", [1, 4])
def test_match_games_are_independent(blobs, psn):
    """Case 4: alone or as game g of 65; a hand-off after every engine step or after every 16."""
    cfg = C.engine_cfg(C.mini_config(psn))
    pos = C.playout_positions(11, 65, 40)
    bib = [(g * 7 // 3) % 2 == 0 for g in range(65)]
    want = C.drive_host(Gpu, cfg, blobs, 65, 9, 300, 8, bib, pos)
    C.assert_same("65", C.drive_match(Gpu, cfg, blobs, 65, 9, 300, 8, bib, pos, step=4, guard=GUARD), want)
    for g in (0, 37, 64):
        alone = C.drive_match(Gpu, cfg, blobs, 1, 9, 300 + g, 8, [bib[g]], [pos[g]], step=1, turn_every=1, guard=GUARD)
        C.assert_same(("alone", g), alone, ([want[0][g]], [want[1][g]]))
    sparse = C.drive_match(Gpu, cfg, blobs, 65, 9, 300, 8, bib, pos, step=1, turn_every=16, guard=GUARD)
    C.assert_same("a hand-off every 16 steps", sparse, want)


def test_match_refusals_and_edges(blobs):
    """Case 5 on the device, through DeviceMatch."""
    from reversi_alpha_zero_amd._native import lib
    from reversi_alpha_zero_amd.engine import DeviceMatch, DeviceNet, SelfPlayEngine
    cfg = C.engine_cfg(C.mini_config(4))
    a, b, c = Gpu.engine(cfg, blobs[0], 65, 0, 8), Gpu.engine(cfg, blobs[1], 65, 1, 8), Gpu.engine(cfg, blobs[1], 64, 1, 8)
    with pytest.raises(ValueError, match="same n_games"):
        DeviceMatch(a, c)
    idle = SelfPlayEngine(cfg, DeviceNet(blobs[1], DEV), 65, seed=1, sims_hint=8, max_plies=64, parts=1, single_stream=True)
    with pytest.raises(RuntimeError, match="raz_engine_start"):
        DeviceMatch(a, idle)
    with pytest.raises(ValueError, match="workspace"):
        DeviceMatch(a, b, workspace=torch.zeros(lib.raz_match_workspace_bytes(65) - 1, dtype=torch.uint8, device=DEV))
    m = Gpu.match(a, b)
    bib = torch.tensor([g % 2 for g in range(65)], dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="CPU"):
        m.w.start(bib.cpu(), sims_best=8)
    with pytest.raises(ValueError, match="CPU"):
        m.w.start(bib, positions=(torch.zeros(65, dtype=torch.int64),) * 2 + (torch.ones(65, dtype=torch.uint8),), sims_best=8)
    with pytest.raises(RuntimeError, match="raz_match_start"):
        m.w.turn()
    # no decided slot: hand-offs change no byte of the workspace, before any step and with every search under way
    m.start([g % 2 for g in range(65)], C.playout_positions(2, 65, 20), 8, 8)
    before = m.workspace()
    st = m.stats()
    assert (st["live"], st["searching_best"] + st["searching_challenger"], st["plies"], st["error"]) == (65, 65, 0, 0)
    m.turn()
    m.turn()
    assert (m.workspace() == before).all()
    a.step(1)
    b.step(1)
    m.turn()
    assert (m.workspace() == before).all() and m.stats()["plies"] == 0
    m.check_guard()


def test_match_ends_on_an_engine_error(blobs):
    """Case 5: a slot's engine error (POOL_FULL: 40 nodes, never pruned - tests/test_match_emu.py says why not RECORDS_FULL) becomes the
    match's error word, DeviceMatch.stats() raises on it, and the match has ended."""
    from reversi_alpha_zero_amd.engine import DeviceMatch
    cfg = C.engine_cfg(C.mini_config(1))
    a, b = Gpu.engine(cfg, blobs[0], 3, 0, 8, nodes_per_game=40), Gpu.engine(cfg, blobs[1], 3, 1, 8)
    m = Gpu.match(a, b)
    m.start([1, 0, 1], C.playout_positions(5, 3, 24), 8, 8)
    for it in range(400):
        a.step(2)
        b.step(2)
        m.turn()
        st = m.stats()
        if not st["live"]:
            break
    assert st["live"] == 0 and st["searching_best"] == 0 and st["searching_challenger"] == 0 and st["error"] & 1, st
    with pytest.raises(RuntimeError, match="node pool full"):
        m.w.stats()
    games = m.read()[0]
    assert (games["searching"] == 0).all() and (games["winner"] == 0).any()
    m.check_guard()


@pytest.mark.parametrize("psn", [1, 4])
def test_match_ends_a_game_whose_slot_left_the_one_move_protocol(blobs, psn):
    """Case 7: ERR_SLOT, the branch of the shared rule (csrc/raz_handoff.h slot_answer) no engine error reaches."""
    C.case_slot_off_protocol(Gpu, blobs, psn)


def test_device_handoff_makes_no_per_game_host_call(nets, monkeypatch):
    """Case 6: during play_games the device route calls neither set_position / set_positions nor pack_records on either engine (the
    host route, counted the same way, calls them once per ply and once per round)."""
    from reversi_alpha_zero_amd.engine import SelfPlayEngine
    from reversi_alpha_zero_amd.worker.evaluate import EvaluateWorker
    calls = {}
    for name in ("set_position", "set_positions", "pack_records"):
        def counted(self, *a, _f=getattr(SelfPlayEngine, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(SelfPlayEngine, name, counted)
    cfg = C.mini_config(4)
    w = EvaluateWorker(cfg, seed=2, device=DEV, handoff="device")
    res = w.play_games(nets[0], nets[1], 6)
    assert len(res) == 6 and calls == {}
    w = EvaluateWorker(cfg, seed=2, device=DEV, handoff="host")
    assert [tuple(r) for r in w.play_games(nets[0], nets[1], 6)] == [tuple(r) for r in res]
    assert calls["set_position"] == sum(len(g["plies"]) for g in w.last_games) and calls["pack_records"] > 0


# ---- worker level -------------------------------------------------------------------------------------------------------------
def _eval_config(root):
    """The configuration of test_evaluate_worker_batched_match (tests/test_engine_gpu.py): 6 games at 8 simulations."""
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.model_helpler import save_as_best_model
    cfg = Config()
    cfg.model.update(dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16))
    rc = cfg.resource
    rc.model_dir = str(root / "model")
    rc.model_best_config_path = str(root / "model" / "model_best_config.json")
    rc.model_best_weight_path = str(root / "model" / "model_best_weight.h5")
    rc.next_generation_model_dir = str(root / "model" / "next_generation")
    os.makedirs(rc.next_generation_model_dir)
    cfg.eval.game_num = 6
    cfg.eval.play_config.simulation_num_per_move = 8
    best = ReversiModel(cfg)
    best.build(seed=1)
    save_as_best_model(best)
    ng = ReversiModel(cfg)
    ng.build(seed=2)
    d = os.path.join(rc.next_generation_model_dir, rc.next_generation_model_dirname_tmpl % "20260101-000000.000000")
    os.makedirs(d)
    ng.save(os.path.join(d, rc.next_generation_model_config_filename), os.path.join(d, rc.next_generation_model_weight_filename))
    return cfg, best, ng, d


def test_evaluate_worker_device_handoff_consumes_the_challenger(tmp_path):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.worker.evaluate import EvaluateWorker, decide
    cfg, best, ng, model_dir = _eval_config(tmp_path)
    w = EvaluateWorker(cfg, seed=11, device=DEV, handoff="device")
    assert w.start(max_models=1) == 1
    assert not os.path.exists(model_dir)
    kept = ReversiModel(cfg)
    assert kept.load(cfg.resource.model_best_config_path, cfg.resource.model_best_weight_path)
    better, played, rate = decide([r[0] for r in w.last_results] + [None] * 6, 6, cfg.eval.replace_rate)
    assert len(w.last_results) == played and kept.model.to_blob() == (ng.model.to_blob() if better else best.model.to_blob())
    host = EvaluateWorker(cfg, seed=11, device=DEV, handoff="host")
    assert [tuple(r) for r in host.play_games(best, ng, 6)][:played] == [tuple(r) for r in w.last_results]
    with pytest.raises(ValueError, match="handoff"):
        EvaluateWorker(cfg, handoff="gpu")


def _self_opt_config(root):
    """tests/test_replay_loop_gpu.py's configuration of self_opt, with eval.game_num 6 at 8 simulations."""
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.model_helpler import save_as_best_model
    cfg = Config()
    cfg.model.update(dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16))
    rc, d = cfg.resource, str(root)
    rc.project_dir = rc.data_dir = d
    rc.model_dir = os.path.join(d, "model")
    rc.model_best_config_path = os.path.join(rc.model_dir, "model_best_config.json")
    rc.model_best_weight_path = os.path.join(rc.model_dir, "model_best_weight.h5")
    rc.next_generation_model_dir = os.path.join(rc.model_dir, "next_generation")
    rc.play_data_dir = os.path.join(d, "play_data")
    rc.self_play_ggf_data_dir = os.path.join(d, "ggf")
    rc.log_dir = os.path.join(d, "logs")
    rc.force_simulation_num_file = os.path.join(d, ".force-sim")
    rc.force_learing_rate_file = os.path.join(d, ".force-lr")
    rc.self_play_game_idx_file = os.path.join(d, ".self-play-game-idx")
    cfg.play.schedule_of_simulation_num_per_move = [(0, 8)]
    cfg.play.update(dict(parallel_search_num=1, use_solver_turn=0, use_solver_turn_in_simulation=0, thinking_loop=1,
                         required_visit_to_decide_action=8))
    cfg.play_data.update(dict(nb_game_in_file=8, enable_ggf_data=False, max_file_num=1000))
    cfg.trainer.update(dict(batch_size=2048, min_data_size_to_learn=100, save_model_steps=10, wait_after_save_model_ratio=0,
                            epoch_to_checkpoint=1))
    cfg.eval.game_num = 6
    cfg.eval.play_config.simulation_num_per_move = 8
    rc.create_directories()
    best = ReversiModel(cfg)
    best.build(seed=5)
    save_as_best_model(best)
    return cfg, best


def test_self_opt_evaluates_its_challengers_in_process(tmp_path, caplog, monkeypatch):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.data_helper import get_next_generation_model_dirs
    from reversi_alpha_zero_amd.worker import evaluate, optimize, self_opt
    monkeypatch.setattr(evaluate, "sleep", lambda s: pytest.fail("the in-process evaluation polls"))
    cfg, best = _self_opt_config(tmp_path / "gated")
    saved = {}   # challenger directory -> the blob the trainer saved there

    def remember(self, _f=optimize.OptimizeWorker.save_current_model):
        out = _f(self)
        rc = self.config.resource
        d = get_next_generation_model_dirs(rc)[-1]
        m = ReversiModel(self.config)
        assert m.load(os.path.join(d, rc.next_generation_model_config_filename), os.path.join(d, rc.next_generation_model_weight_filename))
        saved[d] = m.model.to_blob()
        return out
    monkeypatch.setattr(optimize.OptimizeWorker, "save_current_model", remember)
    with caplog.at_level(logging.INFO, logger=self_opt.logger.name):
        self_opt.start(cfg, games_in_flight=16, backend="hip", total_blocks=2, seed=3, block_games=32, evaluate=True)
    assert get_next_generation_model_dirs(cfg.resource) == [] and os.listdir(cfg.resource.next_generation_model_dir) == []
    kept = ReversiModel(cfg)
    assert kept.load(cfg.resource.model_best_config_path, cfg.resource.model_best_weight_path)   # the best-model files are loadable
    # the logged decisions, in the order they were taken: "evaluated <dir>: new best model" / "... best model kept"
    decisions = [(r.getMessage()[len("evaluated "):].rsplit(": ", 1)) for r in caplog.records if r.getMessage().startswith("evaluated ")]
    assert len(decisions) == len(saved) >= 1 and {d for d, _ in decisions} == set(saved)
    promoted = [saved[d] for d, what in decisions if what == "new best model"]
    assert all(what in ("new best model", "best model kept") for _, what in decisions)
    assert kept.model.to_blob() == (promoted[-1] if promoted else best.model.to_blob())
    # evaluate=False: the challengers stay where the `opt` worker's save put them
    saved.clear()
    cfg2, best2 = _self_opt_config(tmp_path / "plain")
    self_opt.start(cfg2, games_in_flight=16, backend="hip", total_blocks=2, seed=3, block_games=32)
    assert sorted(get_next_generation_model_dirs(cfg2.resource)) == sorted(saved) and len(saved) >= 1
    kept2 = ReversiModel(cfg2)
    assert kept2.load(cfg2.resource.model_best_config_path, cfg2.resource.model_best_weight_path)
    assert kept2.model.to_blob() == best2.model.to_blob()
