"""GPU: the loop closes in HBM.  One outbox of 64 mini-net games goes both ways - written to play_*.json files (write_raw) and added
to a DeviceReplay (csrc/raz_replay.hip) - and the two routes must give the `opt` worker the same bytes, the HIP trainer the same
state, and worker/self_opt.py a model the other workers load.  (The configuration is tests/test_optimize_loop_gpu.py's, restated.)"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH = 12288


def _config(root):
    from reversi_alpha_zero_amd.config import Config
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
    cfg.trainer.update(dict(batch_size=BATCH, min_data_size_to_learn=100, save_model_steps=5, wait_after_save_model_ratio=0,
                            epoch_to_checkpoint=1))
    return cfg


def _best_model(cfg):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.model_helpler import save_as_best_model
    cfg.resource.create_directories()
    best = ReversiModel(cfg)
    best.build(seed=5)
    save_as_best_model(best)
    return best


def test_the_replay_is_the_files_and_trains_to_the_same_state(tmp_path):
    from reversi_alpha_zero_amd.engine import raw_from_packed
    from reversi_alpha_zero_amd.lib.data_helper import get_game_data_filenames
    from reversi_alpha_zero_amd.lib.replay import DeviceReplay
    from reversi_alpha_zero_amd.worker.optimize import OptimizeWorker
    from reversi_alpha_zero_amd.worker.self_play import BatchedSelfPlayWorker
    cfg = _config(tmp_path)
    best = _best_model(cfg)
    # 64 games by continuous batching on 16 slots: one id-ordered outbox
    player = BatchedSelfPlayWorker(cfg, best.model.to_blob(), games_in_flight=16, seed=3, device=DEV, block_games=64)
    pk = player.play_block_continuous(0)(None)
    assert pk["headers"].shape[0] == 64
    player.write_raw(raw_from_packed(*(pk[k].cpu().numpy() for k in ("headers", "root_n", "summary"))), 1)
    assert len(get_game_data_filenames(cfg.resource)) == 8
    replay = DeviceReplay.from_config(cfg, DEV)
    added = replay.add(pk["headers"], pk["root_n"], pk["summary"])
    assert (replay.games, replay.rows, replay.version) == (64, added, 1) and added > BATCH

    def worker(sub, rp):
        c = _config(tmp_path)
        c.resource.next_generation_model_dir = os.path.join(str(tmp_path), sub)
        return c, OptimizeWorker(c, backend="hip", seed=1, device=DEV, replay=rp)
    # the data set: byte-equal to what load_play_data builds from the files
    _, from_files = worker("next_files", None)
    from_files.load_play_data()
    ds = replay.dataset()
    assert all(t.is_cuda and t.is_contiguous() for t in ds) and from_files.dataset_size == replay.rows
    for name, want, got in zip(("own", "enemy", "policy", "z"), from_files.dataset, ds):
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, name
        assert got.tobytes() == want.tobytes(), name
    # two epochs of the HIP trainer from either source: the same rows in the same order, a reproducible step - the same bytes
    _, a = worker("next_files", None)
    a.start(max_epochs=2)
    cfg_b, b = worker("next_replay", replay)
    b.start(max_epochs=2)
    assert b.dataset_size == replay.rows and not b.loaded_filenames and all(t.is_cuda for t in b.dataset)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(b._resident_dataset(), ds))   # the replay's tensors, in place
    sa, sb = a.trainer.state(), b.trainer.state()
    assert sa.keys() == sb.keys()
    for name in sa:
        assert torch.equal(sa[name].cpu(), sb[name].cpu()), name
    assert len(get_game_data_filenames(cfg.resource)) == 8   # (nothing was deleted)


def test_self_opt_plays_stores_and_trains_without_files(tmp_path):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.data_helper import get_game_data_filenames, get_next_generation_model_dirs
    from reversi_alpha_zero_amd.worker import self_opt
    cfg = _config(tmp_path)
    cfg.trainer.update(dict(batch_size=2048, save_model_steps=10))
    _best_model(cfg)
    player, trainer, replay = self_opt.start(cfg, games_in_flight=16, backend="hip", total_blocks=2, seed=3, block_games=32)
    assert replay.games == 64 and replay.rows > 2048 and replay.version == 2
    assert trainer.dataset_size == replay.rows and trainer.epoch_counter == 2
    assert os.listdir(cfg.resource.play_data_dir) == []
    dirs = get_next_generation_model_dirs(cfg.resource)
    assert len(dirs) >= 1
    m = ReversiModel(cfg)
    assert m.load(os.path.join(dirs[-1], cfg.resource.next_generation_model_config_filename),
                  os.path.join(dirs[-1], cfg.resource.next_generation_model_weight_filename))
    with open(cfg.resource.self_play_game_idx_file) as f:
        assert int(f.read()) == 64
    # the same with the files written beside the replay: the directory holds the games the replay holds
    cfg2 = _config(tmp_path / "with_files")
    cfg2.trainer.update(dict(batch_size=2048, save_model_steps=10))
    _best_model(cfg2)
    _, _, replay2 = self_opt.start(cfg2, games_in_flight=16, backend="hip", total_blocks=1, seed=3, block_games=32, write_files=True)
    assert len(get_game_data_filenames(cfg2.resource)) == 4 and replay2.games == 32
