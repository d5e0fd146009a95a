"""raznet-train-v2 on the device (DeviceTrainer(precision="f16x3"): csrc/raz_train_f16x3.h) against the f64 restatement, tensor by
tensor: the scenarios and rules of tests/train_cases.py with v2's constants (tests/train_f16x3_util.py), at the smallest shapes that
reach every edge of the new kernels' tiles - k_tconv_f16x3's 4 positions x 64 output channels (batches 1, 4, 5; 16, 32, 48, 80, 128,
192 channels), k_twgrad_f16x3's 64 x 32 channel tile and the 32 position splits (batches 33, 67, 257).  The test of record of v2;
tests/test_train_f16x3_emu.py is its twin on the wave emulator.  RAZ_TRAIN_ACCURACY_JSON=<path> appends the measured ratios
(driver "gpu-f16x3")."""
import json
import os

import numpy as np
import pytest
import torch

import train_cases as tc
import train_f16x3_util as v2

pytestmark = pytest.mark.gpu
DEV = v2.DEV
make = v2.make_gpu
CASES = [(F, R, V, B) for (F, R, V) in tc.SHAPES for B in (1, 4, 5, 33, 67)]
EDGE_CASES = [(F, R, V, B) for (F, R, V) in [(48, 1, 16), (80, 1, 7)] for B in (3, 33)]


@pytest.fixture(autouse=True)
def _constants(monkeypatch):
    v2.use_v2_constants(monkeypatch)


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_forward_in_training_mode(F, R, V, B):
    tc.forward_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_gradients_tensor_by_tensor(F, R, V, B):
    tc.gradient_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


def test_both_rules_on_a_batch_of_257():
    c = tc.case(make, 16, 1, 16, 257, rows="long")
    tc.forward_rule(make, c, (16, 1, 16, 257))
    tc.gradient_rule(make, c, (16, 1, 16, 257))


def test_degenerate_values():
    c = tc.case(make, 16, 1, 16, 33, rows="degenerate")
    tc.degenerate_guards_and_exact_values(make, c)
    tc.forward_rule(make, c, (16, 1, 16, 33, "degenerate"), guards=False)
    tc.gradient_rule(make, c, (16, 1, 16, 33, "degenerate"))


@pytest.mark.parametrize("F,R,V,B", [(16, 1, 16, 67), (128, 1, 64, 67)])
def test_eight_steps_track_the_f64_trainer(F, R, V, B):
    tc.eight_steps_track_the_f64_trainer(make, F, R, V, B)


def test_two_trainers_hold_the_same_bytes():
    tc.two_trainers_hold_the_same_bytes(make, 128, 1, 64)


@pytest.mark.parametrize("F,R,V", [(16, 1, 16), (32, 2, 7), (128, 1, 64)])
def test_the_batch_size_alone_fixes_the_bytes(F, R, V):
    tc.the_batch_size_alone_fixes_the_bytes(make, F, R, V)


def test_v2_differs_from_v1_in_the_trunk_and_reads_its_precision_back():
    from reversi_alpha_zero_amd import _native as N
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    v2.trunk_differs_and_precisions_read_back(make, lambda net, mb: DeviceTrainer(net, max_batch=mb, device=DEV, l2=tc.L2),
                                              lambda t: N.lib.raz_trainer_precision(t.handle))


def test_one_row_dominates_the_output_gradients(monkeypatch):
    v2.skewed_gradients_meet_the_rule(make, monkeypatch)


def test_the_worker_trains_an_epoch_in_f16x3_and_saves_a_model_the_net_kernels_load(tmp_path):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.engine import DeviceNet
    from reversi_alpha_zero_amd.lib.data_helper import get_next_generation_model_dirs
    from reversi_alpha_zero_amd.lib.model_helpler import save_as_best_model
    from reversi_alpha_zero_amd.worker.optimize import OptimizeWorker
    cfg = Config()
    cfg.model.update(dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=16))
    rc, d = cfg.resource, str(tmp_path)
    rc.data_dir, rc.model_dir = d, os.path.join(d, "model")
    rc.model_best_config_path = os.path.join(rc.model_dir, "model_best_config.json")
    rc.model_best_weight_path = os.path.join(rc.model_dir, "model_best_weight.h5")
    rc.next_generation_model_dir = os.path.join(rc.model_dir, "next_generation")
    rc.play_data_dir = os.path.join(d, "play_data")
    rc.force_learing_rate_file = os.path.join(d, ".force-lr")
    os.makedirs(rc.play_data_dir, exist_ok=True)
    os.makedirs(rc.next_generation_model_dir, exist_ok=True)
    cfg.trainer.update(dict(wait_after_save_model_ratio=0, min_data_size_to_learn=1, batch_size=62, save_model_steps=3, epoch_to_checkpoint=1))
    best = ReversiModel(cfg)
    best.build(seed=5)
    save_as_best_model(best)
    own, enemy, policy, z = tc.data()
    rows = [[[int(own[i]), int(enemy[i])], [float(x) for x in policy[i]], int(z[i])] for i in range(len(own))]
    for name in ("0", "1"):   # the rows twice (a data set may hold a position many times): 372 rows, six batches of 62
        with open(os.path.join(rc.play_data_dir, rc.play_data_filename_tmpl % name), "wt") as f:
            json.dump(rows, f)
    w = OptimizeWorker(cfg, backend="hip", precision="f16x3", seed=1, device=DEV)
    w.start(max_epochs=1)
    assert isinstance(w.trainer, DeviceTrainer) and w.trainer.precision == "f16x3"
    assert w.dataset_size == 2 * len(own) and w.dataset_size >= 200
    dirs = get_next_generation_model_dirs(rc)
    assert w.dataset_size % (62 * 3) == 0 and len(dirs) == w.dataset_size // 62 // 3 and dirs   # the last save follows the last step
    m = ReversiModel(cfg)
    assert m.load(os.path.join(dirs[-1], rc.next_generation_model_config_filename), os.path.join(dirs[-1], rc.next_generation_model_weight_filename))
    trained = w.trainer.to_net()
    assert not np.array_equal(np.frombuffer(trained.to_blob(), np.uint8), np.frombuffer(best.model.to_blob(), np.uint8)), "the epoch changed nothing"
    o, e = torch.from_numpy(own.view(np.int64)).to(DEV), torch.from_numpy(enemy.view(np.int64)).to(DEV)
    sh = np.arange(64, dtype=np.uint64)
    planes = np.stack([((own[:, None] >> sh) & 1), ((enemy[:, None] >> sh) & 1)], axis=1).astype(np.float32).reshape(-1, 2, 8, 8)
    # the saved model (written after the epoch's last step) through the forward kernels against the trainer's own state through torch
    p, v = DeviceNet(m.model.to_blob(), DEV).predict_bitboards(o, e)
    with torch.no_grad():
        tp, tv = trained.eval()(torch.from_numpy(planes))
    assert float((p.cpu() - tp).abs().max()) <= 1e-5 and float((v.cpu() - tv[:, 0]).abs().max()) <= 1e-5
