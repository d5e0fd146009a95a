"""The `opt` worker's host logic (worker/optimize.py) on the torch backend, the train blob and the trainer section of the config."""
import json
import os

import numpy as np
import pytest
import torch

import train_cases as tc


def _config(tmp_path, **trainer):
    from reversi_alpha_zero_amd.config import Config
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
    cfg.trainer.update(dict(wait_after_save_model_ratio=0, min_data_size_to_learn=1, **trainer))
    return cfg


def _rows(lo, hi):
    own, enemy, policy, z = tc.data()
    return [[[int(own[i]), int(enemy[i])], [float(x) for x in policy[i]], int(z[i])] for i in range(lo, hi)]


def _write(cfg, name, rows):
    path = os.path.join(cfg.resource.play_data_dir, cfg.resource.play_data_filename_tmpl % name)
    with open(path, "wt") as f:
        json.dump(rows, f)
    return path


def _worker(cfg, seed=0, best=True):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.model_helpler import save_as_best_model
    from reversi_alpha_zero_amd.worker.optimize import OptimizeWorker
    if best:
        m = ReversiModel(cfg)
        m.build(seed=5)
        save_as_best_model(m)
    return OptimizeWorker(cfg, backend="torch", seed=seed, device="cpu")


STEPS = (0, 149_999, 150_000, 300_000, 10**6)


def test_decide_learning_rate(tmp_path):
    cfg = _config(tmp_path)
    w = _worker(cfg, best=False)
    assert [w.decide_learning_rate(s) for s in STEPS] == [0.01, 0.01, 0.001, 0.0001, 0.0001]
    for text, want in (("0.5", 0.5), (" 0.25\n", 0.25), ("0", 0.001), ("", 0.001), ("abc", 0.001)):
        with open(cfg.resource.force_learing_rate_file, "wt") as f:
            f.write(text)
        assert w.decide_learning_rate(150_000) == want, text


@pytest.mark.needs_reference
def test_decide_learning_rate_as_the_reference(tmp_path):
    import ref_harness
    ref_harness.install()
    from reversi_zero.worker.optimize import OptimizeWorker as RefWorker
    cfg = _config(tmp_path)
    rcfg = ref_harness.load_config()
    rcfg.resource.force_learing_rate_file = cfg.resource.force_learing_rate_file
    assert [tuple(x) for x in rcfg.trainer.lr_schedules] == [tuple(x) for x in cfg.trainer.lr_schedules]
    ours, ref = _worker(cfg, best=False), RefWorker(rcfg)
    for text in (None, "0.5", "0", "", "abc"):
        if text is not None:
            with open(cfg.resource.force_learing_rate_file, "wt") as f:
                f.write(text)
        assert [ours.decide_learning_rate(s) for s in STEPS] == [ref.decide_learning_rate(s) for s in STEPS], text


def test_trainer_config_defaults_and_yml(tmp_path):
    from reversi_alpha_zero_amd.config import load_config
    cfg = load_config()
    t = cfg.trainer
    assert (t.wait_after_save_model_ratio, t.batch_size, t.min_data_size_to_learn, t.epoch_to_checkpoint, t.start_total_steps,
            t.save_model_steps, t.use_tensorboard, t.logging_per_steps, t.delete_self_play_after_number_of_training) == \
        (1, 256, 100000, 1, 0, 200, True, 100, 0)
    assert [tuple(x) for x in t.lr_schedules] == [(0, 0.01), (150000, 0.001), (300000, 0.0001)]
    assert cfg.resource.force_learing_rate_file.endswith(os.path.join("data", ".force-lr")) or "DATA_DIR" in os.environ
    assert cfg.resource.tensorboard_log_dir.endswith("tensorboard")
    yml = tmp_path / "t.yml"
    yml.write_text("trainer:\n  batch_size: 512\n  lr_schedules:\n    - [0, 0.02]\n    - [10, 0.002]\nmodel:\n  cnn_filter_num: 128\n")
    cfg = load_config(str(yml))
    assert cfg.trainer.batch_size == 512 and cfg.trainer.save_model_steps == 200 and cfg.model.cnn_filter_num == 128
    assert [tuple(x) for x in cfg.trainer.lr_schedules] == [(0, 0.02), (10, 0.002)]


def test_train_blob_round_trip():
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    net = tc.make_net(32, 2, 7)
    mom = [torch.randn(t.shape, generator=torch.Generator().manual_seed(i)) for i, (_, t) in enumerate(net.train_tensors())]
    blob = net.to_train_blob(mom)
    assert blob.dtype == np.float32 and blob.size == 2 * sum(t.numel() for _, t in net.train_tensors()) + sum(t.numel() for _, t in net.stat_tensors())
    other = ReversiNet(32, 2, 7).keras_init_(9)
    mom2 = other.load_train_blob(blob)
    assert other.to_blob() == net.to_blob()
    assert all(torch.equal(a, b) for a, b in zip(mom, mom2))
    assert np.array_equal(other.to_train_blob(mom2).view(np.uint32), blob.view(np.uint32))
    assert np.all(net.to_train_blob()[-10:] == 0)
    with pytest.raises(ValueError):
        ReversiNet(16, 1, 16).load_train_blob(blob)
    with pytest.raises(ValueError):
        ReversiNet(16, 1, 16, 5).to_train_blob()


def test_data_bookkeeping(tmp_path):
    cfg = _config(tmp_path, batch_size=8, save_model_steps=1000, delete_self_play_after_number_of_training=2)
    w = _worker(cfg)
    a, b = _write(cfg, "a", _rows(0, 10)), _write(cfg, "b", _rows(10, 30))
    bad = _write(cfg, "c", [])
    with open(bad, "wt") as f:
        f.write("[[[1, 2], [0.5")   # a file cut short
    w.load_play_data()
    assert w.loaded_filenames == {a, b} and w.dataset_size == 30
    own, enemy, policy, z = w.dataset
    d = tc.data()
    assert own.dtype == np.uint64 and policy.dtype == np.float32 and z.dtype == np.int8
    assert np.array_equal(own, d[0][:30]) and np.array_equal(enemy, d[1][:30]) and np.array_equal(policy, d[2][:30]) and np.array_equal(z, d[3][:30])
    first = w.loaded_data[a]
    w.load_play_data()
    assert w.loaded_data[a] is first, "a file was loaded twice"
    os.remove(b)
    w.load_play_data()
    assert w.loaded_filenames == {a} and w.dataset_size == 10
    os.remove(bad)
    b = _write(cfg, "b", _rows(10, 30))
    # delete_self_play_after_number_of_training = 2: files vanish after the second epoch, not the first
    w.model = w.load_model()
    w.training(max_epochs=1)
    assert os.path.exists(a) and os.path.exists(b)
    w2 = _worker(cfg)
    w2.model = w2.load_model()
    w2.training(max_epochs=2)
    assert not os.path.exists(a) and not os.path.exists(b)


def test_load_model_prefers_the_newest_next_generation_and_raises_without_any(tmp_path):
    cfg = _config(tmp_path)
    with pytest.raises(RuntimeError):
        _worker(cfg, best=False).load_model()
    w = _worker(cfg)
    best = w.load_model()
    w.model = best
    with torch.no_grad():
        best.model.value_fc2.bias.fill_(0.25)
    d = w.save_current_model()
    newest = _worker(cfg, best=False).load_model()
    assert float(newest.model.value_fc2.bias.detach()) == 0.25
    assert newest.digest == newest.fetch_digest(os.path.join(d, cfg.resource.next_generation_model_weight_filename))


def test_epoch_shape_and_save_cadence(tmp_path):
    from reversi_alpha_zero_amd.agent.model import ReversiModel
    from reversi_alpha_zero_amd.lib.data_helper import get_next_generation_model_dirs
    B = 8
    cfg = _config(tmp_path, batch_size=B, save_model_steps=2)
    _write(cfg, "a", _rows(0, 2 * B + 3))
    w = _worker(cfg, seed=4)
    w.model = w.load_model()
    w.compile_model()
    w.load_play_data()
    batches = []
    step = w.trainer.step
    w.trainer.step = lambda own, enemy, policy, z, idx, lr, sync=True: (batches.append(np.array(idx)), step(own, enemy, policy, z, idx, lr, sync))[1]
    fired, saved = [], []

    class Count:
        def on_batch_end(self, batch):
            fired.append(batch)
    from reversi_alpha_zero_amd.worker.optimize import PerStepCallback

    def save():
        d = w.save_current_model()
        saved.append((d, w.trainer.to_net().to_blob(), w.trainer.to_net().to_train_blob()))
    assert w.train_epoch(1, [Count(), PerStepCallback(2, save, 0)]) == 2     # (N // batch_size) * epochs, as the reference counts
    assert fired == [0, 1, 2] and [len(b) for b in batches] == [B, B, 3]     # the final short batch is trained too
    perm = np.concatenate(batches)
    assert sorted(perm) == list(range(2 * B + 3))
    assert np.array_equal(perm, w.epoch_permutation(2 * B + 3, 0)) and np.array_equal(perm, np.random.default_rng((4, 0)).permutation(2 * B + 3))
    assert w.train_epoch(2, [Count(), PerStepCallback(2, save, 0)]) == 4
    assert np.array_equal(np.concatenate(batches[3:6]), np.random.default_rng((4, 1)).permutation(2 * B + 3))
    assert not np.array_equal(np.concatenate(batches[3:6]), perm)
    # 3 + 6 batches, a save every 2nd batch of each callback: 1 + 3 directories
    dirs = get_next_generation_model_dirs(cfg.resource)
    assert len(dirs) == 4 and [d for d, _, _ in saved] == dirs
    for d, blob, train_blob in saved:
        m = ReversiModel(cfg)
        assert m.load(os.path.join(d, cfg.resource.next_generation_model_config_filename),
                      os.path.join(d, cfg.resource.next_generation_model_weight_filename))
        assert m.model.to_blob() == blob
        assert np.array_equal(m.model.to_train_blob().view(np.uint32), train_blob.view(np.uint32))   # bit for bit, the unfolded state


def test_backend_names():
    from reversi_alpha_zero_amd.config import Config
    from reversi_alpha_zero_amd.worker.optimize import OptimizeWorker
    with pytest.raises(ValueError):
        OptimizeWorker(Config(), backend="keras")


def test_a_wrong_l2_factor_fails_the_gradient_rule():
    """The regulariser is l2 sum w^2 over the kernels: gradient term 2 l2 w.  A trainer that adds l2 w instead misses the gradient
    rule of tests/train_cases.py on the kernels (shown here on the CPU with a mutated TorchTrainer against the f64 yardstick), and
    one that regularises the biases and BatchNorm parameters too (weight_decay on every parameter) misses it on those."""
    from reversi_alpha_zero_amd.agent.trainer import TorchTrainer
    net, idx = tc.make_net(16, 1, 16), tc.batch_rows(33)
    with torch.no_grad():   # kernels ten times the initialiser's: the regulariser's share of the gradient is then far above rounding
        for n, t in net.train_tensors():
            if n in ("policy_out.kernel", "dense_1.kernel"):
                t.mul_(10.0)
    good = tc.torch_backward(net, idx, torch.float32)
    ref = tc.torch_backward(net, idx, torch.float64, tc.masks_of(good["acts"]))

    class HalfL2(TorchTrainer):
        def _regulariser(self):
            return 0.5 * super()._regulariser()

    class DecayAll(TorchTrainer):
        def _regulariser(self):
            return self.l2 * sum((w * w).sum() for w in self.params)
    rel = {n: tc.rel_l2(good["grads"][n], ref["grads"][n]) for n in ref["grads"] if not tc.is_conv_bias(n)}
    assert max(rel.values()) < 1e-5
    for cls, where in ((HalfL2, "dense_1.kernel"), (DecayAll, "bn1.gamma")):
        t = cls(net, dtype=torch.float32, l2=tc.L2)
        t.relu_masks = tc.masks_of(good["acts"])
        t.backward(*tc.data(), idx)
        r = tc.rel_l2(t.gradients()[where].double(), ref["grads"][where])
        assert r > tc.K_GRAD * rel[where] + 1e-7, (cls.__name__, where, r, rel[where])
