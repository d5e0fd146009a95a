"""CPU: the host side of the device replay (lib/replay.py, worker/optimize.py's replay option, worker/self_opt.py) - the window
arithmetic on game numbers alone against a model of the play-data directory, the row bookkeeping of DeviceReplay on host tensors,
the refusals, and OptimizeWorker(replay=None) still reading the files."""
import os

import numpy as np
import pytest
import torch


def _directory_model(adds, nb, keep):
    """What BatchedSelfPlayWorker.write_raw + remove_play_data leave after each add: a file per nb games (game numbers), the oldest
    files removed beyond `keep`, and the games still in the worker's buffer.  Returns [(first game held, games held)] per add."""
    files, buffer, nxt, out = [], [], 0, []
    for a in adds:
        for _ in range(a):
            buffer.append(nxt)
            nxt += 1
            if nxt % nb == 0:
                files.append(buffer)
                buffer = []
                del files[:max(0, len(files) - keep)]
        held = [g for f in files for g in f] + buffer
        out.append((held[0] if held else nxt, len(held)))
    return out


@pytest.mark.parametrize("nb,keep", [(8, 3), (1, 1), (1, 5), (2, 800), (64, 2), (5, 1)])
def test_window_arithmetic_is_the_directory_s(nb, keep):
    """Adds of 1, nb - 1, nb, of more than the whole window, and a random mixture: the games held after every add are the games the
    files (and the worker's buffer) would hold; whole groups leave, oldest first."""
    from reversi_alpha_zero_amd.lib.replay import games_to_drop
    rng = np.random.default_rng(nb * 1000 + keep)
    adds = [1, max(nb - 1, 1), nb, nb, nb * keep, 1, nb * keep + 1, nb * (keep + 3) + 2, 3 * nb * keep + nb - 1, nb - 1 or 1, 1]
    adds += [int(x) for x in rng.integers(1, 3 * nb + 2, size=40)]
    first, games, got = 0, 0, []
    for a in adds:
        games += a
        drop = games_to_drop(first, games, nb, keep)
        assert drop % nb == 0 and 0 <= drop <= games
        first, games = first + drop, games - drop
        assert first % nb == 0 and games - (first + games) % nb <= nb * keep
        got.append((first, games))
    want = _directory_model(adds, nb, keep)
    # (an empty window has no first game in the model: compare the games, and the first game where there is one)
    assert [g for _, g in got] == [g for _, g in want]
    assert all(a == b for (a, n), (b, _) in zip(got, want) if n)
    with pytest.raises(ValueError):
        games_to_drop(0, 4, 0, 3)
    with pytest.raises(ValueError):
        games_to_drop(0, 4, 8, 0)
    if nb > 1:
        with pytest.raises(ValueError):
            games_to_drop(1, 4, nb, keep)


def test_replay_row_bookkeeping_on_host_tensors():
    """DeviceReplay's parts, per-game row counts and dataset() with the rows given directly (no kernel, tensors on the CPU): games
    of 0, 8, 16 ... rows, groups of 2 games, 2 groups kept."""
    from reversi_alpha_zero_amd.lib.replay import DeviceReplay, games_to_drop
    r = DeviceReplay(2, 2, change_tau_turn=4, save_policy_of_tau_1=True, device="cpu")
    assert (r.games, r.rows, r.version) == (0, 0, 0) and [len(t) for t in r.dataset()] == [0, 0, 0, 0]
    assert r.dataset()[2].shape == (0, 64)
    nxt = 0

    def add(per_game):   # what DeviceReplay.add does once rows_from_outbox has answered
        nonlocal nxt
        n = int(sum(per_game))
        ids = torch.arange(nxt, nxt + n, dtype=torch.int64)
        nxt += n
        if n:
            r._parts.append((ids, -ids, ids[:, None].float().repeat(1, 64), (ids % 3 - 1).to(torch.int8)))
        r._game_rows = np.concatenate([r._game_rows, np.asarray(per_game, dtype=np.int64)])
        r._drop_front(games_to_drop(r.first_game, r.games, r.nb_game_in_file, r.max_file_num))
        r.version += 1

    def check(first_row, rows, games, first_game):
        own, enemy, policy, z = r.dataset()
        assert (r.rows, r.games, r.first_game) == (rows, games, first_game)
        assert own.tolist() == list(range(first_row, first_row + rows)) and enemy.tolist() == [-i for i in own.tolist()]
        assert policy.shape == (rows, 64) and policy[:, 63].tolist() == [float(i) for i in own.tolist()]
        assert all(t.is_contiguous() and t.storage_offset() == 0 for t in (own, enemy, policy, z))
    add([8, 0, 16])            # games 0-2: one whole group and a game of the next
    check(0, 24, 3, 0)
    add([8])                   # games 0-3: two whole groups
    check(0, 32, 4, 0)
    add([24])                  # game 4 opens a third group: nothing leaves until it is whole
    check(0, 56, 5, 0)
    add([8])                   # group 2 whole: group 0 (games 0, 1: 8 rows) leaves - a cut inside the first part
    check(8, 56, 4, 2)
    add([8] * 9)               # more than the whole window: games 6-14 arrive, groups 5 and 6 stay, game 14 behind them
    check(8 + 16 + 8 + 24 + 8 + 8 * 4, 40, 5, 10)
    assert r.version == 5


def test_rows_from_outbox_refuses_host_tensors_and_wrong_shapes():
    from reversi_alpha_zero_amd.lib.replay import rows_from_outbox
    hdr, rn, sm = torch.zeros((2, 3, 48), dtype=torch.uint8), torch.zeros((2, 3, 64), dtype=torch.int32), torch.zeros((2, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="device-only"):
        rows_from_outbox(hdr, rn, sm, change_tau_turn=4, save_policy_of_tau_1=True)
    with pytest.raises(TypeError):
        rows_from_outbox(hdr.numpy(), rn, sm, change_tau_turn=4, save_policy_of_tau_1=True)


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
    rc.self_play_game_idx_file = os.path.join(d, ".self-play-game-idx")
    cfg.trainer.update(dict(delete_self_play_after_number_of_training=1))
    return cfg


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return [[[int(rng.integers(1, 2 ** 62)), int(rng.integers(1, 2 ** 62))], [float(x) for x in rng.random(64)], int(rng.integers(-1, 2))]
            for _ in range(n)]


class _StubReplay:
    """What OptimizeWorker asks of a replay: `version` and `dataset()`."""

    def __init__(self):
        self.version, self.calls = 1, 0
        self.data = (torch.arange(5), torch.arange(5) + 7, torch.rand(5, 64), torch.ones(5, dtype=torch.int8))

    def dataset(self):
        self.calls += 1
        return self.data


def test_optimize_worker_reads_files_without_a_replay_and_the_replay_with_one(tmp_path):
    from reversi_alpha_zero_amd.lib.data_helper import pack_game_data, write_game_data_to_file
    from reversi_alpha_zero_amd.worker.optimize import OptimizeWorker
    cfg = _config(tmp_path)
    os.makedirs(cfg.resource.play_data_dir)
    rows = [_rows(16, 1), _rows(24, 2)]
    paths = [os.path.join(cfg.resource.play_data_dir, cfg.resource.play_data_filename_tmpl % f"2020010{i}-000000.000000") for i in (1, 2)]
    for p, r in zip(paths, rows):
        write_game_data_to_file(p, r)
    # replay=None: the files, as before
    w = OptimizeWorker(cfg, backend="torch", device="cpu")
    assert w.replay is None
    w.load_play_data()
    assert w.dataset_size == 40 and w.loaded_filenames == set(paths)
    for got, want in zip(w.dataset, pack_game_data(rows[0] + rows[1])):
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    w.count_up_training_count_and_delete_self_play_data_files()   # (delete_self_play_after_number_of_training = 1)
    assert not any(os.path.exists(p) for p in paths)
    # with a replay: its tensors as they are, taken again only when its version moves; no file is read and none deleted
    for p, r in zip(paths, rows):
        write_game_data_to_file(p, r)
    stub = _StubReplay()
    w = OptimizeWorker(cfg, backend="torch", device="cpu", replay=stub)
    w.load_play_data()
    w.load_play_data()
    assert stub.calls == 1 and w.dataset_size == 5 and not w.loaded_filenames
    assert all(a is b for a, b in zip(w.dataset, stub.data)) and all(a is b for a, b in zip(w._resident_dataset(), stub.data))
    stub.version, stub.data = 2, tuple(torch.cat([t, t]) for t in stub.data)
    w.load_play_data()
    assert stub.calls == 2 and w.dataset_size == 10
    w.count_up_training_count_and_delete_self_play_data_files()
    assert all(os.path.exists(p) for p in paths)


def test_self_opt_is_one_rank(monkeypatch, tmp_path):
    from reversi_alpha_zero_amd.worker import self_opt
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process on one GPU"):
        self_opt.start(_config(tmp_path), total_blocks=1)
    assert not os.path.exists(os.path.join(str(tmp_path), "model"))   # (refused before anything is touched)


def test_device_replay_refuses_a_config_that_drops_draws(tmp_path):
    from reversi_alpha_zero_amd.lib.replay import DeviceReplay
    cfg = _config(tmp_path)
    r = DeviceReplay.from_config(cfg, "cpu")
    assert (r.nb_game_in_file, r.max_file_num) == (cfg.play_data.nb_game_in_file, cfg.play_data.max_file_num)
    cfg.play_data.drop_draw_game_rate = 0.5
    with pytest.raises(ValueError, match="drop_draw_game_rate"):
        DeviceReplay.from_config(cfg, "cpu")
