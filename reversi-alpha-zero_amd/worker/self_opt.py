"""Self-play and training in ONE process on one GPU, joined in HBM instead of by text files (no reference counterpart: the
reference's `self` and `opt` workers are two processes that meet in data/play_data, worker/self_play.py:180-194 and
worker/optimize.py:165-212).

A block of games is played with BatchedSelfPlayWorker.play_block_continuous; its id-ordered device outbox goes into a
lib/replay.DeviceReplay - the trainer's packed rows, made on the device (csrc/raz_replay.hip), bit for bit the rows the files would
give - and OptimizeWorker(replay=...) trains one pass on the replay's window, saving next_generation/model_* as the `opt` worker
does, so that the `eval` worker is unchanged.  The net that plays is the BEST model, reloaded by digest between blocks exactly as the
`self` worker does it (try_reload_model).  With write_files=True the same games are also written as play_*.json (write_raw), for
the reference's own consumers.  One rank: world > 1 is refused.
"""
import os
from logging import getLogger

logger = getLogger(__name__)


def _world():
    return int(os.environ.get("WORLD_SIZE", "1"))


def start(config, games_in_flight=None, backend="hip", precision=None, write_files=False, total_blocks=None, seed=0, block_games=None):
    """Alternate play - store - train until total_blocks blocks have been played (None = forever).  Returns (the self-play worker, the
    optimize worker, the replay).  block_games: the game ids of a block (default: the `self` worker's default_block_games, rounded up to
    whole play files)."""
    if _world() > 1:
        raise ValueError(f"self_opt runs one process on one GPU (WORLD_SIZE={_world()}): run the `self` and `opt` workers for more")
    import torch
    from ..engine import bookkeeping_from_summaries, packed_to_host
    from ..lib.replay import DeviceReplay
    from .optimize import OptimizeWorker
    from .self_play import (BatchedSelfPlayWorker, default_block_games, load_model, read_as_int, try_reload_model,
                            whole_files_block)
    if not torch.cuda.is_available():
        raise RuntimeError("the self-play engine is device-only: no GPU visible (there is no CPU fallback)")
    device = "cuda:0"
    rc = config.resource
    rc.create_directories()
    model = load_model(config)   # the best model (or the newest next-generation one, as play.use_newest_next_generation_model asks)
    blob = model.model.to_blob()
    B = games_in_flight or 4096
    blk = whole_files_block(config, block_games or default_block_games(blob, B))
    player = BatchedSelfPlayWorker(config, blob, B, seed=seed, device=device, block_games=blk)
    if player._series_length() != 1:
        raise ValueError("self_opt plays blocks with continuous batching: play.share_mtcs_info_in_self_play needs reset_mtcs_info_per_game = 1")
    replay = DeviceReplay.from_config(config, device)
    trainer = OptimizeWorker(config, backend=backend, seed=seed, device=device, precision=precision, replay=replay)
    game_idx = read_as_int(rc.self_play_game_idx_file) or 0
    local_idx, blocks = 1, 0
    while total_blocks is None or blocks < total_blocks:
        # ---- play
        # (a block during which the net left the f16 range of the split-operand trunk is void: played again on the exact-f32 kernels)
        pk = player.play_block_in_range(game_idx, player.play_block_continuous)()
        # ---- store: the rows stay in HBM; the host sees 32 bytes per game (the resignation bookkeeping)
        replay.add(pk["headers"], pk["root_n"], pk["summary"])
        player.bookkeep_raw(bookkeeping_from_summaries(pk["summary"].cpu().numpy()))
        if write_files:
            player.write_raw(packed_to_host(pk), local_idx)
        del pk
        game_idx += blk
        local_idx += blk
        blocks += 1
        player._write_game_idx(game_idx)
        # ---- train: one pass over the window, once it is large enough
        if replay.rows >= config.trainer.min_data_size_to_learn:
            if trainer.model is None:
                trainer.model = trainer.load_model()
            trainer.training(max_epochs=1)
        else:
            logger.info(f"replay rows={replay.rows} is less than {config.trainer.min_data_size_to_learn}")
        new_blob = model.model.to_blob() if try_reload_model(config, model) else None
        if new_blob is not None:
            player.set_net_blob(new_blob)
    return player, trainer, replay
