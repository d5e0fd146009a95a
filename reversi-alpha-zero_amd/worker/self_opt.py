"""Self-play and training in ONE process on one GPU, joined in HBM instead of by text files (no reference counterpart: the
reference's `self` and `opt` workers are two processes that meet in data/play_data, worker/self_play.py:180-194 and
worker/optimize.py:165-212).

A block of games is played with BatchedSelfPlayWorker.play_block_continuous; its id-ordered device outbox goes into a
lib/replay.DeviceReplay - the trainer's packed rows, made on the device (csrc/raz_replay.hip), bit for bit the rows the files would
give - and OptimizeWorker(replay=...) trains one pass on the replay's window, saving next_generation/model_* as the `opt` worker
does, so that the `eval` worker is unchanged.  The net that plays is the BEST model, reloaded by digest between blocks exactly as the
`self` worker does it (try_reload_model).  With write_files=True the same games are also written as play_*.json (write_raw), for
the reference's own consumers.  One rank: world > 1 is refused.

evaluate=True closes the reference's third process into the loop as well: after a training pass every model under next_generation/
is challenged in this process by EvaluateWorker(handoff="device") - the match whose hand-offs stay on the device - and promoted or
removed as the `eval` worker does it, so that the next block's digest check finds a new best model without a second process.

archive_generations=True keeps what the `eval` worker throws away: every promoted challenger is also saved under
<model_dir>/generations/, and the best model the run started from as generation 0, for worker/league.py to rate.
"""
import os
from logging import getLogger

logger = getLogger(__name__)


def _world():
    return int(os.environ.get("WORLD_SIZE", "1"))


GENERATION_ZERO = "00000000-000000.000000"   # sorts before every challenger's time stamp


def generations_dir(config):
    return os.path.join(config.resource.model_dir, "generations")


def archived_generation_dirs(config):
    """The archived generations in name order: the starting model first, then the promotions by their challengers' time stamps."""
    from glob import glob
    return sorted(glob(os.path.join(generations_dir(config), config.resource.next_generation_model_dirname_tmpl % "*")))


def archive_generation(config, model, dirname):
    """Save `model` as <model_dir>/generations/<dirname>/ under the next-generation file names.  Returns the directory."""
    rc = config.resource
    d = os.path.join(generations_dir(config), dirname)
    os.makedirs(d, exist_ok=True)
    model.save(os.path.join(d, rc.next_generation_model_config_filename), os.path.join(d, rc.next_generation_model_weight_filename))
    return d


def evaluate_challengers(config, evaluator, player=None, archive=False):
    """Challenge every model under next_generation/ (evaluate.py:31-42 without the polling sleep: the directory is listed, never waited
    for) with `evaluator`, an EvaluateWorker: the better one becomes the best model, every one is removed.  The two engines of a
    challenge live for that challenge only; where they do not fit beside `player`'s self-play engine, that engine is dropped first
    (BatchedSelfPlayWorker._drop_engine: the next block rebuilds it).  archive: a promoted challenger is also saved under generations/,
    in a directory of its own directory's name.  Returns [(model_dir, became_best)]."""
    import gc
    import torch
    from ..lib.data_helper import get_next_generation_model_dirs
    from ..lib.model_helpler import save_as_best_model
    decisions = []
    while get_next_generation_model_dirs(config.resource):
        if evaluator.best_model is None:
            evaluator.best_model = evaluator.load_best_model()
        ng_model, model_dir = evaluator.load_next_generation_model()   # (a directory is there: it does not sleep)
        draws = evaluator.random.getstate(), evaluator.games_played
        try:
            better = evaluator.evaluate_model(ng_model)
        except torch.cuda.OutOfMemoryError:
            if player is None or player._engine is None:
                raise
            logger.info("the evaluation engines do not fit beside the self-play engine: dropping it for the challenge")
            player._drop_engine()
            evaluator.random.setstate(draws[0])
            evaluator.games_played = draws[1]
            better = evaluator.evaluate_model(ng_model)
        logger.info(f"evaluated {model_dir}: {'new best model' if better else 'best model kept'}")
        if better:
            save_as_best_model(ng_model)
            evaluator.best_model = ng_model
            if archive:
                archive_generation(config, ng_model, os.path.basename(os.path.normpath(model_dir)))
        evaluator.remove_model(model_dir)
        decisions.append((model_dir, better))
        gc.collect()
        torch.cuda.empty_cache()   # the challenge's engines go back to the device before the next engine is sized
    return decisions


def start(config, games_in_flight=None, backend="hip", precision=None, write_files=False, total_blocks=None, seed=0, block_games=None,
          evaluate=False, archive_generations=False):
    """Alternate play - store - train until total_blocks blocks have been played (None = forever).  Returns (the self-play worker, the
    optimize worker, the replay).  block_games: the game ids of a block (default: the `self` worker's default_block_games, rounded up to
    whole play files).  evaluate: challenge the models a training pass saved, in this process (evaluate_challengers).
    archive_generations: with evaluate, keep every promoted model, and the best model of the first block, under <model_dir>/generations/
    (False: nothing is written there)."""
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
    evaluator = None
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
        if evaluate:
            if evaluator is None:
                from .evaluate import EvaluateWorker
                evaluator = EvaluateWorker(config, seed=seed, device=device, handoff="device")
                if archive_generations and not os.path.isdir(os.path.join(generations_dir(config), rc.next_generation_model_dirname_tmpl % GENERATION_ZERO)):
                    archive_generation(config, evaluator.load_best_model(), rc.next_generation_model_dirname_tmpl % GENERATION_ZERO)
            evaluate_challengers(config, evaluator, player, archive=archive_generations)
        new_blob = model.model.to_blob() if try_reload_model(config, model) else None
        if new_blob is not None:
            player.set_net_blob(new_blob)
    return player, trainer, replay
