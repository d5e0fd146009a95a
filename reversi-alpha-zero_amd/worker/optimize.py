"""The `opt` worker (reversi_zero/worker/optimize.py): trains the net on the play_*.json files the `self` worker writes and saves
next_generation/model_* directories the `self` and `eval` workers pick up.  Method by method the reference's behaviour; what Keras
did inside `fit` is agent/trainer.py's raznet-train-v1 step, on the HIP kernels (backend="hip") or restated over torch autograd
(backend="torch", CPU or GPU).  The data set is kept PACKED (lib/data_helper.pack_game_data: 273 bytes a row) and resident on the
trainer's device; a batch is a list of row numbers.  TensorBoard logging is not restated: losses go to `logging`.
"""
import os
from collections import Counter
from datetime import datetime
from logging import getLogger
from time import sleep, time

import numpy as np

from ..agent.model import ReversiModel
from ..lib.data_helper import get_game_data_filenames, get_next_generation_model_dirs, pack_game_data, read_game_data_from_file
from ..lib.model_helpler import load_best_model_weight

logger = getLogger(__name__)

# Which step runs by default: measured on one MI355X at the 256x10 net and batch 256 (tools/bench_train.py, DESIGN.md section 4.8,
# profiles/r7/train_step_timing.json) the HIP step takes 18.6 ms and fp32 torch-ROCm's 14.6 ms ON THE GPU, so the default is the torch
# restatement, run on the GPU (default_device); backend="hip" is the faster step for the mini net (1.2 against 2.7 ms) and the bit-reproducible one everywhere.
# backend="hip" with precision="f16x3" (raznet-train-v2, opt-in) took 11.4 ms in one process with v1's 18.7 and torch's 15.2 (profiles/r10/
# train_step_timing_f16x3.json); whether a default should follow is decided from those numbers, not here.
DEFAULT_BACKEND = "torch"


def default_device(backend):
    """Where a worker trains when it is not told: the first GPU.  The hip backend has no other place; the torch backend is the
    default BECAUSE of its step time on the GPU, so it runs there whenever there is one and on the CPU only without."""
    import torch
    return "cuda:0" if backend == "hip" or torch.cuda.is_available() else "cpu"


def start(config, backend=None, seed=0, max_epochs=None, device=None, precision=None, replay=None):
    return OptimizeWorker(config, backend=backend or DEFAULT_BACKEND, seed=seed, device=device, precision=precision,
                          replay=replay).start(max_epochs=max_epochs)


class OptimizeWorker:
    def __init__(self, config, backend=DEFAULT_BACKEND, seed=0, device=None, precision=None, replay=None):
        """precision (backend="hip" alone): "f32" - raznet-train-v1, what None means - or "f16x3", raznet-train-v2.
        replay (a lib/replay.DeviceReplay, or None): the data set is the replay's - the rows the self-play engine left in HBM, packed
        there - instead of the play_*.json files: no file is read, none is deleted, and the trainer reads the replay's tensors in place."""
        if backend not in ("hip", "torch"):
            raise ValueError(f"backend={backend!r}: 'hip' or 'torch'")
        if precision is not None:
            if backend != "hip":
                raise ValueError(f"precision={precision!r} is an option of backend='hip'; backend='torch' trains in fp32")
            from ..agent.trainer import precision_code
            precision_code(precision)
        self.precision = precision or "f32"
        self.config = config
        self.backend, self.seed, self.device = backend, seed, device or default_device(backend)
        self.model = None  # type: ReversiModel
        self.trainer = None
        self.loaded_filenames = set()
        self.loaded_data = {}   # filename -> (own u64[n], enemy u64[n], policy f32[n,64], z i8[n])
        self.training_count_of_files = Counter()
        self.dataset = None     # the same four arrays over every loaded file
        self._resident = None   # ... as tensors on the trainer's device
        self.replay = replay
        self._replay_version = None
        self._resume = None     # (total steps, callbacks) of the last training() call
        self.lr = None
        self.epoch_counter = 0
        self.last_losses = None

    # ---- the loop (optimize.py:40-71) ----------------------------------------------------------------------------------------
    def start(self, max_epochs=None):
        self.model = self.load_model()
        self.training(max_epochs=max_epochs)

    def training(self, max_epochs=None, sleep_sec=10):
        tc = self.config.trainer
        if self.replay is not None and self._resume is not None:
            # a replay's worker is called once per block of games (worker/self_opt.py): it goes on where the last call stopped - the
            # same trainer (weights, momentum), step count (learning rate schedule) and save cadence
            total_steps, callbacks = self._resume
        else:
            self.compile_model()
            total_steps = tc.start_total_steps
            callbacks = [PerStepCallback(tc.save_model_steps, self.save_current_model, tc.wait_after_save_model_ratio)]
        rounds = 0
        while max_epochs is None or rounds < max_epochs:
            self.load_play_data()
            if self.dataset_size < tc.min_data_size_to_learn:
                logger.info(f"dataset_size={self.dataset_size} is less than {tc.min_data_size_to_learn}")
                if max_epochs is not None:
                    raise RuntimeError(f"dataset_size={self.dataset_size} is less than min_data_size_to_learn={tc.min_data_size_to_learn}")
                sleep(sleep_sec)
                continue
            self.update_learning_rate(total_steps)
            total_steps += self.train_epoch(tc.epoch_to_checkpoint, callbacks)
            self.count_up_training_count_and_delete_self_play_data_files()
            rounds += 1
            self._resume = (total_steps, callbacks)
        return total_steps

    def compile_model(self):
        """SGD(lr=1e-2, momentum=0.9) over the two losses (optimize.py:82-85): the trainer of the chosen backend."""
        from ..agent.trainer import DeviceTrainer, TorchTrainer
        tc, l2 = self.config.trainer, self.config.model.l2_reg
        self.lr = 1e-2
        if self.backend == "hip":
            self.trainer = DeviceTrainer(self.model.model, max_batch=tc.batch_size, device=self.device, l2=l2, precision=self.precision)
        else:
            self.trainer = TorchTrainer(self.model.model, max_batch=tc.batch_size, device=self.device, l2=l2)

    def epoch_permutation(self, n, epoch):
        """Keras fit(shuffle=True): a fresh permutation of the rows per epoch - here a pure function of (seed, epoch counter)."""
        return np.random.default_rng((self.seed, epoch)).permutation(n)

    def train_epoch(self, epochs, callbacks):
        """`epochs` passes over the data set in batches of batch_size, the final short batch included; returns the step count as
        the reference counts it: (N // batch_size) * epochs (optimize.py:73-80)."""
        tc = self.config.trainer
        own, enemy, policy, z = self._resident_dataset()
        n = self.dataset_size
        for _ in range(epochs):
            perm = self._on_device(self.epoch_permutation(n, self.epoch_counter))   # uploaded once, sliced on the device
            self.epoch_counter += 1
            for batch, lo in enumerate(range(0, n, tc.batch_size)):
                self.last_losses = self.trainer.step(own, enemy, policy, z, perm[lo:lo + tc.batch_size], self.lr, sync=False)
                if tc.logging_per_steps and batch % tc.logging_per_steps == 0:   # (the only wait for the device in a step)
                    pl, vl = (float(x) for x in self.last_losses)
                    logger.debug(f"epoch {self.epoch_counter - 1} batch {batch}: policy loss {pl:.4f}, value loss {vl:.4f}")
                for cb in callbacks:
                    cb.on_batch_end(batch)
        return (n // tc.batch_size) * epochs

    def _on_device(self, perm):
        import torch
        return torch.from_numpy(perm.astype(np.int32 if self.backend == "hip" else np.int64)).to(self.trainer.device)

    def _resident_dataset(self):
        if self._resident is None:
            from ..agent.trainer import _tensor
            self._resident = tuple(_tensor(a, self.trainer.device) for a in self.dataset)
        return self._resident

    # ---- learning rate (optimize.py:87-114) ------------------------------------------------------------------------------------
    def update_learning_rate(self, total_steps):
        lr = self.decide_learning_rate(total_steps)
        if lr:
            self.lr = lr
            logger.debug(f"total step={total_steps}, set learning rate to {lr}")

    def decide_learning_rate(self, total_steps):
        ret = None
        path = getattr(self.config.resource, "force_learing_rate_file", None)
        if path and os.path.exists(path):
            try:
                with open(path, "rt") as f:
                    ret = float(str(f.read()).strip())
                    if ret:
                        logger.debug(f"loaded lr from force learning rate file: {ret}")
                        return ret
            except ValueError:
                pass
        for step, lr in self.config.trainer.lr_schedules:
            if total_steps >= step:
                ret = lr
        return ret

    # ---- models (optimize.py:116-123,147-163) ---------------------------------------------------------------------------------
    def save_current_model(self):
        rc = self.config.resource
        model_id = datetime.now().strftime("%Y%m%d-%H%M%S.%f")
        model_dir = os.path.join(rc.next_generation_model_dir, rc.next_generation_model_dirname_tmpl % model_id)
        os.makedirs(model_dir, exist_ok=True)
        config_path = os.path.join(model_dir, rc.next_generation_model_config_filename)
        weight_path = os.path.join(model_dir, rc.next_generation_model_weight_filename)
        if self.trainer is not None:
            self.model.model = self.trainer.to_net()
        self.model.save(config_path, weight_path)
        return model_dir

    def load_model(self):
        model = ReversiModel(self.config)
        rc = self.config.resource
        dirs = get_next_generation_model_dirs(rc)
        if not dirs:
            logger.debug("loading best model")
            if not load_best_model_weight(model):
                raise RuntimeError("Best model can not loaded!")
        else:
            logger.debug("loading latest model")
            config_path = os.path.join(dirs[-1], rc.next_generation_model_config_filename)
            weight_path = os.path.join(dirs[-1], rc.next_generation_model_weight_filename)
            if not model.load(config_path, weight_path):
                raise RuntimeError(f"the newest next-generation model in {dirs[-1]} can not be loaded")
        return model

    # ---- data (optimize.py:125-212) --------------------------------------------------------------------------------------------
    @property
    def dataset_size(self):
        return 0 if self.dataset is None else len(self.dataset[0])

    def load_play_data(self):
        if self.replay is not None:
            if self._replay_version != self.replay.version:
                logger.debug("taking the training dataset from the device replay")
                self.dataset = self._resident = self.replay.dataset()   # device tensors, as they are: no host copy
                self._replay_version = self.replay.version
            return
        filenames = get_game_data_filenames(self.config.resource)
        updated = False
        for filename in filenames:
            if filename in self.loaded_filenames:
                continue
            updated |= self.load_data_from_file(filename)
        for filename in (self.loaded_filenames - set(filenames)):
            self.unload_data_of_file(filename)
            updated = True
        if updated:
            logger.debug("updating training dataset")
            self.dataset = self.collect_all_loaded_data()
            self._resident = None

    def load_data_from_file(self, filename):
        try:
            logger.debug(f"loading data from {filename}")
            self.loaded_data[filename] = self.convert_to_training_data(read_game_data_from_file(filename))
            self.loaded_filenames.add(filename)
            return True
        except Exception as e:   # a file the self-play worker is still writing, or a damaged one: skipped, tried again next round
            logger.warning(f"{filename}: {e}")
            return False

    def unload_data_of_file(self, filename):
        logger.debug(f"removing data about {filename} from training set")
        self.loaded_filenames.remove(filename)
        self.loaded_data.pop(filename, None)
        self.training_count_of_files.pop(filename, None)

    def collect_all_loaded_data(self):
        parts = [self.loaded_data[f] for f in sorted(self.loaded_data)]
        if not parts:
            return None
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def count_up_training_count_and_delete_self_play_data_files(self):
        limit = self.config.trainer.delete_self_play_after_number_of_training
        if not limit or self.replay is not None:   # (a replay keeps its own window: there are no files of it to delete)
            return
        for filename in self.loaded_filenames:
            self.training_count_of_files[filename] += 1
            if self.training_count_of_files[filename] >= limit and os.path.exists(filename):
                try:
                    logger.debug(f"remove {filename}")
                    os.remove(filename)
                except Exception as e:
                    logger.warning(e)

    @staticmethod
    def convert_to_training_data(data):
        """Rows [[own, enemy], policy64, z] -> the packed arrays (the planes are formed on the device, by the stem kernel)."""
        return pack_game_data(data)


class PerStepCallback:
    """optimize.py:234-256: every `per_step` batches call `callback` (save the model), then sleep wait_after_save_model_ratio
    x the time since the last wait - the reference's way of leaving the GPU to the self-play worker."""

    def __init__(self, per_step, callback, wait_after_save_model_ratio=None):
        self.per_step = per_step
        self.step = 0
        self.callback = callback
        self.wait_after_save_model_ratio = wait_after_save_model_ratio
        self.last_wait_time = time()

    def on_batch_end(self, batch, logs=None):
        self.step += 1
        if self.step % self.per_step == 0:
            self.callback()
            self.wait()

    def wait(self):
        if self.wait_after_save_model_ratio:
            time_spent = time() - self.last_wait_time
            logger.debug(f"start sleeping {time_spent} seconds")
            sleep(time_spent * self.wait_after_save_model_ratio)
            logger.debug("finish sleeping")
            self.last_wait_time = time()
