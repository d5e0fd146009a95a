"""The WAVE-EMULATOR builds of the kernels (tests/native/wave_emu -> tests/native/libraz_emu*.so) - the C ABI (include/raz.h) on host
memory - as _native.Backend instances, and the product's own wrappers on them: EmuEngine is engine.SelfPlayEngine, EmuTrainer is
agent/trainer.py's DeviceTrainer, each with a constructor's choices and nothing else, so that csrc/raz_engine.hip AND engine.py can be
stepped and checked against the CPU oracle in a container without a GPU.  TEST INFRASTRUCTURE ONLY - the product never loads these
libraries, and the GPU parity tests (tests/test_engine_gpu.py ...) remain the tests of record; this is the debugging loop the build
container otherwise lacks."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT, _locked
from reversi_alpha_zero_amd._native import Backend
from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
from reversi_alpha_zero_amd.engine import DeviceNet, SelfPlayEngine

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
EMU_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu.so")
EMU_FULL_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_full.so")
EMU_TRAIN_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_train.so")
_backends = {}


def _zeros(nbytes, dtype, device):
    """What the emulator's backend allocates with: zero-filled (the emulated kernels have always started from np.zeros; the product's
    torch.empty hands the library whatever the heap held) and 256-byte aligned as the device allocator's blocks are."""
    import torch
    t = torch.zeros(nbytes + 256, dtype=dtype, device=device)
    off = -t.data_ptr() % 256
    return t[off:off + nbytes]


def backend(which=False):
    """The _native.Backend of one emulator library - what DeviceNet / DeviceTrainer take as backend=: stream NULL, no device guard.
    which=False: the tree kernels, leaves evaluated by the oracle's C net (libraz_emu.so, seconds to build).  True: the whole product
    incl. the real net kernels on emulated matrix cores (libraz_emu_full.so, a minute to build): what the fused tree + net kernel
    needs.  "train": the training kernels (csrc/raz_train.hip + raz_capi.hip, unchanged; libraz_emu_train.so, seconds to build)."""
    if which not in _backends:
        # RAZ_EMU_VARIANT=<name> RAZ_EMU_EXTRA=<flags>: a build of the tree kernels with other compile-time options, in a library of its own
        # (a child process of a test that wants the kernels' optional forms checked: tests/test_engine_emu.py)
        variant, extra = os.environ.get("RAZ_EMU_VARIANT"), os.environ.get("RAZ_EMU_EXTRA", "")
        if which == "train":
            path, args, lock = EMU_TRAIN_LIB, ["../libraz_emu_train.so"], "emu_train"
        elif which:
            path, args, lock = EMU_FULL_LIB, ["../libraz_emu_full.so"], "emu"
        elif variant:
            path, args, lock = os.path.join(ROOT, "tests", "native", f"libraz_emu_{variant}.so"), [f"OUT=../libraz_emu_{variant}.so", f"EXTRA={extra}"], f"emu_{variant}"
        else:
            path, args, lock = EMU_LIB, [], "emu"
        with _locked(lock):
            r = subprocess.run(["make", "-C", EMU_DIR] + args, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("wave-emulator build failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
        _backends[which] = Backend(ctypes.CDLL(path), host=True, empty=_zeros)
    return _backends[which]


def load(full=False):
    """The library itself (a ctypes.CDLL with _native.SIGNATURES applied), for the tests that call its entries directly."""
    return backend(bool(full)).lib


def load_train():
    return backend("train").lib


def aligned(nbytes, align=256):
    """(the array that owns the memory, an address in it aligned to `align` with nbytes behind it)"""
    a = np.zeros(nbytes + align, dtype=np.uint8)
    return a, (a.ctypes.data + align - 1) // align * align


class EmuEngine(SelfPlayEngine):
    """reversi_alpha_zero_amd.engine.SelfPlayEngine itself on the emulated kernels: a DeviceNet on the CPU with the emulator's
    backend, and the constructor choices the emulator tests were written against.  Every method is the product's."""

    def __init__(self, config, blob, n_games, seed=0, nodes_per_game=None, sims_hint=None, max_plies=72, record_root_w=True,
                 inner_max=0, force_slot_kernel=False, pool_bytes_per_game=0, fused=False, full_lib=False, **cfg_overrides):
        """fused: the tree + net kernel (raz_engine_config.reserved bit 4); it, and full_lib, run on the whole-product library.
        One stream, one part, record_root_w, and a pruned pool (232 B a node) of the product's whole-game node count, whatever the
        product would choose; cfg_overrides: further keywords of SelfPlayEngine (solver_pool_waves, solver_pool_every, ...)."""
        if nodes_per_game is None:
            s = sims_hint or config.play.simulation_num_per_move
            share = bool(config.play.share_mtcs_info_in_self_play)
            nodes_per_game = (s * max(1, config.play.thinking_loop) * 62 + 128) * (2 if share else 1)
        net = DeviceNet(blob, device="cpu", backend=backend(bool(fused or full_lib)))
        super().__init__(config, net, n_games, seed=seed, nodes_per_game=nodes_per_game, max_plies=max_plies, record_root_w=record_root_w,
                         single_stream=True, parts=1, inner_max=inner_max, force_slot_kernel=force_slot_kernel,
                         pool_bytes_per_game=pool_bytes_per_game, fused=fused, **cfg_overrides)


class EmuTrainer(DeviceTrainer):
    """agent/trainer.py's DeviceTrainer itself on the emulated training kernels (CPU tensors, stream NULL: the emulator runs every
    launch and copy to its end before it returns)."""

    def __init__(self, net, max_batch, l2=1e-4, precision="f32"):
        super().__init__(net, max_batch, device="cpu", l2=l2, precision=precision, backend=backend("train"))
