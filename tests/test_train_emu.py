"""CPU: raznet-train-v1's kernels - csrc/raz_train.hip as it stands, compiled for the host against the wave emulator
(tests/native/wave_emu -> tests/native/libraz_emu_train.so) - through tests/emu_util.py's EmuTrainer, held to the rules and run
through the scenarios of tests/train_cases.py, the same ones tests/test_train_gpu.py runs on the device.  The GPU tests remain the
tests of record (the emulator's double exp / log / tanh / sqrt are libm's; no bits are carried from one driver to the other); this
file is what tells a pull request without an MI355X that a training kernel's indexing, guards, launch sizes or summation order
broke.  Shapes are the ones a CPU can afford: the mini net at every batch edge, 32x2 at three, the width and head edges
(48, 80 channels, value_fc_size 256), a batch of 257 rows.  RAZ_TRAIN_ACCURACY_JSON=<path> appends the measured ratios.

Measured on the build container, one process: 92 s for the 50 tests, 5 s of it the library's build - 31 s the seven steps in two
trainers at 32x2 (test_the_batch_size_alone_fixes_the_bytes), 14 s the two trainers of 32x2 at 33 rows, 7 s each the rules at
80 channels x 33 rows and the eight steps at 67 rows; every other test takes 3 s or less."""
import numpy as np
import pytest

import emu_util
import train_cases as tc

CASES = [(16, 1, 16, B) for B in tc.BATCHES] + [(32, 2, 7, B) for B in (1, 5, 33)]
EDGE_CASES = [(F, R, V, B) for (F, R, V) in tc.EDGE_SHAPES for B in tc.EDGE_BATCHES]


class _Raw:
    """The raw C entries on host memory (tests/train_cases.py, the module docstring)."""
    stream = staticmethod(lambda: None)
    sync = staticmethod(lambda: None)

    @property
    def lib(self):
        return emu_util.load_train()

    def last_error(self):
        return (self.lib.raz_last_error() or b"").decode()

    def alloc(self, nbytes):
        keep, ptr = emu_util.aligned(nbytes)
        return tc.Buf(ptr, keep, lambda: keep.copy())

    def put(self, a):
        a = np.array(a, copy=True, order="C")
        return tc.Buf(a.ctypes.data, a, lambda: a.copy())


def make(net, max_batch):
    return emu_util.EmuTrainer(net, max_batch, l2=tc.L2)


make.driver = "emu"
make.raw = _Raw()


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_forward_in_training_mode(F, R, V, B):
    tc.forward_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_gradients_tensor_by_tensor(F, R, V, B):
    tc.gradient_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


@pytest.mark.parametrize("B", tc.LONG_BATCHES)
def test_both_rules_on_a_batch_longer_than_256(B):
    c = tc.case(make, 16, 1, 16, B, rows="long")
    tc.forward_rule(make, c, (16, 1, 16, B))
    tc.gradient_rule(make, c, (16, 1, 16, B))


def test_degenerate_values():
    c = tc.case(make, 16, 1, 16, 33, rows="degenerate")
    tc.degenerate_guards_and_exact_values(make, c)
    tc.forward_rule(make, c, (16, 1, 16, 33, "degenerate"), guards=False)
    tc.gradient_rule(make, c, (16, 1, 16, 33, "degenerate"))


@pytest.mark.parametrize("F,R,V,B", [(16, 1, 16, 5), (16, 1, 16, 67)])
def test_eight_steps_track_the_f64_trainer(F, R, V, B):
    tc.eight_steps_track_the_f64_trainer(make, F, R, V, B)


def test_two_trainers_hold_the_same_bytes():
    tc.two_trainers_hold_the_same_bytes(make, 32, 2, 7, B=33)   # one row past the 32 splits; 67 rows cost the CPU twice the time


@pytest.mark.parametrize("F,R,V", [(16, 1, 16), (32, 2, 7)])
def test_the_batch_size_alone_fixes_the_bytes(F, R, V):
    tc.the_batch_size_alone_fixes_the_bytes(make, F, R, V)


def test_abi_guards_refuse_and_leave_the_state_untouched():
    tc.abi_guards_refuse_and_leave_the_state_untouched(make)


def test_reads_are_refused_before_a_step_and_at_a_wrong_size():
    tc.reads_are_refused_before_a_step_and_at_a_wrong_size(make)
