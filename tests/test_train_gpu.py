"""raznet-train-v1 on the device (csrc/raz_train.hip through agent/trainer.py's DeviceTrainer) against the f64 restatement, tensor by
tensor - the rules and the scenarios are in tests/train_cases.py, which tests/test_train_emu.py runs on the wave emulator too.
RAZ_TRAIN_ACCURACY_JSON=<path> appends the measured ratios of every case."""
import numpy as np
import pytest
import torch

import train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(F, R, V, B) for (F, R, V) in tc.SHAPES for B in tc.BATCHES]
EDGE_CASES = [(F, R, V, B) for (F, R, V) in tc.EDGE_SHAPES for B in tc.EDGE_BATCHES]


def _native():
    from reversi_alpha_zero_amd import _native as N
    return N


class _Raw:
    """The raw C entries on device memory (tests/train_cases.py, the module docstring)."""
    lib = property(lambda self: _native().lib)

    def stream(self):
        return _native().current_stream_ptr()

    def last_error(self):
        return _native().last_error()

    def alloc(self, nbytes):
        t = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        return tc.Buf(t.data_ptr(), t, lambda: t.cpu().numpy())

    def put(self, a):
        from reversi_alpha_zero_amd.agent.trainer import _tensor
        t = _tensor(a, torch.device(DEV))
        return tc.Buf(t.data_ptr(), t, lambda: t.cpu().numpy())

    def sync(self):
        torch.cuda.synchronize()


def make(net, max_batch):
    from reversi_alpha_zero_amd.agent.trainer import DeviceTrainer
    return DeviceTrainer(net, max_batch=max_batch, device=DEV, l2=tc.L2)


make.driver = "gpu"
make.raw = _Raw()


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_forward_in_training_mode(F, R, V, B):
    tc.forward_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


@pytest.mark.parametrize("F,R,V,B", CASES + EDGE_CASES)
def test_gradients_tensor_by_tensor(F, R, V, B):
    tc.gradient_rule(make, tc.case(make, F, R, V, B), (F, R, V, B))


@pytest.mark.parametrize("B", tc.LONG_BATCHES)
def test_both_rules_on_a_batch_longer_than_256(B):
    """The strided loop of k_loss_sum and more than eight positions per split of k_twgrad (tests/train_cases.py, long_batch_rows)."""
    c = tc.case(make, 16, 1, 16, B, rows="long")
    tc.forward_rule(make, c, (16, 1, 16, B))
    tc.gradient_rule(make, c, (16, 1, 16, B))


def test_degenerate_values():
    """A channel with variance exactly 0, a ReLU that never passes, a saturated softmax and tanh at +-1 (tests/train_cases.py,
    degenerate_net): both rules with their constants unchanged, and the values that are exact."""
    c = tc.case(make, 16, 1, 16, 33, rows="degenerate")
    tc.degenerate_guards_and_exact_values(make, c)
    tc.forward_rule(make, c, (16, 1, 16, 33, "degenerate"), guards=False)
    tc.gradient_rule(make, c, (16, 1, 16, 33, "degenerate"))


@pytest.mark.parametrize("F,R,V,B", [(16, 1, 16, 5), (16, 1, 16, 67), (128, 1, 64, 5), (128, 1, 64, 67)])
def test_eight_steps_track_the_f64_trainer(F, R, V, B):
    tc.eight_steps_track_the_f64_trainer(make, F, R, V, B)


def test_two_trainers_hold_the_same_bytes():
    tc.two_trainers_hold_the_same_bytes(make, 128, 1, 64)


@pytest.mark.parametrize("F,R,V", [(16, 1, 16), (32, 2, 7), (128, 1, 64)])
def test_the_batch_size_alone_fixes_the_bytes(F, R, V):
    tc.the_batch_size_alone_fixes_the_bytes(make, F, R, V)


def test_abi_guards_refuse_and_leave_the_state_untouched():
    tc.abi_guards_refuse_and_leave_the_state_untouched(make)


def test_reads_are_refused_before_a_step_and_at_a_wrong_size():
    tc.reads_are_refused_before_a_step_and_at_a_wrong_size(make)
