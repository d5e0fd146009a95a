"""CPU: raznet-train-v2 (precision "f16x3": the trunk's three 3x3 products on the f16 matrix cores over split operands,
csrc/raz_train_f16x3.h) on the wave emulator, through the scenarios and rules of tests/train_cases.py with v2's constants
(tests/train_f16x3_util.py) - the twin of tests/test_train_emu.py, which stays the test of v1.  The emulator adds the 16 products
of a matrix instruction in k order, the device in an order of its own: the GPU file is the test of record, this one tells a pull
request without an MI355X that an index, a guard, a scale or a summation order broke.  RAZ_TRAIN_ACCURACY_JSON=<path> appends the
measured ratios (driver "emu-f16x3").

One process takes about 250 s for the 44 tests (v1's twin: 92 s): an emulated 32x32x16 matrix instruction costs 16 k multiply-adds
and a rendezvous of 64 fibers, and a product issues three.  The shapes are the ones asked of this file; the long ones are the seven
steps in two trainers at 32x2 (74 s), the two trainers of 32x2 at 33 rows (34 s), the eight steps at 67 rows (28 s) and the rules
at 80 channels x 33 rows (22 s); every other test takes 14 s or less."""
import numpy as np
import pytest

import train_cases as tc
import train_f16x3_util as v2

make = v2.make_emu
CASES = [(16, 1, 16, B) for B in tc.BATCHES] + [(32, 2, 7, B) for B in (1, 5, 33)]
EDGE_CASES = [(F, R, V, B) for (F, R, V) in [(48, 1, 16), (80, 1, 7)] for B in (3, 5, 33)]


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
    """The scale rule on tensors it could trip over: a channel that is constant over the batch, one whose gradient is exactly 0,
    heads 40 times as sharp."""
    c = tc.case(make, 16, 1, 16, 33, rows="degenerate")
    tc.degenerate_guards_and_exact_values(make, c)
    tc.forward_rule(make, c, (16, 1, 16, 33, "degenerate"), guards=False)
    tc.gradient_rule(make, c, (16, 1, 16, 33, "degenerate"))


@pytest.mark.parametrize("F,R,V,B", [(16, 1, 16, 5), (16, 1, 16, 67)])
def test_eight_steps_track_the_f64_trainer(F, R, V, B):
    tc.eight_steps_track_the_f64_trainer(make, F, R, V, B)


def test_two_trainers_hold_the_same_bytes():
    tc.two_trainers_hold_the_same_bytes(make, 32, 2, 7, B=33)


@pytest.mark.parametrize("F,R,V", [(16, 1, 16), (32, 2, 7)])
def test_the_batch_size_alone_fixes_the_bytes(F, R, V):
    tc.the_batch_size_alone_fixes_the_bytes(make, F, R, V)


def test_v2_differs_from_v1_in_the_trunk_and_reads_its_precision_back():
    lib = v2.make_emu.raw.lib
    v2.trunk_differs_and_precisions_read_back(make, lambda net, mb: v2.EmuTrainerF32Via2(net, mb, l2=tc.L2),
                                              lambda t: lib.raz_trainer_precision(t.handle))


def test_precision_0_through_the_new_entries_is_v1_to_the_byte():
    """raz_trainer_bytes2 / _create2 at RAZ_TRAIN_F32 against raz_trainer_bytes / _create: the same workspace size, the same state
    after two steps."""
    import emu_util
    lib = v2.make_emu.raw.lib
    assert lib.raz_trainer_bytes2(32, 2, 7, 33, 0) == lib.raz_trainer_bytes(32, 2, 7, 33)
    assert lib.raz_trainer_bytes2(32, 2, 7, 33, 1) > lib.raz_trainer_bytes(32, 2, 7, 33)
    net, blobs = tc.make_net(16, 1, 16), []
    for cls in (v2.EmuTrainerV1Entry, v2.EmuTrainerF32Via2):
        t = cls(net, 5, l2=tc.L2)
        for step in range(2):
            t.step(*tc.data(), tc.batch_rows(5, salt=step), 1e-2)
        blobs.append(t.get_blob())
        t.close()
    assert np.array_equal(blobs[0].view(np.uint32), blobs[1].view(np.uint32))


def test_one_row_dominates_the_output_gradients(monkeypatch):
    v2.skewed_gradients_meet_the_rule(make, monkeypatch)
