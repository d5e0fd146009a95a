"""GPU: raz_train_rows_count / raz_train_rows_fill (csrc/raz_replay.hip) on the outboxes of tests/replay_cases.py - the cases the
wave emulator runs in tests/test_replay_rows_emu.py, here on the hardware: every row bit for bit the row the play_*.json text gives,
row_offset numpy's cumsum, and not one byte written at or beyond capacity_rows."""
import ctypes

import numpy as np
import pytest
import torch

import replay_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from reversi_alpha_zero_amd import _native as N
    return N.lib


@pytest.fixture(scope="module")
def mem():
    return C.DeviceMemory(DEV)


@pytest.mark.parametrize("name", C.case_names())
def test_rows(lib, mem, name):
    C.check_case(lib, mem, C.case_by_name(name))


@pytest.mark.parametrize("name", ["plies=65", "games=257,done=holes"])
def test_capacity(lib, mem, name):
    case = C.case_by_name(name)
    total = int(C.expected(case)[4][-1])
    assert total > 16
    for cap in (total, total - 8, total - 1, total + 5, 0):
        assert C.check_case(lib, mem, case, capacity=cap) == min(cap, total)


def test_the_total_is_optional_and_no_games_is_ok(lib, mem):
    C.check_case(lib, mem, C.case_by_name("plies=2"), host_total=False)
    off = torch.full((3,), 0x55555555, dtype=torch.int32, device=DEV)
    total = ctypes.c_uint64(99)
    assert lib.raz_train_rows_count(None, None, None, 0, 3, off.data_ptr(), ctypes.byref(total), mem.stream) == C.RAZ_OK
    assert off.cpu().tolist() == [0, 0x55555555, 0x55555555] and total.value == 0
    assert lib.raz_train_rows_fill(None, None, None, None, 0, 3, 4, 1, off.data_ptr(), 0, None, None, None, None, mem.stream) == C.RAZ_OK


@pytest.mark.parametrize("name", ["plies=65", "games=1025,done=holes", "counts", "argmax,tau1=0"])
def test_rows_from_outbox(name):
    """The Python wrapper on device tensors shaped as SelfPlayEngine.pack_records hands them out."""
    from reversi_alpha_zero_amd.lib.replay import rows_from_outbox
    case = C.case_by_name(name)
    G, plies = len(case["summary"]), case["plies"]
    hdr = torch.from_numpy(case["headers"].view(np.uint8).reshape(G, plies, 48).copy()).to(DEV)
    rn = torch.from_numpy(case["root_n"].view(np.int32).copy()).to(DEV)
    sm = torch.from_numpy(case["summary"].view(np.uint8).reshape(G, 32).copy()).to(DEV)
    done = None if case["done"] is None else torch.from_numpy(case["done"].copy()).to(DEV)
    out = rows_from_outbox(hdr, rn, sm, done, change_tau_turn=case["change_tau_turn"], save_policy_of_tau_1=case["save_policy_of_tau_1"])
    assert all(t.is_cuda and t.is_contiguous() for t in out)
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.float32, torch.int8, torch.int32]
    got = (out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy().view(np.uint64), out[2].cpu().numpy(), out[3].cpu().numpy(),
           out[4].cpu().numpy().view(np.uint32))
    C.assert_same_rows(got, C.expected(case), name)
