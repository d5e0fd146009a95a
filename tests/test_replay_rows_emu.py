"""CPU: the kernels of raz_train_rows_count / raz_train_rows_fill (csrc/raz_replay.hip) on the wave emulator -
tests/native/libraz_emu_replay.so, the emulator's Makefile with the kernel list given on the command line - on the outboxes of
tests/replay_cases.py, whose two expectations must first agree with each other; and the host-side contract of the two entries on the
real library (refusals before any launch; no GPU here: RAZ_EDEVICE).  The emulator also checks what the hardware does not: that
every ballot, shuffle and reduction of the kernels is reached by all lanes of its wave."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import replay_cases as C
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
EMU_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_replay.so")
NAMES = ("raz_last_error", "raz_train_rows_count", "raz_train_rows_fill")


def _build(out):
    """The emulator's Makefile, untouched, run in a private COPY of its directory beside it (see tests/test_solver_batch_emu.py)."""
    with _locked("emu_replay"), tempfile.TemporaryDirectory(prefix="wave_emu_replay.", dir=os.path.dirname(EMU_DIR)) as work:
        shutil.copytree(EMU_DIR, work, ignore=shutil.ignore_patterns("*.o", "_net", "_full"), dirs_exist_ok=True)
        r = subprocess.run(["make", "-C", work, "OUT=../" + os.path.basename(out),
                            "KERNELS=$(CSRC)/raz_replay.hip $(CSRC)/raz_capi.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from reversi_alpha_zero_amd import _native as N
    lib = ctypes.CDLL(out)
    for name in NAMES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def emu():
    return _build(EMU_LIB)


MEM = C.HostMemory()


@pytest.mark.parametrize("name", C.case_names())
def test_the_two_expectations_agree(name):
    """rows_of_game + saved_policy + pack_game_data against the native text read back with json: no kernel involved."""
    case = C.case_by_name(name)
    C.assert_same_rows(C.expected_python(case), C.expected_text(case), name)


def test_the_cases_hold_what_they_are_for():
    """The ply-axis sets have their empty, clamped, row-less and one-sided games; the f64 division is pinned (the same quotient in
    f32 has other bits); the big counts pass 2^32; the game axis crosses the scan's block three times."""
    for plies in C.PLY_AXIS:
        case = C.ply_axis_case(plies)
        n_plies = case["summary"]["n_plies"].tolist()
        assert {0, 1, max(plies - 1, 0), plies} <= set(n_plies) and max(n_plies) > plies
        rows = np.diff(C.expected(case)[4].astype(np.int64))
        assert (rows == 0).sum() >= 2 and rows.max() == 8 * plies   # (n_plies 0 and the row-less game; the clamped game is full)
        assert any(int(a) == -1 for a in case["headers"]["action"].reshape(-1))
    a, b = C.F32_DIVISION_DIFFERS
    assert np.float32(a) / np.float32(a + b) != np.float32(a / (a + b))
    assert int(C.counts_case()["root_n"][1, 0].astype(np.uint64).sum()) > 2 ** 32
    exp = C.expected(C.counts_case())
    assert (exp[2][:8] == 1.0).sum() == 8 and (exp[2][:8] == 0.0).sum() == 8 * 63   # one visited square: p = 1.0 exactly
    assert max(C.GAME_AXIS) >= 3 * C.SCAN_BLOCK
    for kind in (None, "holes"):
        case = C.game_axis_case(257, kind)
        assert (case["done"] is None) == (kind is None)
    d = C.game_axis_case(1025, "holes")["done"]
    assert d[0] == 0 and d[-1] == 0 and d[len(d) // 2] == 0 and d[1] == 1
    # the 8 symmetries of a row are 8 different rows (boards and policies are asymmetric)
    exp = C.expected(C.ply_axis_case(2))
    first = [(int(exp[0][i]), int(exp[1][i]), exp[2][i].tobytes()) for i in range(8)]
    assert len(set(first)) == 8
    z = C.expected(C.winner_case())[3]
    assert {-1, 0, 1} == set(z.tolist())


@pytest.mark.parametrize("name", C.case_names())
def test_rows_on_the_emulator(emu, name):
    C.check_case(emu, MEM, C.case_by_name(name))


@pytest.mark.parametrize("name", ["plies=65", "games=257,done=holes"])
def test_capacity_on_the_emulator(emu, name):
    """capacity_rows equal to the total: everything; 8 and 1 below it: the rows below the capacity, and not one byte from it on."""
    case = C.case_by_name(name)
    total = int(C.expected(case)[4][-1])
    assert total > 16
    for cap in (total, total - 8, total - 1, total + 5, 0):
        assert C.check_case(emu, MEM, case, capacity=cap) == min(cap, total)


def test_the_total_is_optional_and_no_games_is_ok(emu):
    C.check_case(emu, MEM, C.case_by_name("plies=2"), host_total=False)
    off = np.full(3, 0x55555555, dtype=np.uint32)
    total = ctypes.c_uint64(99)
    assert emu.raz_train_rows_count(None, None, None, 0, 3, off.ctypes.data, ctypes.byref(total), None) == C.RAZ_OK
    assert off.tolist() == [0, 0x55555555, 0x55555555] and total.value == 0
    assert emu.raz_train_rows_fill(None, None, None, None, 0, 3, 4, 1, off.ctypes.data, 0, None, None, None, None, None) == C.RAZ_OK


def _refusals(lib):
    a = 1 << 20   # (an aligned address that is never dereferenced: every call below is refused before anything is launched)
    ok_count = dict(h=a, s=a, d=None, g=4, p=3, off=a)
    ok_fill = dict(h=a, rn=a, s=a, d=None, g=4, p=3, off=a, cap=100, own=a, enemy=a, pol=a, z=a)

    def count(**kw):
        k = dict(ok_count, **kw)
        return lib.raz_train_rows_count(k["h"], k["s"], k["d"], k["g"], k["p"], k["off"], None, None)

    def fill(**kw):
        k = dict(ok_fill, **kw)
        return lib.raz_train_rows_fill(k["h"], k["rn"], k["s"], k["d"], k["g"], k["p"], 4, 1, k["off"], k["cap"], k["own"], k["enemy"], k["pol"],
                                       k["z"], None)
    bad_count = [dict(h=None), dict(s=None), dict(off=None), dict(h=a + 4), dict(s=a + 4), dict(off=a + 2), dict(p=0),
                 dict(g=1 << 20, p=512), dict(g=(1 << 29) // 3 + 1, p=3)]
    bad_fill = [dict(h=None), dict(rn=None), dict(s=None), dict(off=None), dict(own=None), dict(enemy=None), dict(pol=None), dict(z=None),
                dict(h=a + 4), dict(rn=a + 2), dict(s=a + 4), dict(off=a + 2), dict(own=a + 4), dict(enemy=a + 4), dict(pol=a + 2), dict(p=0),
                dict(g=1 << 20, p=512), dict(g=(1 << 29) // 3 + 1, p=3)]
    for kw in bad_count:
        assert count(**kw) == C.RAZ_EINVAL and b"raz_train_rows_count" in lib.raz_last_error(), kw
    for kw in bad_fill:
        assert fill(**kw) == C.RAZ_EINVAL and b"raz_train_rows_fill" in lib.raz_last_error(), kw
    return count, fill


def test_refusals_on_the_emulated_library(emu):
    _refusals(emu)


def test_refusals_on_the_real_library():
    from reversi_alpha_zero_amd import _native as N
    _refusals(N.lib)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a machine without a GPU")
def test_without_a_gpu_the_calls_are_device_errors():
    """The real library on a machine without a GPU: RAZ_EDEVICE, like every other device entry point."""
    from reversi_alpha_zero_amd import _native as N
    count, fill = _refusals(N.lib)
    assert count() == C.RAZ_EDEVICE, N.last_error()
    assert fill() == C.RAZ_EDEVICE, N.last_error()
    assert count(g=0) == C.RAZ_EDEVICE, N.last_error()   # (d_row_offset[0] = 0 is device work too)
