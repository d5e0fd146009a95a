"""CPU: the kernels of raz_solve_batch (csrc/raz_solver_batch.hip) on the wave emulator - tests/native/libraz_emu_solver.so, the
emulator's Makefile with the kernel list given on the command line - against the yardsticks of tests/solver_batch_cases.py at the
emulator's sizes, and the host-side contract of the two entry points on the real library (no GPU here: RAZ_EDEVICE).  The emulator
also checks what the hardware does not: that every cross-lane operation of the leaf kernel is reached by all lanes of its wave."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import solver_batch_cases as C
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
EMU_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_solver.so")
EMU_LIB_LAST2 = os.path.join(ROOT, "tests", "native", "libraz_emu_solver_last2.so")   # (the same kernels with -DRAZ_SOLVER_INLINE_LAST=2)


def _build(out, extra=""):
    """The emulator's Makefile, untouched, run in a private COPY of its directory beside it (the same depth, so every relative path
    of the Makefile and of the sources still holds): its rule keeps intermediates (orc_*.o) beside itself and removes them at the
    end, so a build in the shared directory could take them from under another worker's build of another emulator library.
    (copytree keeps the time stamps: an up-to-date library is not rebuilt.)"""
    with _locked("emu_solver"), tempfile.TemporaryDirectory(prefix="wave_emu_solver.", dir=os.path.dirname(EMU_DIR)) as work:
        shutil.copytree(EMU_DIR, work, ignore=shutil.ignore_patterns("*.o", "_net", "_full"), dirs_exist_ok=True)
        r = subprocess.run(["make", "-C", work, "OUT=../" + os.path.basename(out), "EXTRA=" + extra,
                            "KERNELS=$(CSRC)/raz_solver_batch.hip $(CSRC)/raz_capi.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from reversi_alpha_zero_amd import _native as N
    lib = ctypes.CDLL(out)
    for name in ("raz_last_error", "raz_solve_batch", "raz_solve_batch_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def emu():
    return _build(EMU_LIB)


def _aligned(nbytes):
    buf = np.zeros(nbytes + 256, dtype=np.uint8)
    off = (-buf.ctypes.data) % 256
    return buf, buf[off:off + nbytes]


def solve(lib, cases, exactly, tuning=0, ws_bytes=None, max_empties=10, expect=C.RAZ_OK):
    """(move, score, status) of the cases on the emulated kernels; outputs start as 0x55 so that an untouched byte shows."""
    b, w, p = C.arrays(cases)
    n = len(cases)
    mv, sc, st = np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.uint8)
    ws_bytes = lib.raz_solve_batch_workspace_bytes(n, max_empties) if ws_bytes is None else ws_bytes
    keep, ws = _aligned(max(ws_bytes, 1))
    rc = lib.raz_solve_batch(b.ctypes.data, w.ctypes.data, p.ctypes.data, n, int(exactly), mv.ctypes.data, sc.ctypes.data, st.ctypes.data,
                             ws.ctypes.data, ws_bytes, tuning, None)
    assert rc == expect, (rc, (lib.raz_last_error() or b"").decode())
    return mv, sc, st


@pytest.mark.parametrize("exactly", [0, 1])
def test_golden_and_random_positions(emu, exactly):
    """G at <= 8 empties plus four of 10, R(1..8) at 16 positions each: one batch per list and mode."""
    for name, cases in C.emu_lists().items():
        C.assert_answers(solve(emu, cases, exactly), cases, exactly, name)


def test_status_rows(emu):
    cases = C.status_cases()
    assert sorted({c[3] for c in cases}) == [1, 2, 3]
    for exactly in (0, 1):
        C.assert_answers(solve(emu, cases, exactly), cases, exactly, "status rows")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(emu, n):
    """The mixed list - neighbouring lanes differ in depth, status rows in between - cycled to n rows: every answer is the
    position's own (its answer alone: the oracle's), rows beside refused rows included."""
    cases = C.cycled(C.mixed_list(), n)
    for exactly in (0, 1):
        C.assert_answers(solve(emu, cases, exactly), cases, exactly, f"n={n}")


def test_a_13_empties_position_is_split_five_plies(emu):
    """The first position of the 13/14-empties fixture in win/loss mode: five plies of expansion and fold around the leaf tasks.
    (The whole fixture, and the full scan, are the GPU's: on the emulator they take minutes.)"""
    cases = C.deep_cases()[:1]
    assert 64 - bin(cases[0][0] | cases[0][1]).count("1") == 13
    C.assert_answers(solve(emu, cases, 0, max_empties=13), cases, 0, "deep")


def test_n_zero_is_ok_and_launches_nothing(emu):
    assert emu.raz_solve_batch(None, None, None, 0, 1, None, None, None, None, 0, 0, None) == C.RAZ_OK


@pytest.mark.parametrize("exactly", [0, 1])
def test_partition_independence(emu, exactly):
    """65 rows of the mixed list (empties 1..10) under every tuning there is - no split, every number of split plies at the default
    and at the smallest leaf size, every leaf size, a chunk of one row, the minimum workspace and twice it: byte-identical to
    tuning = 0, which is right."""
    cases = C.mixed_list(65)
    least = emu.raz_solve_batch_workspace_bytes(len(cases), 10)
    base = solve(emu, cases, exactly, ws_bytes=4 * least)
    C.assert_answers(base, cases, exactly, "tuning 0")
    variants = [(C.TUNE_SPLIT(p), None) for p in range(0, 7)] + [(C.TUNE_SPLIT(p) | C.TUNE_LEAF(2), None) for p in range(1, 7)]
    variants += [(C.TUNE_LEAF(k), None) for k in range(2, 9)]
    variants += [(C.TUNE_CHUNK(1), None), (C.TUNE_CHUNK(7) | C.TUNE_LEAF(3), None), (0, least), (0, 2 * least)]
    for tuning, ws_bytes in variants:
        got = solve(emu, cases, exactly, tuning=tuning, ws_bytes=ws_bytes)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), (hex(tuning), ws_bytes, exactly)


def test_two_squares_finished_in_the_move_function(emu):
    """RAZ_SOLVER_INLINE_LAST=2 (csrc/raz_solver_search.h: solver_play finishes positions of TWO empty squares with the reference's
    loop and its non-exact stop) is the batch solver's option too, since it shares the pool's move function - k_sb_expand then makes
    values of such children, in the call's mode (only a split down to a leaf size of 2 or 3 gets there).  The kernels built with
    it, in a library of their own: the golden and random lists, and 65 rows of the mixed list as they come and split down to 2
    empties, in both modes - equal to the yardsticks and byte-identical to the default build."""
    last2 = _build(EMU_LIB_LAST2, "-DRAZ_SOLVER_INLINE_LAST=2")
    runs = [(name, cases, 0) for name, cases in C.emu_lists().items()] + [("mixed", C.mixed_list(65), t) for t in (0, C.TUNE_LEAF(2))]
    for exactly in (0, 1):
        for name, cases, tuning in runs:
            got, base = solve(last2, cases, exactly, tuning=tuning), solve(emu, cases, exactly, tuning=tuning)
            C.assert_answers(got, cases, exactly, f"{name}, tuning {tuning:#x} (two squares in the move function)")
            for a, b in zip(got, base):
                assert a.tobytes() == b.tobytes(), (name, hex(tuning), exactly)


def test_workspace_and_tuning_edges(emu):
    cases = C.cycled(C.mixed_list(), 65)
    n = len(cases)
    assert emu.raz_solve_batch_workspace_bytes(n, 15) == 0 and emu.raz_solve_batch_workspace_bytes(n, 14) > 0
    assert emu.raz_solve_batch_workspace_bytes((1 << 31) + 1, 4) == 0
    sizes = [emu.raz_solve_batch_workspace_bytes(n, e) for e in range(0, 15)]
    assert sizes == sorted(sizes)
    least = sizes[10]   # (the list's deepest row has 10 empties)
    C.assert_answers(solve(emu, cases, 1, ws_bytes=least), cases, 1, "minimum workspace")
    for short in (least - 1, sizes[0] - 1):
        got = solve(emu, cases, 1, ws_bytes=short, expect=C.RAZ_EINVAL)
        assert all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got), "an output byte was written"
    for bad in (1 << 24, 1 << 31, C.TUNE_LEAF(1), C.TUNE_LEAF(9), C.TUNE_SPLIT(7)):
        got = solve(emu, cases, 1, tuning=bad, expect=C.RAZ_EINVAL)
        assert all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)


def test_size_query_on_the_real_library():
    """raz_solve_batch_workspace_bytes needs no device: it refuses 15 empties and too many rows, and grows with both arguments."""
    from reversi_alpha_zero_amd import _native as N
    lib = N.lib
    assert lib.raz_solve_batch_workspace_bytes(100, 15) == 0 and lib.raz_solve_batch_workspace_bytes((1 << 31) + 1, 14) == 0
    assert 0 < lib.raz_solve_batch_workspace_bytes(100, 0) < lib.raz_solve_batch_workspace_bytes(100, 14) < lib.raz_solve_batch_workspace_bytes(100000, 14)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a machine without a GPU")
def test_without_a_gpu_the_call_is_a_device_error():
    """The real library on a machine without a GPU: RAZ_EDEVICE, like every other device entry point."""
    from reversi_alpha_zero_amd import _native as N
    lib = N.lib
    need = lib.raz_solve_batch_workspace_bytes(100, 14)
    fake = 1 << 20   # (never dereferenced: the first HIP call fails)
    rc = lib.raz_solve_batch(fake, fake, fake, 100, 1, fake, fake, fake, fake, need, 0, None)
    assert rc == C.RAZ_EDEVICE, (rc, N.last_error())
