"""CPU: the kernels of raz_solve_wld (csrc/raz_solver_wld.hip) on the wave emulator - tests/native/libraz_emu_solver_wld.so, the
emulator's Makefile with the kernel list given on the command line - against the yardsticks of tests/solver_wld_cases.py at the
emulator's sizes.  The emulator also checks what the hardware does not: that every cross-lane operation of the search kernel is
reached by all lanes of its wave."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import solver_wld_cases as W
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
EMU_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_solver_wld.so")
NAMES = ("raz_last_error", "raz_solve_wld", "raz_solve_wld_workspace_bytes")


def _build(out, extra=""):
    """As tests/test_solver_exact_emu.py builds its library: the Makefile, untouched, in a private copy of its directory."""
    with _locked("emu_solver_wld"), tempfile.TemporaryDirectory(prefix="wave_emu_solver_wld.", dir=os.path.dirname(EMU_DIR)) as work:
        shutil.copytree(EMU_DIR, work, ignore=shutil.ignore_patterns("*.o", "_net", "_full"), dirs_exist_ok=True)
        r = subprocess.run(["make", "-C", work, "OUT=../" + os.path.basename(out), "EXTRA=" + extra,
                            "KERNELS=$(CSRC)/raz_solver_wld.hip $(CSRC)/raz_capi.hip"],
                           capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from reversi_alpha_zero_amd import _native as N
    lib = ctypes.CDLL(out)
    for name in NAMES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def emu():
    return _build(EMU_LIB)


def _aligned(nbytes):
    buf = np.zeros(nbytes + 256, dtype=np.uint8)
    off = (-buf.ctypes.data) % 256
    return buf, buf[off:off + nbytes]


def solve(lib, cases, tuning=0, ws_bytes=None, max_empties=10, expect=W.RAZ_OK, visits=None):
    """(move, outcome, status) of the cases on the emulated kernels; outputs start as 0x55 so that an untouched byte shows."""
    b, w, p = W.arrays(cases)
    n = len(cases)
    mv, sc, st = np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.uint8)
    ws_bytes = lib.raz_solve_wld_workspace_bytes(n, max_empties) if ws_bytes is None else ws_bytes
    keep, ws = _aligned(max(ws_bytes, 1))
    rc = lib.raz_solve_wld(b.ctypes.data, w.ctypes.data, p.ctypes.data, n, mv.ctypes.data, sc.ctypes.data, st.ctypes.data,
                           ws.ctypes.data, ws_bytes, tuning, None)
    assert rc == expect, (rc, (lib.raz_last_error() or b"").decode())
    if visits is not None:
        visits.append(int(ws[:8].view(np.uint64)[0]))
    return mv, sc, st


def _untouched(got):
    return all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)


def test_golden_and_random_positions(emu):
    """G at <= 8 empties plus four of 10, R(1..8) at 16 positions each: one batch per list; the coverage conditions hold."""
    W.assert_wld_coverage(emu=True)
    for name, cases in W.emu_lists().items():
        W.assert_answers(solve(emu, cases), cases, 1, name)


def test_status_rows(emu):
    """One empty square more than the limit and the opening are refused, a root that must pass, a finished game and what is not a
    position answer as raz_solve_batch answers them.  (The 15-empties row that is solved here is the GPU's.)"""
    cases = W.status_cases(deep_row=False)
    assert sorted({c[3] for c in cases}) == [1, 2, 3]
    W.assert_answers(solve(emu, cases), cases, 1, "status rows")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(emu, n):
    cases = W.cycled(W.mixed_wld(deep_row=False), n)
    W.assert_answers(solve(emu, cases), cases, 1, f"n={n}")


def test_n_zero_is_ok_and_launches_nothing(emu):
    assert emu.raz_solve_wld(None, None, None, 0, None, None, None, None, 0, 0, None) == W.RAZ_OK


def test_partition_independence(emu):
    """The 257-row mixed list plus one 12-empties row (a parked stack several levels deep) under every tuning - leaf 2 with a budget of
    3 nodes, 0..6 plies, cuts off among them - the minimum workspace and twice it: byte-identical to tuning = 0, which is right."""
    cases = W.mixed_wld(257, deep_row=False) + W.random_cases(12)[:1]
    least = emu.raz_solve_wld_workspace_bytes(len(cases), 12)
    base = solve(emu, cases, ws_bytes=4 * least)
    W.assert_answers(base, cases, 1, "tuning 0")
    variants = [(t, None, name) for name, t in W.tunings().items()] + [(0, least, "minimum workspace"), (0, 2 * least, "twice the minimum")]
    for tuning, ws_bytes, name in variants:
        got = solve(emu, cases, tuning=tuning, ws_bytes=ws_bytes, max_empties=12)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), (name, hex(tuning), ws_bytes)


def test_a_parked_task_is_dropped_on_resume(emu):
    """Budget 3, 9-empties rows split 3 plies to leaf 4: every task parks many times, and tasks whose ancestor is decided while they
    are parked are dropped when they resume - the visit counter stays strictly below the run with cuts off, where every task
    runs to its end, and no task goes missing: the answers are right."""
    cases = W.random_cases(9, 4)
    tuning = W.TUNE_BUDGET[3] | W.TUNE_SPLIT(3) | W.TUNE_LEAF(4)
    for i, c in enumerate(cases):
        on, off = [], []
        W.assert_answers(solve(emu, [c], tuning=tuning, visits=on), [c], 1, f"cuts on, row {i}")
        W.assert_answers(solve(emu, [c], tuning=tuning | W.TUNE_NO_CUTS, visits=off), [c], 1, f"cuts off, row {i}")
        assert 0 < on[0] < off[0], (i, on, off)


def test_cuts_and_windows_prune(emu):
    """R(8) x 16: record cuts visit fewer nodes than the search without them."""
    cases = W.random_cases(8, 16)
    on, off = [], []
    a = solve(emu, cases, tuning=W.TUNE_LEAF(4), visits=on)
    b = solve(emu, cases, tuning=W.TUNE_LEAF(4) | W.TUNE_NO_CUTS, visits=off)
    W.assert_answers(a, cases, 1, "cuts on")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert 0 < on[0] < off[0], (on, off)


def test_workspace_and_tuning_edges(emu):
    """Refusals leave the outputs' 0x55 bytes."""
    cases = W.cycled(W.mixed_wld(deep_row=False), 65)
    n = len(cases)
    assert emu.raz_solve_wld_workspace_bytes(n, W.MAX_EMPTIES + 1) == 0 and emu.raz_solve_wld_workspace_bytes(n, W.MAX_EMPTIES) > 0
    assert emu.raz_solve_wld_workspace_bytes((1 << 31) + 1, 4) == 0
    sizes = [emu.raz_solve_wld_workspace_bytes(n, e) for e in range(0, W.MAX_EMPTIES + 1)]
    assert sizes == sorted(sizes)
    least = sizes[10]   # (the list's deepest searched row has 10 empties)
    for short in (least - 1, sizes[0] - 1):
        assert _untouched(solve(emu, cases, ws_bytes=short, expect=W.RAZ_EINVAL)), "an output byte was written"
    for bad in (1 << 27, 1 << 31, W.TUNE_LEAF(1), W.TUNE_LEAF(W.MAX_EMPTIES + 1), 7 << 20):
        assert _untouched(solve(emu, cases, tuning=bad, expect=W.RAZ_EINVAL))
