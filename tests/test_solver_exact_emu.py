"""CPU: the kernels of raz_solve_exact (csrc/raz_solver_exact.hip) on the wave emulator - tests/native/libraz_emu_solver_exact.so,
the emulator's Makefile with the kernel list given on the command line - against the yardsticks of tests/solver_exact_cases.py at the
emulator's sizes.  The emulator also checks what the hardware does not: that every cross-lane operation of the search kernel is
reached by all lanes of its wave."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import solver_exact_cases as X
from conftest import ROOT, _locked

EMU_DIR = os.path.join(ROOT, "tests", "native", "wave_emu")
EMU_LIB = os.path.join(ROOT, "tests", "native", "libraz_emu_solver_exact.so")
NAMES = ("raz_last_error", "raz_solve_exact", "raz_solve_exact_workspace_bytes", "raz_solve_batch", "raz_solve_batch_workspace_bytes")


def _build(out, extra=""):
    """As tests/test_solver_batch_emu.py builds its library: the Makefile, untouched, in a private copy of its directory."""
    with _locked("emu_solver_exact"), tempfile.TemporaryDirectory(prefix="wave_emu_solver_exact.", dir=os.path.dirname(EMU_DIR)) as work:
        shutil.copytree(EMU_DIR, work, ignore=shutil.ignore_patterns("*.o", "_net", "_full"), dirs_exist_ok=True)
        r = subprocess.run(["make", "-C", work, "OUT=../" + os.path.basename(out), "EXTRA=" + extra,
                            "KERNELS=$(CSRC)/raz_solver_exact.hip $(CSRC)/raz_solver_batch.hip $(CSRC)/raz_capi.hip"],
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


def solve(lib, cases, tuning=0, ws_bytes=None, max_empties=10, expect=X.RAZ_OK, visits=None):
    """(move, score, status) of the cases on the emulated kernels; outputs start as 0x55 so that an untouched byte shows."""
    b, w, p = X.arrays(cases)
    n = len(cases)
    mv, sc, st = np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.int8), np.full(n, 0x55, dtype=np.uint8)
    ws_bytes = lib.raz_solve_exact_workspace_bytes(n, max_empties) if ws_bytes is None else ws_bytes
    keep, ws = _aligned(max(ws_bytes, 1))
    rc = lib.raz_solve_exact(b.ctypes.data, w.ctypes.data, p.ctypes.data, n, mv.ctypes.data, sc.ctypes.data, st.ctypes.data,
                             ws.ctypes.data, ws_bytes, tuning, None)
    assert rc == expect, (rc, (lib.raz_last_error() or b"").decode())
    if visits is not None:
        visits.append(int(ws[:8].view(np.uint64)[0]))
    return mv, sc, st


def test_golden_and_random_positions(emu):
    """G at <= 8 empties plus four of 10, R(1..8) at 16 positions each: one batch per list."""
    for name, cases in X.emu_lists().items():
        X.assert_answers(solve(emu, cases), cases, 1, name)


def test_status_rows(emu):
    """18 empties and the opening are refused, the other rows as raz_solve_batch answers them.  (The 15-empties row that is solved
    now is the GPU's: on the emulator it takes more than two minutes, so no 15-empties row runs here.)"""
    cases = [c for c in X.status_cases() if c[3] != 0]
    assert sorted({c[3] for c in cases}) == [1, 2, 3]
    X.assert_answers(solve(emu, cases), cases, 1, "status rows")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(emu, n):
    cases = X.cycled(X.mixed_exact(deep_row=False), n)
    X.assert_answers(solve(emu, cases), cases, 1, f"n={n}")


def test_n_zero_is_ok_and_launches_nothing(emu):
    assert emu.raz_solve_exact(None, None, None, 0, None, None, None, None, 0, 0, None) == X.RAZ_OK


def test_a_13_empties_position(emu):
    cases = X.deep_cases()[:1]
    assert 64 - bin(cases[0][0] | cases[0][1]).count("1") == 13
    visits = []
    X.assert_answers(solve(emu, cases, max_empties=13, visits=visits), cases, 1, "deep")
    assert 0 < visits[0] < 20_000_000   # (the exhaustive scan visits hundreds of millions of nodes here)


def test_partition_independence(emu):
    """The 257-row mixed list plus one 12-empties row (a parked stack several levels deep) under every tuning, the minimum
    workspace and twice it: byte-identical to tuning = 0, which is right."""
    cases = X.mixed_exact(257, deep_row=False) + X.random_cases(12)[:1]
    least = emu.raz_solve_exact_workspace_bytes(len(cases), 12)
    base = solve(emu, cases, ws_bytes=4 * least)
    X.assert_answers(base, cases, 1, "tuning 0")
    variants = [(t, None, name) for name, t in X.tunings().items()] + [(0, least, "minimum workspace"), (0, 2 * least, "twice the minimum")]
    for tuning, ws_bytes, name in variants:
        got = solve(emu, cases, tuning=tuning, ws_bytes=ws_bytes, max_empties=12)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), (name, hex(tuning), ws_bytes)


def test_a_parked_stack_is_resumed_thousands_of_times(emu):
    """One 12-empties row on ONE lane (no split) at a budget of 3 nodes a launch: every launch parks, the next resumes."""
    cases = X.random_cases(12)[:1]
    visits = []
    X.assert_answers(solve(emu, cases, tuning=X.TUNE_SPLIT(0) | X.TUNE_BUDGET[3], max_empties=12, visits=visits), cases, 1, "parked")
    assert visits[0] > 3000


def test_pruning_happens(emu):
    """R(8) x 16: fewer node visits than the exhaustive scan of raz_solve_batch on the same rows."""
    cases = X.random_cases(8, 16)
    b, w, p = X.arrays(cases)
    n = len(cases)
    mine = []
    got = solve(emu, cases, visits=mine)
    mv, sc, st = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint8)
    nbytes = emu.raz_solve_batch_workspace_bytes(n, 8)
    keep, ws = _aligned(nbytes)
    assert emu.raz_solve_batch(b.ctypes.data, w.ctypes.data, p.ctypes.data, n, 1, mv.ctypes.data, sc.ctypes.data, st.ctypes.data,
                               ws.ctypes.data, nbytes, 0, None) == X.RAZ_OK
    assert (got[0] == mv).all() and (got[1] == sc).all() and (got[2] == st).all()
    assert 0 < mine[0] < int(ws[:8].view(np.uint64)[0])


def test_workspace_and_tuning_edges(emu):
    cases = X.cycled(X.mixed_exact(deep_row=False), 65)
    n = len(cases)
    assert emu.raz_solve_exact_workspace_bytes(n, X.MAX_EMPTIES + 1) == 0 and emu.raz_solve_exact_workspace_bytes(n, X.MAX_EMPTIES) > 0
    assert emu.raz_solve_exact_workspace_bytes((1 << 31) + 1, 4) == 0
    sizes = [emu.raz_solve_exact_workspace_bytes(n, e) for e in range(0, X.MAX_EMPTIES + 1)]
    assert sizes == sorted(sizes)
    least = sizes[10]   # (the list's deepest searched row has 10 empties)
    for short in (least - 1, sizes[0] - 1):
        got = solve(emu, cases, ws_bytes=short, expect=X.RAZ_EINVAL)
        assert all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got), "an output byte was written"
    for bad in (1 << 26, 1 << 31, X.TUNE_LEAF(1), X.TUNE_LEAF(19), 6 << 20):
        got = solve(emu, cases, tuning=bad, expect=X.RAZ_EINVAL)
        assert all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)
