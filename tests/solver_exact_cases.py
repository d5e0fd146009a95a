"""Positions and expected answers for raz_solve_exact (include/raz.h), shared by tests/test_solver_exact_gpu.py (the kernels on an
MI355X), tests/test_solver_exact_emu.py (the same kernels on the wave emulator) and tests/test_solver_exact_host.py.

The lists of tests/solver_batch_cases.py are taken as they are - a case is (black, white, player byte, status, {0: .., 1: (move,
score)}) and raz_solve_exact answers the full scan, entry 1.  Added here:
  ab_check     tests/native/ab_check.c, a plain host negamax with bounds on loops of its own, compiled by the test: the yardstick
               beyond 14 empties, where the oracle's exhaustive scan takes hours.  It searches every root child under the full window,
               so it knows every root child's exact value;
  deep2        tests/golden/solver_exact_deep.json - R(15) x 8, R(16) x 4, R(17) x 2 (seed 7100 + e) with ab_check's
               answers and root values recorded (make_golden_solver_exact_deep.py);
  status rows  of raz_solve_exact: the 15-empties row is searched now, an 18-empties row and the opening are refused.
Every comparison made with these is exact equality of move, score and status."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import solver_batch_cases as C
from solver_batch_cases import (GOLDEN, NO_MOVE, RAZ_OK, RAZ_EINVAL, RAZ_EDEVICE, arrays, assert_answers, cycled, deep_cases,  # noqa: F401
                                emu_lists, expected, gpu_lists, mixed_list, moves_of, play, random_cases, random_positions, squares)

MAX_EMPTIES = 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tuning word of raz_solve_exact (include/raz.h)
TUNE_LEAF = lambda n: n                        # noqa: E731
TUNE_SPLIT = lambda plies: (plies + 1) << 5    # noqa: E731
TUNE_CHUNK = lambda n: n << 8                  # noqa: E731
TUNE_BUDGET = {3: 1 << 20, 16: 2 << 20, 128: 3 << 20, 1024: 4 << 20, 8192: 5 << 20}
TUNE_NO_ORDER = 1 << 24
TUNE_NO_SIBLINGS = 1 << 25


def tunings():
    """name -> tuning word: every knob on its own and the hardest combinations."""
    t = {"budget 3": TUNE_BUDGET[3], "budget 16": TUNE_BUDGET[16], "budget 128": TUNE_BUDGET[128],
         "no order": TUNE_NO_ORDER, "no siblings": TUNE_NO_SIBLINGS, "chunk of one row": TUNE_CHUNK(1)}
    for plies in range(0, 7):
        t[f"split {plies} plies to leaf 4"] = TUNE_SPLIT(plies) | TUNE_LEAF(4)
    t["leaf 2, budget 3"] = TUNE_LEAF(2) | TUNE_BUDGET[3]
    t["leaf 7, budget 16, no order"] = TUNE_LEAF(7) | TUNE_BUDGET[16] | TUNE_NO_ORDER
    t["leaf 6, budget 128, no siblings, chunk 3"] = TUNE_LEAF(6) | TUNE_BUDGET[128] | TUNE_NO_SIBLINGS | TUNE_CHUNK(3)
    return t


# ---- ab_check ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ab():
    d = tempfile.mkdtemp(prefix="ab_check.")
    so = os.path.join(d, "ab_check.so")
    r = subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "native", "ab_check.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.ab_root.restype = ctypes.c_int
    lib.ab_root.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def ab_answer(black, white, player):
    """((move, score), {square: exact value of that root move}, node visits) of the side to move, by ab_check."""
    own, enemy = (black, white) if player == 1 else (white, black)
    values = np.zeros(64, dtype=np.int8)
    mv, sc, nodes = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
    n = _ab().ab_root(own, enemy, values.ctypes.data, ctypes.addressof(mv), ctypes.addressof(sc), ctypes.addressof(nodes))
    if n == 0:
        return NO_MOVE, {}, 0
    return (mv.value, sc.value), {s: int(values[s]) for s in range(64) if values[s] != -100}, nodes.value


# ---- the fixture beyond 14 empties --------------------------------------------------------------------------------------------
DEEP2_COUNTS = {15: 8, 16: 4, 17: 2}


def deep2_positions():
    return [(e, pos) for e, count in DEEP2_COUNTS.items() for pos in random_positions(e, count, 7100 + e)]


@functools.lru_cache(maxsize=None)
def deep2_cases():
    with open(os.path.join(GOLDEN, "solver_exact_deep.json")) as f:
        doc = json.load(f)
    got = [(p["empties"], (int(p["black"], 16), int(p["white"], 16), p["next_player"])) for p in doc["positions"]]
    assert got == deep2_positions(), "the fixture is not the generator's"
    out = []
    for p in doc["positions"]:
        values = {int(s): v for s, v in p["root_values"].items()}
        best = max(values.values())
        assert tuple(p["exact"]) == (min(s for s, v in values.items() if v == best), best), "the fixture's answer is not its values' first maximum"
        out.append((int(p["black"], 16), int(p["white"], 16), p["next_player"], 0, {1: tuple(p["exact"])}))
    return tuple(out)


# ---- status rows ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def status_cases():
    """solver_batch_cases' rows with the limit moved: its 15-empties row is SOLVED here (ab_check's answer), a playout
    position of one empty square more than the limit and the opening are refused."""
    rows = []
    for b, w, p, st, ans in C.status_cases():
        e = 64 - bin(b | w).count("1")
        if st == 2 and e == 15:
            rows.append((b, w, p, 0, {1: ab_answer(b, w, p)[0]}))
        else:
            rows.append((b, w, p, st, ans))
    bx, wx, px = random_positions(MAX_EMPTIES + 1, 1, 9000 + MAX_EMPTIES + 1)[0]
    rows.append((bx, wx, px, 2, {1: NO_MOVE}))
    assert sorted({r[3] for r in rows}) == [0, 1, 2, 3] and sum(r[3] == 2 for r in rows) == 2
    return tuple(rows)


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def tied_maximum(case):
    """Two or more root moves attain the maximum (by ab_check's root values)."""
    b, w, p, st, ans = case
    if st != 0:
        return False
    _, values, _ = ab_answer(b, w, p)
    return sum(v == ans[1][1] for v in values.values()) >= 2


@functools.lru_cache(maxsize=None)
def assert_exact_coverage():
    """Over everything the GPU lists hold: >= 10 rows with a tied maximum, with a pass / an end of the game within three plies, with
    one legal root move.  (ab_check is only asked about rows of at most 10 empties here: they are enough.)"""
    cases = [c for cs in gpu_lists().values() for c in cs]
    c = C.coverage(cases)
    tied = sum(tied_maximum(x) for x in cases if 64 - bin(x[0] | x[1]).count("1") <= 10)
    got = {"tied maximum": tied, **{k: c[k] for k in ("pass in three plies", "game ends in three plies", "one legal root move")}}
    assert all(v >= 10 for v in got.values()), got
    return got


@functools.lru_cache(maxsize=None)
def mixed_exact(rows=257, deep_row=True):
    """The mixed list with raz_solve_exact's status rows in the places of raz_solve_batch's.  deep_row=False (the emulator, where
    a 15-empties search takes most of a minute): the refused row just above the limit stands where the 15-empties row would."""
    old, new = C.status_cases(), status_cases()
    swap = {o[:3]: nw for o, nw in zip(old, new)}
    if not deep_row:
        swap = {k: (new[-1] if v[3] == 0 else v) for k, v in swap.items()}
    return tuple(swap.get(c[:3], c) if c[3] != 0 else c for c in mixed_list(rows))
