"""Positions and expected answers for raz_solve_wld (include/raz.h), shared by tests/test_solver_wld_gpu.py (the kernels on an
MI355X), tests/test_solver_wld_emu.py (the same kernels on the wave emulator) and tests/test_solver_wld_host.py.

raz_solve_wld answers (move, outcome): outcome = the sign of the game-theoretic disc difference from the side to move's view,
move = the lowest-numbered legal move whose own outcome is that outcome.  The lists of tests/solver_batch_cases.py and
tests/solver_exact_cases.py are taken as they are and their expectations are computed from the EXACT root values - ab_check's
(tests/native/ab_check.c) or the ones recorded in tests/golden/solver_exact_deep.json - as
    (min(s : sign(v[s]) == sign(max v)), sign(max v)).
A converted case is (black, white, player byte, status, {1: (move, outcome)}), so solver_batch_cases.assert_answers(got, cases, 1)
compares it.  Added here:
  wld_check    tests/native/wld_check.c, a plain host negamax over the three outcomes with the (-1, +1) window under every root move,
               compiled by the test: the yardstick beyond 17 empties;
  deep3        tests/golden/solver_wld_deep.json - R(18), R(19), R(20) x 4 and R(21) x 2 (seed 7200 + e) with wld_check's per-move
               outcomes, answer, nodes and seconds recorded (make_golden_solver_wld_deep.py);
  status rows  of raz_solve_wld: a row of one empty square more than the limit and the opening are refused.
Every comparison made with these is exact equality of move, outcome and status."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import solver_batch_cases as C
import solver_exact_cases as X
from solver_batch_cases import (GOLDEN, NO_MOVE, RAZ_OK, RAZ_EINVAL, RAZ_EDEVICE, arrays, assert_answers, cycled, moves_of, play,  # noqa: F401
                                random_positions, squares)

MAX_EMPTIES = 21   # RAZ_SOLVE_WLD_MAX_EMPTIES: measured (the win/draw/loss solver)
ROOT = X.ROOT

# tuning word of raz_solve_wld (include/raz.h): raz_solve_exact's fields, and bit 26
TUNE_LEAF, TUNE_SPLIT, TUNE_CHUNK, TUNE_BUDGET, TUNE_NO_ORDER = X.TUNE_LEAF, X.TUNE_SPLIT, X.TUNE_CHUNK, X.TUNE_BUDGET, X.TUNE_NO_ORDER
TUNE_NO_CUTS = 1 << 26


def tunings():
    """name -> tuning word: every knob on its own and the hardest combinations."""
    t = {"budget 3": TUNE_BUDGET[3], "budget 16": TUNE_BUDGET[16], "budget 128": TUNE_BUDGET[128],
         "no order": TUNE_NO_ORDER, "no cuts": TUNE_NO_CUTS, "chunk of one row": TUNE_CHUNK(1)}
    for plies in range(0, 7):
        t[f"split {plies} plies to leaf 4"] = TUNE_SPLIT(plies) | TUNE_LEAF(4)
    t["leaf 2, budget 3"] = TUNE_LEAF(2) | TUNE_BUDGET[3]
    t["leaf 2, budget 3, no cuts"] = TUNE_LEAF(2) | TUNE_BUDGET[3] | TUNE_NO_CUTS
    t["leaf 7, budget 16, no order"] = TUNE_LEAF(7) | TUNE_BUDGET[16] | TUNE_NO_ORDER
    t["leaf 6, budget 128, no cuts, chunk 3"] = TUNE_LEAF(6) | TUNE_BUDGET[128] | TUNE_NO_CUTS | TUNE_CHUNK(3)
    return t


def sign(v):
    return (v > 0) - (v < 0)


def from_values(values):
    """The WLD answer that follows from a root's exact (or three-valued) move values {square: value}."""
    o = sign(max(values.values()))
    return min(s for s, v in values.items() if sign(v) == o), o


# ---- wld_check ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wld():
    d = tempfile.mkdtemp(prefix="wld_check.")
    so = os.path.join(d, "wld_check.so")
    r = subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "native", "wld_check.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.wld_root.restype = ctypes.c_int
    lib.wld_root.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def wld_answer(black, white, player):
    """((move, outcome), {square: outcome of that root move}, node visits) of the side to move, by wld_check."""
    own, enemy = (black, white) if player == 1 else (white, black)
    values = np.zeros(64, dtype=np.int8)
    mv, sc, nodes = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
    n = _wld().wld_root(own, enemy, values.ctypes.data, ctypes.addressof(mv), ctypes.addressof(sc), ctypes.addressof(nodes))
    if n == 0:
        return NO_MOVE, {}, 0
    return (mv.value, sc.value), {s: int(values[s]) for s in range(64) if values[s] != -100}, nodes.value


# ---- the existing lists, converted --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _converted(b, w, p, st):
    if st != 0:
        return (b, w, p, st, {1: NO_MOVE})
    _, values, _ = X.ab_answer(b, w, p)
    return (b, w, p, 0, {1: from_values(values)})


def convert(case):
    """A case of solver_batch_cases / solver_exact_cases with raz_solve_wld's answer in entry 1 (from ab_check's root values)."""
    return _converted(*case[:4])


def _convert_all(cases):
    return tuple(convert(c) for c in cases)


@functools.lru_cache(maxsize=None)
def gpu_lists():
    return {name: _convert_all(cases) for name, cases in C.gpu_lists().items()}


@functools.lru_cache(maxsize=None)
def emu_lists():
    return {name: _convert_all(cases) for name, cases in C.emu_lists().items()}


@functools.lru_cache(maxsize=None)
def random_cases(empties, count=None):
    return _convert_all(C.random_cases(empties, count))


@functools.lru_cache(maxsize=None)
def deep_cases():
    """The 13 / 14 empties fixture rows of raz_solve_batch."""
    return _convert_all(C.deep_cases())


@functools.lru_cache(maxsize=None)
def deep2_cases():
    """The 15..17 empties rows of solver_exact_deep.json, from their RECORDED root values."""
    with open(os.path.join(GOLDEN, "solver_exact_deep.json")) as f:
        doc = json.load(f)
    assert len(doc["positions"]) == len(X.deep2_cases())
    return tuple((int(p["black"], 16), int(p["white"], 16), p["next_player"], 0,
                  {1: from_values({int(s): v for s, v in p["root_values"].items()})}) for p in doc["positions"])


# ---- the fixture beyond 17 empties --------------------------------------------------------------------------------------------
DEEP3_COUNTS = {18: 4, 19: 4, 20: 4, 21: 2}


def deep3_positions():
    return [(e, pos) for e, count in DEEP3_COUNTS.items() for pos in random_positions(e, count, 7200 + e)]


@functools.lru_cache(maxsize=None)
def deep3_doc():
    with open(os.path.join(GOLDEN, "solver_wld_deep.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def deep3_cases():
    doc = deep3_doc()
    got = [(p["empties"], (int(p["black"], 16), int(p["white"], 16), p["next_player"])) for p in doc["positions"]]
    assert got == deep3_positions(), "the fixture is not the generator's"
    out = []
    for p in doc["positions"]:
        outcomes = {int(s): v for s, v in p["root_outcomes"].items()}
        assert tuple(p["wld"]) == from_values(outcomes), "the fixture's answer is not its outcomes' lowest-numbered best"
        out.append((int(p["black"], 16), int(p["white"], 16), p["next_player"], 0, {1: tuple(p["wld"])}))
    return tuple(out)


def empties_of(case):
    return 64 - bin(case[0] | case[1]).count("1")


# ---- status rows ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def status_cases(deep_row=True):
    """solver_batch_cases' rows with the limit moved: its 15-empties row is SOLVED here, a playout position of one empty square more
    than the limit and the opening are refused.  deep_row=False (the emulator): without the 15-empties row."""
    rows = []
    for c in C.status_cases():
        if c[3] == 2 and empties_of(c) == 15:
            if deep_row:
                rows.append(convert((c[0], c[1], c[2], 0, None)))
        else:
            rows.append((c[0], c[1], c[2], c[3], {1: NO_MOVE}))
    bx, wx, px = random_positions(MAX_EMPTIES + 1, 1, 9000 + MAX_EMPTIES + 1)[0]
    rows.append((bx, wx, px, 2, {1: NO_MOVE}))
    assert {1, 2, 3} <= {r[3] for r in rows} and sum(r[3] == 2 for r in rows) == 2
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def mixed_wld(rows=257, deep_row=True):
    """solver_batch_cases.mixed_list with raz_solve_wld's status rows in the places of raz_solve_batch's (deep_row=False: the
    refused row just above the limit stands where the 15-empties row would)."""
    old, new = C.status_cases(), status_cases()
    by_pos = {r[:3]: r for r in new}
    swap = {}
    for o in old:
        swap[o[:3]] = by_pos[o[:3]] if (deep_row or by_pos[o[:3]][3] != 0) else new[-1]
    return tuple(swap[c[:3]] if c[3] != 0 else convert(c) for c in C.mixed_list(rows))


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def coverage(lists):
    """Rows of at most 10 empties: the WLD move differs from the exact move / outcome 0 / outcome +1 whose lowest-numbered legal
    move does not win / outcome 0 whose lowest-numbered legal move loses."""
    got = {"differs from the exact move": 0, "draw": 0, "win, first move does not win": 0, "draw, first move loses": 0}
    for cases in lists.values():
        for b, w, p, st, ans in cases:
            if st != 0 or empties_of((b, w)) > 10:
                continue
            (xm, _), values, _ = X.ab_answer(b, w, p)
            mv, o = ans[1]
            first = sign(values[min(values)])
            got["differs from the exact move"] += mv != xm
            got["draw"] += o == 0
            got["win, first move does not win"] += o == 1 and first != 1
            got["draw, first move loses"] += o == 0 and first == -1
    return got


@functools.lru_cache(maxsize=None)
def assert_wld_coverage(emu=False):
    got = coverage(emu_lists() if emu else gpu_lists())
    least = (10, 3, 10, 0) if emu else (10, 10, 10, 10)
    assert all(v >= m for v, m in zip(got.values(), least)), got
    return got
