"""Positions and expected answers for raz_solve_batch (include/raz.h), shared by tests/test_solver_batch_gpu.py (the kernels on an
MI355X) and tests/test_solver_batch_emu.py (the same kernels on the wave emulator), as spec_cases.py / slot_cases.py are.

A case is (black, white, player byte, status, {0: (move, score), 1: (move, score)}): the answers of win/loss mode (exactly = 0)
and of the full scan (exactly = 1); rows with status != 0 answer (-1, -100) in both modes.  Yardsticks:
  G      tests/golden/solver_kat.json - the reference's compiled Cython solver on its 3 known answers and 120 positions;
  R(e)   seeded random playouts with e empties and the side to move able to move, answered by the oracle (oracle/orc_solver.c, pinned
         to that solver by tests/test_oracle_solver.py);
  deep   tests/golden/solver_batch_deep.json - R(13) x 4 and R(14) x 2 with the oracle's answers recorded (an exact solve there takes
         the oracle 11 s and 78 s: make_golden_solver_batch_deep.py);
  status rows the call answers without a search.
Every comparison made with these is exact equality of move, score and status."""
import ctypes
import functools
import json
import os
import random

import numpy as np

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INIT_BLACK, INIT_WHITE = 0x0000000810000000, 0x0000001008000000
M64 = (1 << 64) - 1
NO_MOVE = (-1, -100)
RAZ_OK, RAZ_EINVAL, RAZ_EDEVICE = 0, -1, -2

# tuning word of raz_solve_batch (include/raz.h): bits 0-3 leaf size, 4-7 split plies + 1, 8-23 rows per chunk
TUNE_LEAF = lambda n: n                 # noqa: E731
TUNE_SPLIT = lambda plies: (plies + 1) << 4   # noqa: E731
TUNE_CHUNK = lambda n: n << 8           # noqa: E731


def _orc():
    return O.load_ext()


def moves_of(own, enemy):
    return _orc().orc_find_correct_moves(own, enemy)


def play(a, own, enemy):
    """(own, enemy) after `own` played square a, still from the mover's view."""
    f = _orc().orc_calc_flip(a, own, enemy)
    return (own ^ f) | (1 << a), enemy ^ f


def squares(mask):
    return [i for i in range(64) if mask >> i & 1]


def random_positions(empties, count, seed):
    """`count` positions with `empties` empty squares in which the side to move can move: random.Random(seed) playouts from the
    opening position (a side without a move passes; a playout that ends or gets stuck before the count is reached is dropped)."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        own, enemy, player = INIT_BLACK, INIT_WHITE, 1
        ok = True
        while bin(own | enemy).count("1") < 64 - empties:
            legal = moves_of(own, enemy)
            if not legal:
                own, enemy, player = enemy, own, 3 - player
                legal = moves_of(own, enemy)
                if not legal:
                    ok = False
                    break
            own, enemy = play(rng.choice(squares(legal)), own, enemy)
            own, enemy, player = enemy, own, 3 - player
        if not ok:
            continue
        if not moves_of(own, enemy):
            if not moves_of(enemy, own):
                continue
            own, enemy, player = enemy, own, 3 - player
        out.append((own, enemy, 1) if player == 1 else (enemy, own, 2))
    return out


def oracle_answer(black, white, player, exactly):
    lib = _orc()
    s = lib.orc_solver_new()
    mv, sc = ctypes.c_int(-1), ctypes.c_int(0)
    ok = lib.orc_solver_solve(s, black, white, player, int(exactly), ctypes.byref(mv), ctypes.byref(sc))
    lib.orc_solver_free(s)
    return (mv.value, sc.value) if ok else NO_MOVE


def _case(b, w, p, ans0, ans1):
    return (b, w, p, 0, {0: tuple(ans0), 1: tuple(ans1)})


@functools.lru_cache(maxsize=None)
def golden_cases(max_empties=14, extra_at_10=None):
    """G.  max_empties / extra_at_10: the emulator's subset (positions of <= max_empties empties plus the first extra_at_10 of 10)."""
    with open(os.path.join(GOLDEN, "solver_kat.json")) as f:
        kat = json.load(f)
    rows = []
    for k in kat["kat"]:
        ans = {int(k["exactly"]): k["answer"], int(not k["exactly"]): k["answer_other_mode"]}
        rows.append((int(k["black"], 16), int(k["white"], 16), k["next_player"], ans[0], ans[1]))
    for p in kat["positions"]:
        rows.append((int(p["black"], 16), int(p["white"], 16), p["next_player"], p["non_exact"], p["exact"]))
    out, at10 = [], 0
    for b, w, p, a0, a1 in rows:
        e = 64 - bin(b | w).count("1")
        if e > max_empties:
            if not (extra_at_10 and e == 10 and at10 < extra_at_10):
                continue
            at10 += 1
        out.append(_case(b, w, p, a0, a1))
    return tuple(out)


R_COUNTS = {**{e: 64 for e in range(1, 11)}, 11: 8, 12: 3}


@functools.lru_cache(maxsize=None)
def random_cases(empties, count=None):
    """R(empties): the first `count` (default: R_COUNTS) positions of the seeded generator, answered by the oracle in both modes."""
    count = R_COUNTS[empties] if count is None else count
    return tuple(_case(b, w, p, oracle_answer(b, w, p, 0), oracle_answer(b, w, p, 1))
                 for b, w, p in random_positions(empties, count, 7000 + empties))


DEEP_COUNTS = {13: 4, 14: 2}


@functools.lru_cache(maxsize=None)
def deep_cases():
    with open(os.path.join(GOLDEN, "solver_batch_deep.json")) as f:
        doc = json.load(f)
    out = []
    for e, count in DEEP_COUNTS.items():
        want = random_positions(e, count, 7000 + e)
        got = [p for p in doc["positions"] if p["empties"] == e]
        assert [(int(p["black"], 16), int(p["white"], 16), p["next_player"]) for p in got] == want, "the fixture is not the generator's"
        out += [_case(int(p["black"], 16), int(p["white"], 16), p["next_player"], p["non_exact"], p["exact"]) for p in got]
    return tuple(out)


def _bits(sq):
    m = 0
    for s in sq:
        m |= 1 << s
    return m


@functools.lru_cache(maxsize=None)
def status_cases():
    """Rows answered without a search.  Checked here against the host's move generator, so that each row is what its name says."""
    full = M64
    rows = []
    # 1. the side to move must pass while the opponent can move: one ply below a playout position, a child in which the opponent
    # is stuck and the mover is not - that child with the OPPONENT to move
    pass_row = None
    for bb, ww, pl in random_positions(5, 400, 9100):
        own, enemy = (bb, ww) if pl == 1 else (ww, bb)
        for a in squares(moves_of(own, enemy)):
            no, ne = play(a, own, enemy)
            if not moves_of(ne, no) and moves_of(no, ne):
                pass_row = (no, ne, 2) if pl == 1 else (ne, no, 1)
                break
        if pass_row:
            break
    assert pass_row is not None
    pb, pw, pp = pass_row
    own, enemy = (pb, pw) if pp == 1 else (pw, pb)
    assert not moves_of(own, enemy) and moves_of(enemy, own) and 0 < 64 - bin(pb | pw).count("1") <= 14
    rows.append(("root must pass", pb, pw, pp, 1))
    # 2. a finished game with empties left: nobody can move
    fb, fw = _bits(range(0, 60)), 0   # (a wipe-out)
    assert not moves_of(fb, fw) and not moves_of(fw, fb) and 64 - bin(fb | fw).count("1") == 4
    rows.append(("finished game", fb, fw, 1, 1))
    # 3. a full board
    rows.append(("full board", _bits(range(0, 30)), full ^ _bits(range(0, 30)), 2, 1))
    # 4. 15 empties (a playout position whose mover can move) and the opening position: refused
    b15, w15, p15 = random_positions(15, 1, 9015)[0]
    rows.append(("15 empties", b15, w15, p15, 2))
    rows.append(("opening", INIT_BLACK, INIT_WHITE, 1, 2))
    # 5. not a position: a square of both colours (on an otherwise searchable board), player bytes 0 and 3
    gb, gw, gp = random_positions(6, 1, 9006)[0]
    rows.append(("both colours", gb | (gw & -gw), gw, gp, 3))
    rows.append(("player 0", gb, gw, 0, 3))
    rows.append(("player 3", gb, gw, 3, 3))
    return tuple((b, w, p, st, {0: NO_MOVE, 1: NO_MOVE}) for _, b, w, p, st in rows)


# ---- coverage conditions: a host-side walk over the first three plies -------------------------------------------------------
def _walk(own, enemy, plies, seen):
    """seen['pass'] / seen['end']: some line passes / ends the game within the next `plies` moves."""
    if plies == 0:
        return
    for a in squares(moves_of(own, enemy)):
        no, ne = play(a, own, enemy)
        if moves_of(ne, no):
            _walk(ne, no, plies - 1, seen)
        elif moves_of(no, ne):
            seen["pass"] = True
            _walk(no, ne, plies - 1, seen)
        else:
            seen["end"] = True


def coverage(cases):
    c = {"pass in three plies": 0, "game ends in three plies": 0, "one legal root move": 0, "first root move wins": 0, "no move wins": 0}
    for b, w, p, st, ans in cases:
        if st != 0:
            continue
        own, enemy = (b, w) if p == 1 else (w, b)
        legal = moves_of(own, enemy)
        seen = {"pass": False, "end": False}
        _walk(own, enemy, 3, seen)
        c["pass in three plies"] += seen["pass"]
        c["game ends in three plies"] += seen["end"]
        c["one legal root move"] += bin(legal).count("1") == 1
        c["first root move wins"] += ans[0][1] > 0 and ans[0][0] == squares(legal)[0]
        c["no move wins"] += ans[0][1] <= 0
    return c


def assert_coverage(cases, least=10):
    c = coverage(cases)
    assert all(v >= least for v in c.values()), c
    return c


@functools.lru_cache(maxsize=None)
def gpu_lists():
    """name -> cases, each solved as one batch per mode on the GPU.  The coverage conditions hold over all of them."""
    lists = {"G": golden_cases()}
    for e in range(1, 13):
        lists[f"R{e}"] = random_cases(e)
    assert_coverage([c for cs in lists.values() for c in cs])
    return lists


@functools.lru_cache(maxsize=None)
def emu_lists():
    lists = {"G": golden_cases(8, 4)}
    for e in range(1, 9):
        lists[f"R{e}"] = random_cases(e, 16)
    assert_coverage([c for cs in lists.values() for c in cs])
    return lists


@functools.lru_cache(maxsize=None)
def mixed_list(rows=257, deepest=10):
    """Empties 1..deepest interleaved, so that neighbouring lanes differ in depth, with a status row after every seventh position."""
    per = {e: random_cases(e, 16) for e in range(1, deepest + 1)}
    st = status_cases()
    out, i = [], 0
    while len(out) < rows:
        out.append(per[1 + i % deepest][(i // deepest) % 16])
        if i % 7 == 6:
            out.append(st[(i // 7) % len(st)])
        i += 1
    return tuple(out[:rows])


def cycled(cases, n):
    return tuple(cases[i % len(cases)] for i in range(n))


def arrays(cases):
    b = np.array([c[0] for c in cases], dtype=np.uint64)
    w = np.array([c[1] for c in cases], dtype=np.uint64)
    p = np.array([c[2] for c in cases], dtype=np.uint8)
    return b, w, p


def expected(cases, exactly):
    mv = np.array([c[4][int(exactly)][0] for c in cases], dtype=np.int8)
    sc = np.array([c[4][int(exactly)][1] for c in cases], dtype=np.int8)
    st = np.array([c[3] for c in cases], dtype=np.uint8)
    return mv, sc, st


def assert_answers(got, cases, exactly, what=""):
    """got = (move, score, status) arrays: exact equality with the cases' answers, reporting the first rows that differ."""
    want = expected(cases, exactly)
    for name, g, w in zip(("status", "move", "score"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
        g = np.asarray(g)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, f"exactly={int(exactly)}", name, [(int(i), int(g[i]), int(w[i]), hex(cases[i][0]), hex(cases[i][1]), cases[i][2]) for i in bad[:5]])
