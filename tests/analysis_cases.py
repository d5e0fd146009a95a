"""Shared cases of the retrograde analysis on the device (include/raz.h raz_analysis_*, csrc/raz_analysis.h), run by
tests/test_analysis_emu.py on the wave emulator and by tests/test_analysis_gpu.py on the device.

Both drive the product's engine.DeviceAnalysis.  A BACKEND (tests/match_cases.py's Adapter) gives the cases
    backend.engine(cfg, blob, n_slots, seed, sims, first_game_id=0, **kw)   a started engine (record_root_w) with every slot idle
    backend.raw(engine)        record 0 of every slot: dict of action, flags, q, n [slots] and root_n, root_w [slots, 64]
    backend.controls(engine)   the slots' control blocks, uint8 [slots, 256] (raz_engine_debug_read, which = 3)
    backend.analysis(engine, n_games, max_moves, first_slot=0, guard=4096)
                               an AnalysisHarness: start(moves int8 [n, max_moves], positions or None, sims), collect(), stats() -> dict,
                               read() -> (ANALYSIS_GAME [n], ANALYSIS_POS [n, P], ANALYSIS_EVAL [n, P]), workspace(), check_guard()

The EXPECTATION of the replay is py_walk: a pure-Python restatement of ReversiEnv.step (rays walked square by square on integers; none
of the product's bitboard primitives), checked once against the package's ReversiEnv facade on the same lists.  The expectation of
the evals is a second engine of the same seed whose SEARCH slots are armed one by one with raz_engine_set_position, reduced by numpy.
All comparisons are exact."""
from random import Random

import numpy as np

import match_cases as M

PA, END = -1, -2
INIT = (0x0000000810000000, 0x0000001008000000, 1)
NONE, SEARCH, PASS_ENTRY, OVER = 0, 1, 2, 3
END_LIST, END_RULES, END_ILLEGAL = 0, 1, 2
BAD_CODE = 0x400


class AnalysisHarness(M.Guarded):
    """engine.DeviceAnalysis behind the interface of the cases, in a guarded workspace."""

    def __init__(self, backend, engine, n_games, max_moves, first_slot=0, guard=M.GUARD):
        from reversi_alpha_zero_amd.engine import DeviceAnalysis
        super().__init__(backend, engine.lib.raz_analysis_workspace_bytes(n_games, max_moves), guard)
        self.w, self.n, self.mm = DeviceAnalysis(engine, first_slot=first_slot, workspace=self.given), n_games, max_moves

    def start(self, moves, positions, sims):
        assert moves.shape == (self.n, self.mm)
        self.w.start(self.backend.tensor(moves), None if positions is None else tuple(self.backend.tensor(a) for a in positions), sims)

    def collect(self):
        self.w.collect()

    def read(self):
        return self.w.results()


# ---- the independent walk -----------------------------------------------------------------------------------------------------
def py_flips(own, enemy, a):
    """The discs a move on square a turns over: along each of the 8 rays a run of enemy discs closed by an own disc."""
    y, x = divmod(a, 8)
    out = 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            run, yy, xx = 0, y + dy, x + dx
            while 0 <= yy < 8 and 0 <= xx < 8 and (enemy >> (yy * 8 + xx)) & 1:
                run |= 1 << (yy * 8 + xx)
                yy, xx = yy + dy, xx + dx
            if run and 0 <= yy < 8 and 0 <= xx < 8 and (own >> (yy * 8 + xx)) & 1:
                out |= run
    return out


def py_legal(own, enemy):
    return [a for a in range(64) if not ((own | enemy) >> a) & 1 and py_flips(own, enemy, a)]


def py_step(black, white, player, action):
    """ReversiEnv.step: (black, white, player, winner or 0, illegal)."""
    own, enemy = (black, white) if player == 1 else (white, black)
    f = py_flips(own, enemy, action)
    if not f:
        return black, white, player, 3 - player, True
    own, enemy = (own ^ f) | (1 << action), enemy ^ f
    black, white = (own, enemy) if player == 1 else (enemy, own)
    if py_legal(enemy, own):
        return black, white, 3 - player, 0, False
    if py_legal(own, enemy):
        return black, white, player, 0, False
    nb, nw = bin(black).count("1"), bin(white).count("1")
    return black, white, player, (1 if nb > nw else 2 if nb < nw else 3), False


def py_walk(start, entries, max_moves):
    """The positions (black, white, player, state, moves_made, played) of one list and the game's summary dict."""
    black, white, player = start or INIT
    pos, over, summary = [], False, dict(ended=END_LIST, winner=0, errors=0, searched=0)
    entries = list(entries)[:max_moves]
    for j in range(max_moves + 1):
        code = entries[j] if j < len(entries) else END
        if not over and not (END <= code <= 63):
            summary["errors"] |= BAD_CODE
            code = END
        if over:
            pos.append((black, white, player, OVER, j, END))
            break
        if code == END:
            pos.append((black, white, player, SEARCH, j, END))
            summary["searched"] += 1
            break
        if code == PA:
            pos.append((black, white, player, PASS_ENTRY, j, PA))
            continue
        pos.append((black, white, player, SEARCH, j, code))
        summary["searched"] += 1
        black, white, player, winner, illegal = py_step(black, white, player, code)
        if winner:
            over = True
            summary.update(winner=winner, ended=END_ILLEGAL if illegal else END_RULES)
    summary.update(positions=len(pos), blacks=bin(black).count("1"), whites=bin(white).count("1"))
    return pos, summary


def facade_walk(start, entries, max_moves):
    """The same through the package's ReversiEnv, as NBoardEngine.set_game drives it; entries after the end are not played."""
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
    b, w, p = start or INIT
    env = ReversiEnv().reset().update(b, w, Player(p))
    seen = []
    for j, code in enumerate(list(entries)[:max_moves] + [END]):
        seen.append((env.board.black, env.board.white, env.next_player.value, env.done))
        if env.done or not (PA <= code <= 63):
            break
        if code != PA:
            env.step(code)
    return seen, (env.winner.value if env.done else 0)


def check_walk_against_facade(games, max_moves):
    for start, entries in games:
        pos, summary = py_walk(start, entries, max_moves)
        seen, winner = facade_walk(start, entries, max_moves)
        assert [(p[0], p[1], p[2], p[3] == OVER) for p in pos] == seen, (start, entries)
        assert summary["winner"] == winner


# ---- lists ----------------------------------------------------------------------------------------------------------------------
def playout(rnd, start=None, stop_discs=65):
    """A random legal playout: (entries, positions before each entry and the last, passes: indices of entries after which the
    opponent had no move, winner or 0)."""
    b, w, p = start or INIT
    entries, seen, passes, winner = [], [(b, w, p)], [], 0
    while not winner and bin(b | w).count("1") < stop_discs:
        own, enemy = (b, w) if p == 1 else (w, b)
        a = rnd.choice(py_legal(own, enemy))
        nb, nw, np_, winner, _ = py_step(b, w, p, a)
        if not winner and np_ == p:
            passes.append(len(entries))
        entries.append(a)
        b, w, p = nb, nw, np_
        seen.append((b, w, p))
    return entries, seen, passes, winner


def no_flip_square(pos):
    b, w, p = pos
    own, enemy = (b, w) if p == 1 else (w, b)
    return next(a for a in range(64) if not ((b | w) >> a) & 1 and not py_flips(own, enemy, a))


def special_games(max_moves=64, seed=3):
    """The named lists of case 1, each (start or None, entries), found by seeded random playouts."""
    rnd, found = Random(seed), {}
    want = {"full60", "auto_pass", "pass_entry", "white_start", "early_end", "illegal_middle", "after_end", "empty", "no_terminator", "bad_code"}
    found["empty"] = (None, [])
    while set(found) != want:
        entries, seen, passes, winner = playout(rnd)
        discs = bin(seen[-1][0] | seen[-1][1]).count("1")
        if winner and discs == 64 and len(entries) == 60 and not passes:
            found.setdefault("full60", (None, entries))
            found.setdefault("after_end", (None, entries + [0, PA, 63]))
        if winner and discs < 64:
            found.setdefault("early_end", (None, entries))
        if passes and passes[0] < len(entries) - 1:
            found.setdefault("auto_pass", (None, entries))
            k = passes[0] + 1
            found.setdefault("pass_entry", (None, entries[:k] + [PA] + entries[k:]))
        if len(entries) >= 58 and "no_terminator" not in found:
            cut = entries[:58]
            for k in (3, 10, 11, 30, 50, 63):   # pass entries wherever: 64 entries, a game still running, no room for a terminator
                cut.insert(k, PA)
            if not py_walk(None, cut, max_moves)[1]["winner"]:
                found["no_terminator"] = (None, cut)
        whites = [j for j, s in enumerate(seen[:20]) if s[2] == 2 and j >= 5]
        if whites:
            j = whites[0]
            found.setdefault("white_start", (seen[j], entries[j:]))
        found.setdefault("illegal_middle", (None, entries[:12] + [no_flip_square(seen[12])] + entries[12:20]))
        found.setdefault("bad_code", (None, entries[:7] + [64] + entries[7:9]))
    return found


def assert_special_set(sp, max_moves=64):
    """Case 1's fixture: the set holds what it is named for, by the independent walk, before a kernel is looked at."""
    w = {k: py_walk(s, e, max_moves) for k, (s, e) in sp.items()}
    pos, sm = w["full60"]
    assert len(sp["full60"][1]) == 60 and sm["positions"] == 61 and sm["blacks"] + sm["whites"] == 64 and sm["ended"] == END_RULES and pos[-1][3] == OVER
    pos, sm = w["auto_pass"]
    assert PA not in sp["auto_pass"][1] and any(a[2] == b[2] and a[3] == b[3] == SEARCH for a, b in zip(pos, pos[1:]))   # the same side moves twice
    pos, sm = w["pass_entry"]
    j = sp["pass_entry"][1].index(PA)
    assert pos[j][3] == PASS_ENTRY and pos[j + 1][:3] == pos[j][:3] and pos[j + 1][3] == SEARCH and pos[j - 1][2] == pos[j][2]
    assert sp["white_start"][0][2] == 2 and w["white_start"][0][0][2] == 2
    pos, sm = w["early_end"]
    assert sm["ended"] == END_RULES and sm["blacks"] + sm["whites"] < 64 and pos[-1][3] == OVER
    pos, sm = w["illegal_middle"]
    assert sm["ended"] == END_ILLEGAL and sm["positions"] == 14 and pos[13][3] == OVER and pos[13][:2] == pos[12][:2] and sm["winner"] == 3 - pos[12][2]
    assert len(sp["illegal_middle"][1]) > 13   # entries after the end
    pos, sm = w["after_end"]
    assert len(sp["after_end"][1]) == 63 and sm["positions"] == 61 and not sm["errors"]
    assert w["empty"][1]["positions"] == 1 and w["empty"][0][0][3] == SEARCH
    pos, sm = w["no_terminator"]
    assert len(sp["no_terminator"][1]) == max_moves and END not in sp["no_terminator"][1] and sm["positions"] == max_moves + 1 and pos[-1][3] == SEARCH
    pos, sm = w["bad_code"]
    assert sm["errors"] == BAD_CODE and sm["positions"] == 8 and pos[7][3] == SEARCH and pos[7][5] == END


def one_entry_games(n, seed=5):
    """n lists for max_moves = 1: a legal first move, a pass entry, an empty list, a bad code, a move that flips nothing - from the
    initial position and from positions of playouts, white to move among them."""
    rnd, out = Random(seed), []
    starts = [None] + [s for k in range(6) for s in playout(Random(seed + k), stop_discs=12 + 7 * k)[1][-1:]]
    for g in range(n):
        start = starts[g % len(starts)]
        b, w, p = start or INIT
        own, enemy = (b, w) if p == 1 else (w, b)
        kind = g % 7
        entry = [PA] if kind == 3 else [] if kind == 4 else [-7 if g % 2 else 99] if kind == 5 else \
            [no_flip_square((b, w, p))] if kind == 6 else [rnd.choice(py_legal(own, enemy))]
        out.append((start, entry))
    return out


def pack(games, max_moves):
    """(moves int8 [n, max_moves], (black, white, player) arrays or None when every game starts on the initial position)."""
    moves = np.full((len(games), max_moves), END, dtype=np.int8)
    for g, (_, entries) in enumerate(games):
        moves[g, :min(len(entries), max_moves)] = entries[:max_moves]
    if all(s is None for s, _ in games):
        return moves, None
    st = [s or INIT for s, _ in games]
    return moves, (np.array([s[0] for s in st], dtype=np.uint64), np.array([s[1] for s in st], dtype=np.uint64), np.array([s[2] for s in st], dtype=np.uint8))


# ---- case 1: the replay -----------------------------------------------------------------------------------------------------------
CB_ROOT_BLACK, CB_ROOT_WHITE, CB_PLAYER, CB_PHASE, CB_SIMS_PER_MOVE, CB_ONE_MOVE, CB_N_PLIES = 0, 8, 68, 76, 108, 92, 128


def _u32(cb, off):
    return cb[:, off:off + 4].copy().view(np.uint32).reshape(-1)


def _u64(cb, off):
    return cb[:, off:off + 8].copy().view(np.uint64).reshape(-1)


def check_replay(backend, engine, games, max_moves, sims=8, first_slot=0):
    """Start an analysis of `games` on `engine` and compare positions, states, summaries, error bits, counters, the guard and the
    slots' control blocks with the independent walk.  Returns the started analysis."""
    n, P = len(games), max_moves + 1
    moves, positions = pack(games, max_moves)
    before = backend.controls(engine)
    an = backend.analysis(engine, n, max_moves, first_slot=first_slot)
    an.start(moves, positions, sims)
    got_games, got_pos, got_evals = an.read()
    after = backend.controls(engine)
    want = [py_walk(s, e, max_moves) for s, e in games]
    armed = np.zeros(len(before), dtype=bool)
    for g, (pos, sm) in enumerate(want):
        for k in ("positions", "ended", "winner", "blacks", "whites", "errors", "searched"):
            assert int(got_games[g][k]) == sm[k], (g, k, got_games[g], sm)
        for j in range(P):
            r = got_pos[g, j]
            if j < len(pos):
                assert (int(r["black"]), int(r["white"]), int(r["player"]), int(r["state"]), int(r["moves_made"]), int(r["played"])) == pos[j], (g, j)
                assert int(r["pad"]) == 0
                armed[first_slot + g * P + j] = pos[j][3] == SEARCH
                assert int(got_evals[g, j]["state"]) == (1 if pos[j][3] == SEARCH else 0)
            else:
                assert r.tobytes() == bytes(24), (g, j, "a position beyond the walk")
            assert got_evals[g, j].tobytes()[1:] == bytes(127), (g, j, "an eval before any collect")
    st = an.stats()
    n_armed = sum(sm["searched"] for _, sm in want)
    err = 0
    for _, sm in want:
        err |= sm["errors"]
    assert st == dict(games=n, positions=sum(sm["positions"] for _, sm in want), armed=n_armed, pending=n_armed, searched=0, solved=0,
                      failed=0, error=err), st
    an.check_guard()
    assert (before[~armed] == after[~armed]).all(), "a slot that was not armed changed"
    # the armed slots: the mover's discs as "black", player 1, one move, `sims` simulations, waiting for their first step
    ab = after[armed]
    own = [p[0] if p[2] == 1 else p[1] for pos, _ in want for p in pos if p[3] == SEARCH]
    enemy = [p[1] if p[2] == 1 else p[0] for pos, _ in want for p in pos if p[3] == SEARCH]
    assert _u64(ab, CB_ROOT_BLACK).tolist() == own and _u64(ab, CB_ROOT_WHITE).tolist() == enemy
    assert (_u32(ab, CB_PLAYER) == 1).all() and (_u32(ab, CB_PHASE) == 0).all() and (_u32(ab, CB_SIMS_PER_MOVE) == sims).all()
    assert (_u32(ab, CB_ONE_MOVE) == 1).all() and (_u32(ab, CB_N_PLIES) == 0).all()
    return an, want


# ---- case 2: search and collect ---------------------------------------------------------------------------------------------------
def expected_evals(want, raw, max_moves, first_slot=0):
    """ANALYSIS_EVAL [n, P] from the walk and record 0 of a host-armed engine's slots."""
    from reversi_alpha_zero_amd.engine import ANALYSIS_EVAL, ANALYSIS_TOP
    P = max_moves + 1
    out = np.zeros((len(want), P), dtype=ANALYSIS_EVAL)
    for g, (pos, _) in enumerate(want):
        for j, p in enumerate(pos):
            if p[3] != SEARCH:
                continue
            s, e, played = first_slot + g * P + j, out[g, j], p[5]
            action = int(raw["action"][s])
            e["action"], e["played"] = action, played
            if int(raw["flags"][s]) & 1:
                n, q = np.uint32(raw["n"][s]), np.float64(raw["q"][s])
                e["state"], e["n_top"], e["sum_n"] = 3, 1, n
                e["top_square"][0], e["top_n"][0], e["top_q"][0] = action, n, q
                if played == action:
                    e["played_n"], e["played_q"] = n, q
                continue
            n = raw["root_n"][s].astype(np.uint32)
            q = raw["root_w"][s].astype(np.float64) / (n.astype(np.float64) + 1e-5)
            order = [int(a) for a in np.argsort(-n.astype(np.int64), kind="stable") if n[a] > 0][:ANALYSIS_TOP]
            e["state"], e["n_top"], e["sum_n"] = 2, len(order), n.sum(dtype=np.uint64)
            for k, a in enumerate(order):
                e["top_square"][k], e["top_n"][k], e["top_q"][k] = a, n[a], q[a]
            if played >= 0:
                e["played_n"], e["played_q"] = n[played], q[played]
    return out


def host_route(backend, cfg, blob, n_slots, seed, first_id, sims, want, max_moves, first_slot=0, step=8, **kw):
    """The expectation: a second engine of the same seed, its SEARCH slots armed one by one, stepped until every slot idles."""
    e = backend.engine(cfg, blob, n_slots, seed, sims, first_game_id=first_id, **kw)
    P = max_moves + 1
    for g, (pos, _) in enumerate(want):
        for j, p in enumerate(pos):
            if p[3] == SEARCH:
                own, enemy = (p[0], p[1]) if p[2] == 1 else (p[1], p[0])
                e.set_position(first_slot + g * P + j, own, enemy, 1, sims, enable_resign=False, one_move=True)
    for _ in range(100000):
        if e.stats()["idle_or_done"] >= n_slots:
            break
        e.step(step)
    else:
        raise AssertionError("the host route does not end")
    return expected_evals(want, backend.raw(e), max_moves, first_slot)


def run_device(backend, engine, an, step=4, collect_every=1, max_iterations=100000):
    """Step, collect, read the counters, until nothing is pending."""
    st = an.stats()
    it = 0
    while st["pending"]:
        for _ in range(collect_every):
            engine.step(step)
        an.collect()
        st = an.stats()
        assert not (st["error"] & ~BAD_CODE), st
        it += 1
        assert it < max_iterations, "the analysis does not end"
    assert st["searched"] + st["solved"] == st["armed"] and st["failed"] == 0
    return st


def assert_same_evals(tag, got, want):
    assert got.shape == want.shape
    for g in range(got.shape[0]):
        for j in range(got.shape[1]):
            assert got[g, j].tobytes() == want[g, j].tobytes(), (tag, g, j, got[g, j], want[g, j])


def case_search(backend, blob, games, max_moves, psn, seed=11, first_id=70, sims=8, **play):
    """Case 2 for one set of games: (device evals, expected evals, the walk)."""
    cfg = M.engine_cfg(M.mini_config(psn, sims=sims, **play))
    n_slots = len(games) * (max_moves + 1)
    e = backend.engine(cfg, blob, n_slots, seed, sims, first_game_id=first_id)
    an, want = check_replay(backend, e, games, max_moves, sims)
    run_device(backend, e, an)
    e.stats()   # raises on engine error flags
    got = an.read()[2]
    an.check_guard()
    exp = host_route(backend, cfg, blob, n_slots, seed, first_id, sims, want, max_moves)
    assert_same_evals((len(games), max_moves, psn), got, exp)
    return got, exp, want


# ---- case 7: a slot that leaves the one-move protocol -----------------------------------------------------------------------------
def case_slot_off_protocol(backend, blob, psn=1):
    """tests/match_cases.py's case 7 for the analysis: three positions, one per game, and the slot of game 1's is re-armed outside
    one-move mode behind the start.  Its eval is ERROR with flags 0x100 exactly, the error word is 0x100, the engine reports no error
    flag, and the two other evals are those of the undisturbed analysis, byte for byte."""
    from reversi_alpha_zero_amd.engine import EVAL_ERROR, EVAL_SEARCHED, EVAL_SOLVED
    seed, first_id, sims, play = 11, 70, 8, dict(use_solver_turn=0, use_solver_turn_in_simulation=0)
    cfg = M.engine_cfg(M.mini_config(psn, sims=sims, **play))
    games = [(pos, []) for pos in M.playout_positions(11, 3, 50)]
    clean = case_search(backend, blob, games, 1, psn, seed=seed, first_id=first_id, sims=sims, **play)[0]
    e = backend.engine(cfg, blob, 6, seed, sims, first_game_id=first_id)
    an, want = check_replay(backend, e, games, 1, sims)
    b, w, p = games[1][0]
    assert want[1][0][0][3] == SEARCH
    M.rearm_outside_one_move(e, 1 * 2 + 0, b, w, p, sims)
    st = an.stats()
    for _ in range(100000):
        if not st["pending"]:
            break
        e.step(4)
        an.collect()
        e.stats()   # raises on engine error flags
        st = an.stats()
        assert st["error"] in (0, 0x100), st
    assert (st["pending"], st["failed"], st["searched"] + st["solved"], st["error"]) == (0, 1, 2, 0x100), st
    got = an.read()[2]
    an.check_guard()
    assert (int(got[1, 0]["state"]), int(got[1, 0]["flags"]), int(got[1, 0]["action"])) == (EVAL_ERROR, 0x100, -1), got[1, 0]
    for g in (0, 2):
        assert int(clean[g, 0]["state"]) in (EVAL_SEARCHED, EVAL_SOLVED) and got[g, 0].tobytes() == clean[g, 0].tobytes(), (g, got[g, 0], clean[g, 0])
    assert got[:, 1].tobytes() == clean[:, 1].tobytes()
