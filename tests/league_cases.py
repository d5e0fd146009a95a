"""Shared cases of the device league (include/raz.h raz_league_*, csrc/raz_league.h), run by tests/test_league_emu.py on the wave
emulator and by tests/test_league_gpu.py on the device.

Both drive the product's engine.DeviceLeague.  A BACKEND (tests/match_cases.py's Adapter) gives the cases
    backend.league(engines, n_games, guard=...)   a LeagueHarness: start(pairings, positions, sims, enable_resign) with pairings a
                                                  list of (black_model, black_slot, white_model, white_slot), turn(), stats() ->
                                                  dict, read() -> (games, pairings, plies, root_n), workspace(), check_guard()
    backend.blocks(engine)                        the control blocks of every slot, uint8 [n_games, 256]

The EXPECTATION of every case is drive_host_league: ReversiEnv objects and one set_position call per ply on the mapped slot, which
looks at no league kernel."""
import numpy as np

import match_cases as C
from match_cases import GUARD
SIZES = (5, 7, 9)          # case 2: the three engines' slots
SEEDS = (48, 49, 50)
FIRSTS = (100, 200, 300)
# case 2: (black_model, black_slot, white_model, white_slot).  Slots out of order; model 1's slot 1 and model 2's slots 2 and 4 unused;
# every ordered pair of models; every model plays both colours.
PAIRINGS = [(0, 4, 1, 0), (1, 6, 0, 2), (0, 0, 2, 8), (2, 3, 0, 1), (1, 2, 2, 5), (2, 0, 1, 5), (1, 3, 2, 6), (2, 7, 0, 3), (1, 4, 2, 1)]
SPECIAL = ["pass", "white", "one_empty", "dead_end"]


def mini_blobs3():
    """Three mini nets (16 filters, 1 residual layer, value_fc 16), seeds 1, 2, 3."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return [ReversiNet(16, 1, 16).keras_init_(s).randomize_bn_(s + 1).to_blob() for s in (1, 2, 3)]


class LeagueHarness(C.Guarded):
    """engine.DeviceLeague behind the interface of the cases, in a guarded workspace."""

    def __init__(self, backend, engines, n_games, guard=GUARD):
        import ctypes
        from reversi_alpha_zero_amd.engine import DeviceLeague
        slots = (ctypes.c_uint32 * len(engines))(*[e.n_games for e in engines])
        super().__init__(backend, engines[0].lib.raz_league_workspace_bytes(len(engines), slots, n_games), guard)
        self.w, self.n = DeviceLeague(engines, workspace=self.given), n_games

    def start(self, pairings, positions, sims, enable_resign=True):
        from reversi_alpha_zero_amd.engine import league_pairings
        assert len(pairings) == self.n
        pr = self.backend.tensor(league_pairings(pairings).view(np.uint8).reshape(self.n, 16))
        self.w.start(pr, self.backend.positions(positions), sims, enable_resign)

    def turn(self):
        self.w.turn()

    def read(self):
        return self.w.read()


def three_engines(backend, cfg, blobs, sims=8, **kw):
    return lambda: [backend.engine(cfg, blobs[m], SIZES[m], SEEDS[m], sims, first_game_id=FIRSTS[m], **kw) for m in range(3)]


def case2_positions():
    sp = C.special_positions()
    return [sp[k] for k in SPECIAL] + C.playout_positions(21, len(PAIRINGS) - len(SPECIAL), 50)


# ---- the rule of raz_league_start, in Python ------------------------------------------------------------------------------------
def expected_started(pairings, sizes):
    """Which games raz_league_start starts: sound pairings whose two slots are claimed by no lower SOUND game index."""
    sound = [bm < len(sizes) and wm < len(sizes) and bm != wm and bs < sizes[bm] and ws < sizes[wm] for bm, bs, wm, ws in pairings]
    claim = {}
    for g, (bm, bs, wm, ws) in enumerate(pairings):
        if sound[g]:
            claim.setdefault((bm, bs), g)
            claim.setdefault((wm, ws), g)
    return [sound[g] and claim[(bm, bs)] == g and claim[(wm, ws)] == g for g, (bm, bs, wm, ws) in enumerate(pairings)]


def unused_slots(pairings, started, sizes):
    used = {(m, s) for (bm, bs, wm, ws), on in zip(pairings, started) if on for m, s in ((bm, bs), (wm, ws))}
    return [(m, s) for m in range(len(sizes)) for s in range(sizes[m]) if (m, s) not in used]


# ---- the two drivers --------------------------------------------------------------------------------------------------------------
def _result(env, bm, wm):
    from reversi_alpha_zero_amd.env.reversi_env import Winner
    winner = bm if env.winner == Winner.black else wm if env.winner == Winner.white else None
    return winner, bm, wm, tuple(env.observation.number_of_black_and_white)


def drive_host_league(backend, make_engines, pairings, positions=None, sims=8, enable_resign=True, step=16):
    """The independent driver: (per game [(model, action, root_n list)], per game (winner model or None, black_model, white_model,
    (blacks, whites))).  sims: one number or one per model."""
    from reversi_alpha_zero_amd.env.reversi_env import Player, ReversiEnv
    engines = make_engines()
    per = [sims] * len(engines) if np.isscalar(sims) else list(sims)
    n = len(pairings)
    envs = [ReversiEnv().reset() if positions is None else ReversiEnv().update(positions[g][0], positions[g][1], Player(positions[g][2]))
            for g in range(n)]
    plies, live = [[] for _ in range(n)], list(range(n))
    while live:
        armed = [[] for _ in engines]
        for g in live:
            bm, bs, wm, ws = pairings[g]
            m, s = (bm, bs) if envs[g].next_player == Player.black else (wm, ws)
            own, enemy = envs[g].get_own_and_enemy()
            engines[m].set_position(s, own, enemy, 1, per[m], enable_resign=enable_resign, one_move=True)
            armed[m].append((g, s))
        for m, e in enumerate(engines):
            if not armed[m]:
                continue
            while e.stats()["idle_or_done"] < e.n_games:
                e.step(step)
            actions, root_n = backend.answers(e)
            for g, s in armed[m]:
                a = int(actions[s])
                plies[g].append((m, a, [int(x) for x in root_n[s]]))
                envs[g].step(a if a >= 0 else None)
        live = [g for g in live if not envs[g].done]
    return plies, [_result(envs[g], pairings[g][0], pairings[g][2]) for g in range(n)]


def drive_league(backend, make_engines, pairings, positions=None, sims=8, enable_resign=True, step=4, turn_every=1, started=None,
                 between=None, max_iterations=100000, after_start=None, error=0):
    """The same games through raz_league_*: step every engine `turn_every` times by `step`, hand off, read the counters.  started: which
    games raz_league_start is expected to start (None: all).  between(engines, league): called once, after the first hand-off;
    after_start(engines, league): called once, behind the start.  error: the error word the league is to end with, beside PAIRING.
    The league's workspace lies between guard bytes, checked at the end; the control blocks of all slots no started game names are
    compared before start and after the last turn."""
    from reversi_alpha_zero_amd.engine import LEAGUE_ERR_PAIRING, LEAGUE_GAME_NOT_STARTED, league_games, league_results
    engines = make_engines()
    n = len(pairings)
    started = [True] * n if started is None else started
    allowed = 0 if all(started) else LEAGUE_ERR_PAIRING
    idle = unused_slots(pairings, started, [e.n_games for e in engines])
    blocks = [backend.blocks(e) for e in engines]
    league = backend.league(engines, n, guard=GUARD)
    league.start(pairings, positions, sims, enable_resign)
    st = league.stats()
    assert st["live"] == sum(started) and sum(st["searching"]) == st["live"] and st["plies"] == 0 and st["error"] == allowed, st
    assert st["n_models"] == len(engines)
    games = league.read()[0]
    assert [bool(f & LEAGUE_GAME_NOT_STARTED) for f in games["flags"]] == [not s for s in started]
    assert all((sr != 0) == on for sr, on in zip(games["searching"], started))
    if after_start is not None:
        after_start(engines, league)
    it = 0
    while st["live"]:
        for _ in range(turn_every):
            for e in engines:
                e.step(step)
        league.turn()
        if between is not None and it == 0:
            between(engines, league)
        for e in engines:
            e.stats()   # raises on engine error flags
        st = league.stats()
        assert st["error"] in (allowed, allowed | error), st
        it += 1
        assert it < max_iterations, "the league does not end"
    assert st["error"] == allowed | error and sum(st["searching"]) == 0, st
    games, kept, log, root_n = league.read()
    assert [(int(p["black_model"]), int(p["black_slot"]), int(p["white_model"]), int(p["white_slot"])) for p in kept] == [tuple(p) for p in pairings]
    assert st["plies"] == int(games["n_plies"].sum())
    got = league_games(games, log, root_n)
    after = [backend.blocks(e) for e in engines]
    for m, s in idle:
        assert (blocks[m][s] == after[m][s]).all(), ("an unused slot's control block changed", m, s)
    league.check_guard()
    plies = [[(p["who"], p["action"], [int(x) for x in p["root_n"]]) for p in g["plies"]] for g in got]
    return plies, league_results(games)


def assert_same(tag, got, want, only=None):
    (gp, gr), (wp, wr) = got, want
    assert len(gp) == len(wp)
    for g in (range(len(gp)) if only is None else only):
        assert [(w, x) for w, x, _ in gp[g]] == [(w, x) for w, x, _ in wp[g]], (tag, g)
        for i, (p, q) in enumerate(zip(gp[g], wp[g])):
            assert p[2] == q[2], (tag, g, i, "root_n")
        assert gr[g] == wr[g], (tag, g, gr[g], wr[g])


def pick(run, games):
    return [run[0][g] for g in games], [run[1][g] for g in games]


# ---- case 1: two models, identity slots, equals raz_match_* -----------------------------------------------------------------------
def as_match(run):
    """A two-model league's logs and results in drive_match's terms: model 0 the best model, model 1 the challenger."""
    plies, results = run
    return ([[("ng" if w else "best", a, rn) for w, a, rn in g] for g in plies],
            [(None if w is None else int(w == 1), bm == 0, counts) for w, bm, wm, counts in results])


def case_equals_match(backend, blobs, n, psn, positions, want_match=None, want_host=None):
    cfg = C.engine_cfg(C.mini_config(psn, use_solver_turn=0, use_solver_turn_in_simulation=0))
    bib = [(g * 7 // 3) % 2 == 0 for g in range(n)]
    args = (backend, cfg, blobs, n, 9, 300, 8, bib, positions)
    want_host = want_host or C.drive_host(*args)
    want_match = want_match or C.drive_match(*args)

    def make():
        sides = C._engines(backend, cfg, blobs, n, 9, 300, 8)
        return [sides[True], sides[False]]
    pairings = [(0, g, 1, g) if bib[g] else (1, g, 0, g) for g in range(n)]
    got = as_match(drive_league(backend, make, pairings, positions))
    C.assert_same(("league == raz_match_*", n, psn), got, want_match)
    C.assert_same(("league == host driver", n, psn), got, want_host)


# ---- case 2: three models, scattered slots, engines of different sizes ----------------------------------------------------------
def case_three_models(backend, blobs, psn):
    """Returns (cfg, positions, the host driver's run) for case 3."""
    cfg = C.engine_cfg(C.mini_config(psn))
    positions = case2_positions()
    make = three_engines(backend, cfg, blobs)
    want = drive_host_league(backend, make, PAIRINGS, positions)
    again = drive_host_league(backend, make, PAIRINGS, positions, step=3)
    assert_same("host driver agrees with itself", again, want)
    wp, wr = want
    g = SPECIAL.index("pass")      # the mover of ply 0 moves again
    assert len(wp[g]) >= 2 and wp[g][0][0] == wp[g][1][0], ("no pass", wp[g][:2])
    g = SPECIAL.index("white")     # white to move, and white's model is not black's
    assert positions[g][2] == 2 and wp[g][0][0] == PAIRINGS[g][2] != PAIRINGS[g][0]
    g = SPECIAL.index("one_empty")
    assert len(wp[g]) == 1 and wp[g][0][1] >= 0 and sum(wr[g][3]) == 64, "not a last square"
    g = SPECIAL.index("dead_end")  # neither side can move, squares empty
    assert len(wp[g]) == 1 and wp[g][0][1] >= 0 and sum(wr[g][3]) < 64, "no early end"
    assert {(bm, wm) for bm, _, wm, _ in PAIRINGS} == {(a, b) for a in range(3) for b in range(3) if a != b}
    assert all({bm for bm, _, _, _ in PAIRINGS} >= {m} and {wm for _, _, wm, _ in PAIRINGS} >= {m} for m in range(3))
    assert unused_slots(PAIRINGS, [True] * len(PAIRINGS), SIZES) == [(1, 1), (2, 2), (2, 4)]
    assert_same("three models", drive_league(backend, make, PAIRINGS, positions), want)
    # a resign threshold no search value reaches: the mover of every game resigns at once (turn >= allowed_resign_turn 0)
    rcfg = C.engine_cfg(C.mini_config(psn, resign_threshold=2.0, allowed_resign_turn=0))
    rpair = [PAIRINGS[1], PAIRINGS[4], PAIRINGS[7]]
    rpos = [C.special_positions()["white"]] + C.playout_positions(3, 2, 30)   # (before use_solver_turn: the search decides, and resigns)
    rmake = three_engines(backend, rcfg, blobs)
    rwant = drive_host_league(backend, rmake, rpair, rpos)
    assert all(len(p) == 1 and p[0][1] == -1 for p in rwant[0]), ("no resignation", rwant[0])
    assert [r[0] for r in rwant[1]] == [(bm, wm)[pos[2] == 1] for (bm, _, wm, _), pos in zip(rpair, rpos)]   # the resigner's opponent wins
    assert_same("resignation", drive_league(backend, rmake, rpair, rpos), rwant)
    off = drive_league(backend, rmake, rpair, rpos, enable_resign=False)
    assert all(p[0][1] >= 0 for p in off[0]), "enable_resign = 0 must reach the slots"
    return cfg, positions, want


# ---- case 3: independence ---------------------------------------------------------------------------------------------------------
def case_independence(backend, blobs, cfg, positions, want):
    make = three_engines(backend, cfg, blobs)
    for g in (0, 4, 7):   # alone: the same slots of the same engines
        alone = drive_league(backend, make, [PAIRINGS[g]], [positions[g]], step=1, turn_every=1)
        assert_same(("alone", g), alone, pick(want, [g]))
    assert_same("a hand-off every 16 steps", drive_league(backend, make, PAIRINGS, positions, step=1, turn_every=16), want)
    order = [5, 2, 8, 0, 7, 3, 6, 1, 4]
    permuted = drive_league(backend, make, [PAIRINGS[g] for g in order], [positions[g] for g in order])
    assert_same("the pairing array permuted", permuted, pick(want, order))


# ---- case 4: bad pairings ---------------------------------------------------------------------------------------------------------
# Slot 1 of model 0 is named by games 4 and 6.  The game index IS the position in the array, so the lower index cannot lie behind the
# higher one; what can differ is the order of the claims: game 4 names the slot as its WHITE slot (its second claim), game 6 as its
# BLACK slot (its first).
BAD_PAIRINGS = [(0, 0, 1, 0), (3, 0, 1, 1), (1, 2, 1, 3), (0, 5, 2, 0), (2, 1, 0, 1), (1, 4, 2, 2), (0, 1, 2, 3), (2, 5, 1, 5)]


def case_bad_pairings(backend, blobs, psn):
    from reversi_alpha_zero_amd.engine import LEAGUE_ERR_PAIRING
    cfg = C.engine_cfg(C.mini_config(psn))
    make = three_engines(backend, cfg, blobs)
    started = expected_started(BAD_PAIRINGS, SIZES)
    assert started == [True, False, False, False, True, True, False, True]
    positions = C.playout_positions(31, len(BAD_PAIRINGS), 50)
    good = [g for g, s in enumerate(started) if s]
    clean = drive_league(backend, make, [BAD_PAIRINGS[g] for g in good], [positions[g] for g in good])
    assert_same("the clean league equals the host driver", clean,
                drive_host_league(backend, make, [BAD_PAIRINGS[g] for g in good], [positions[g] for g in good]))
    got = drive_league(backend, make, BAD_PAIRINGS, positions, started=started)   # asserts flags, live and LEAGUE_ERR_PAIRING
    assert_same("the started games of a league with bad pairings", pick(got, good), clean)
    for g, on in enumerate(started):
        if not on:
            assert got[0][g] == [] and got[1][g][0] is None and got[1][g][3] == (0, 0)
    assert LEAGUE_ERR_PAIRING == 0x800


# ---- case 5: a searching slot that leaves the one-move protocol -------------------------------------------------------------------
def case_slot_off_protocol(backend, blobs, psn=1):
    """tests/match_cases.py's case 7 in a league of three: game 1's searching slot is re-armed outside one-move mode behind the start.
    The game ends undecided with error word 0x100 exactly, no engine reports an error flag, the searching counters end at 0, and games
    0 and 2 are the games of the undisturbed league."""
    cfg = C.engine_cfg(C.mini_config(psn, use_solver_turn=0, use_solver_turn_in_simulation=0))
    make, pairings, positions = three_engines(backend, cfg, blobs), PAIRINGS[:3], C.playout_positions(11, 3, 50)
    clean = drive_league(backend, make, pairings, positions)
    kept = {}

    def rearm(engines, league):
        g = league.read()[0][1]
        assert g["searching"] in (1, 2) and g["n_plies"] == 0
        model, slot = pairings[1][0:2] if g["searching"] == 1 else pairings[1][2:4]
        C.rearm_outside_one_move(engines[model], slot, g["black"], g["white"], g["player"], 8)
        kept["league"] = league
    got = drive_league(backend, make, pairings, positions, after_start=rearm, error=0x100)   # (asserts the final error word, the counters, e.stats())
    games = kept["league"].read()[0]
    assert (int(games[1]["searching"]), int(games[1]["winner"]), int(games[1]["n_plies"])) == (0, 0, 0), games[1]
    assert got[0][1] == [] and got[1][1][0] is None
    assert all(len(clean[0][g]) > 0 and games[g]["winner"] != 0 for g in (0, 2))
    assert_same("beside a slot off the protocol", got, clean, only=(0, 2))
