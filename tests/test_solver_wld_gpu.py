"""GPU: raz_solve_wld (include/raz.h; csrc/raz_solver_wld.hip) and ReversiSolver.solve_wld / solve_wld_batch against the yardsticks
of tests/solver_wld_cases.py - the signs of ab_check's exact root values on every existing list, the recorded root values at 15..17
empties, the recorded answers of tests/native/wld_check.c at 18 empties and above - against the sign of raz_solve_exact's score of
the same build, and against itself under every tuning.  Every comparison is exact equality of move, outcome and status; every round
loop is the library's own capped one."""
import numpy as np
import pytest

import solver_exact_cases as X
import solver_wld_cases as W

pytestmark = pytest.mark.gpu


def _dev(cases):
    import torch
    b, w, p = W.arrays(cases)
    return (torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda())


def solve(cases, tuning=0, ws_bytes=None, max_empties=17, expect=W.RAZ_OK, stream=None, visits=None, exact=False):
    """(move, outcome, status) as numpy arrays; the outputs start as 0x55 so that an untouched byte shows.  exact=True:
    raz_solve_exact instead."""
    import torch
    from reversi_alpha_zero_amd._native import lib, last_error
    n = len(cases)
    b, w, p = _dev(cases) if n else (None, None, None)
    mv = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    sc = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    size = lib.raz_solve_exact_workspace_bytes if exact else lib.raz_solve_wld_workspace_bytes
    ws_bytes = size(n, max_empties) + min(n * 65536, 1 << 30) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in (b, w, p)] if n else [None, None, None]
    call = lib.raz_solve_exact if exact else lib.raz_solve_wld
    rc = call(*ptrs, n, mv.data_ptr(), sc.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes, tuning, s.cuda_stream)
    assert rc == expect, (rc, last_error())
    torch.cuda.synchronize()
    if visits is not None:
        visits.append(int(ws[:8].cpu().numpy().view(np.uint64)[0]))
    return mv.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _untouched(got):
    return all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)


def test_golden_and_random_positions():
    """G and R(1..12), each list one batch; the coverage conditions hold over the lists."""
    W.assert_wld_coverage()
    for name, cases in W.gpu_lists().items():
        W.assert_answers(solve(cases, max_empties=14), cases, 1, name)


def test_deep_positions_of_the_batch_solver():
    cases = W.deep_cases()
    W.assert_answers(solve(cases, max_empties=14), cases, 1, "deep 13 / 14")


@pytest.mark.parametrize("empties", sorted(X.DEEP2_COUNTS))
def test_positions_of_15_to_17_empties(empties):
    """The answers that follow from ab_check's recorded root values: one batch per depth."""
    cases = [c for c in W.deep2_cases() if W.empties_of(c) == empties]
    assert len(cases) == X.DEEP2_COUNTS[empties]
    W.assert_answers(solve(cases, max_empties=empties), cases, 1, f"{empties} empties")


@pytest.mark.parametrize("empties", range(18, W.MAX_EMPTIES + 1))
def test_positions_beyond_the_exact_solvers_limit(empties):
    """The recorded answers of wld_check: one batch per depth - every row below limit - 1, the first two rows at limit - 1 and at
    the limit."""
    cases = [c for c in W.deep3_cases() if W.empties_of(c) == empties]
    assert len(cases) == W.DEEP3_COUNTS[empties]
    if empties >= W.MAX_EMPTIES - 1:
        cases = cases[:2]
    W.assert_answers(solve(cases, max_empties=empties), cases, 1, f"{empties} empties")


def test_the_mixed_list_against_the_sign_of_the_exact_solver():
    cases = W.mixed_wld()
    mine, theirs = solve(cases, max_empties=15), solve(cases, max_empties=15, exact=True)
    assert mine[2].tobytes() == theirs[2].tobytes()
    solved = mine[2] == 0
    assert (mine[1][solved] == np.sign(theirs[1][solved])).all()
    assert (mine[0][~solved] == -1).all() and (mine[1][~solved] == -100).all()
    assert (mine[0][solved] != theirs[0][solved]).sum() >= 10   # (the two calls name different moves on many rows)


def test_status_rows():
    cases = W.status_cases()
    W.assert_answers(solve(cases, max_empties=15), cases, 1, "status rows")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_batch_edges(n):
    cases = W.cycled(W.mixed_wld(), n)
    got = solve(cases, max_empties=15)
    if n == 0:
        return
    W.assert_answers(got, cases, 1, f"n={n}")


def test_rows_alone_and_in_the_batch():
    cases = W.mixed_wld()[:40]
    together = solve(cases, max_empties=15)
    for i, c in enumerate(cases):
        alone = solve([c], max_empties=15)
        assert all(int(a[0]) == int(t[i]) for a, t in zip(alone, together)), i


_PARTITION = {}


def _partition_list():
    """257 mixed rows, one 15- and one 16-empties fixture row, answered once under tuning 0 (and checked): shared by the cases below."""
    if not _PARTITION:
        deep2 = W.deep2_cases()
        cases = W.mixed_wld(257) + deep2[:1] + deep2[8:9]
        assert [W.empties_of(c) for c in cases[-2:]] == [15, 16]
        base = solve(cases, max_empties=16)
        W.assert_answers(base, cases, 1, "tuning 0")
        _PARTITION.update(cases=cases, base=base)
    return _PARTITION["cases"], _PARTITION["base"]


_VARIANTS = list(W.tunings()) + ["minimum workspace", "twice the minimum"]


@pytest.mark.parametrize("name", _VARIANTS)
def test_partition_independence(name):
    """EVERY tuning of tunings(), the minimum workspace and twice it, on the whole list - the 16-empties row included: a record of
    more than 15 empties is split whatever the tuning says - on a stream of its own: byte-identical to tuning 0."""
    import torch
    from reversi_alpha_zero_amd._native import lib
    cases, base = _partition_list()
    least = lib.raz_solve_wld_workspace_bytes(len(cases), 16)
    tuning = W.tunings().get(name, 0)
    ws_bytes = {"minimum workspace": least, "twice the minimum": 2 * least}.get(name)
    got = solve(cases, tuning=tuning, ws_bytes=ws_bytes, max_empties=16, stream=torch.cuda.Stream())
    for a, b in zip(got, base):
        assert a.tobytes() == b.tobytes(), (name, hex(tuning), ws_bytes)


def test_two_streams_twice():
    """The same list on two streams, twice each: byte-identical to the run on the current stream."""
    import torch
    cases, base = _partition_list()
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        for rep in range(2):
            got = solve(cases, max_empties=16, stream=stream)
            for a, b in zip(got, base):
                assert a.tobytes() == b.tobytes(), rep


def test_a_parked_task_is_dropped_on_resume():
    """Budget 3, 9-empties rows split 3 plies to leaf 4: tasks whose ancestor is decided while they are parked are dropped when they
    resume - fewer visits than with cuts off - and no task goes missing: the answers are right."""
    cases = W.random_cases(9, 16)
    tuning = W.TUNE_BUDGET[3] | W.TUNE_SPLIT(3) | W.TUNE_LEAF(4)
    on, off = [], []
    W.assert_answers(solve(cases, tuning=tuning, visits=on), cases, 1, "cuts on")
    W.assert_answers(solve(cases, tuning=tuning | W.TUNE_NO_CUTS, visits=off), cases, 1, "cuts off")
    assert 0 < on[0] < off[0], (on, off)


def test_refusals_leave_the_outputs_alone():
    from reversi_alpha_zero_amd._native import lib
    cases = W.cycled(W.mixed_wld(), 65)
    n = len(cases)
    sizes = [lib.raz_solve_wld_workspace_bytes(n, e) for e in range(W.MAX_EMPTIES + 1)]
    for short in (sizes[15] - 1, sizes[0] - 1):
        assert _untouched(solve(cases, ws_bytes=short, expect=W.RAZ_EINVAL))
    for bad in (1 << 27, 1 << 31, W.TUNE_LEAF(1), W.TUNE_LEAF(W.MAX_EMPTIES + 1), 7 << 20):
        assert _untouched(solve(cases, tuning=bad, expect=W.RAZ_EINVAL))


def test_fewer_visits_than_the_exact_solver():
    """R(12): strictly fewer node visits than raz_solve_exact on the same rows, and the sign of its score."""
    cases = W.random_cases(12)
    mine, theirs = [], []
    a, b = solve(cases, max_empties=12, visits=mine), solve(cases, max_empties=12, visits=theirs, exact=True)
    W.assert_answers(a, cases, 1, "R12")
    assert (a[1] == np.sign(b[1])).all()
    assert 0 < mine[0] < theirs[0], (mine, theirs)


def test_the_python_class():
    import torch
    from reversi_alpha_zero_amd.lib.reversi_solver import ReversiSolver, WLD_MAX_EMPTIES
    assert WLD_MAX_EMPTIES == W.MAX_EMPTIES
    s = ReversiSolver()
    cases = W.status_cases() + W.random_cases(9, 8)
    mv, sc, st = s.solve_wld_batch(*_dev(cases))
    assert mv.is_cuda and mv.dtype == torch.int8 and st.dtype == torch.uint8
    W.assert_answers((mv.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), cases, 1, "solve_wld_batch")
    for b, w, p, status, ans in cases:
        if status == 0:
            assert s.solve_wld(b, w, p) == ans[1]
        elif status == 1:
            assert s.solve_wld(b, w, p) == (None, None)
        elif status == 2:
            with pytest.raises(ValueError, match=str(W.MAX_EMPTIES)):
                s.solve_wld(b, w, p)
        elif p in (1, 2):
            with pytest.raises(ValueError, match="not a position"):
                s.solve_wld(b, w, p)
    with pytest.raises(ValueError):
        s.solve_wld_batch(*(t.cpu() for t in _dev(cases)))


def test_analyze_with_wld_empties():
    """GameAnalyzer.analyze(games, exact_empties=12, wld_empties=17) on two short mini-net games from 17 empties at 8 sims a move:
    every added field equals solve_wld called per position; without wld_empties the dictionaries are today's."""
    import random
    from test_analysis_gpu import _python_config
    from test_match_gpu import DEV
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.lib.analysis import GameAnalyzer
    from reversi_alpha_zero_amd.lib.reversi_solver import ReversiSolver
    rng, games = random.Random(11), []
    for b, w, p in W.random_positions(17, 2, 9317):   # two games from 17 empties to their ends (random moves, passes as None)
        b0, w0, p0, actions = b, w, p, []
        while True:
            own, enemy = (b, w) if p == 1 else (w, b)
            legal = W.moves_of(own, enemy)
            if not legal:
                if not W.moves_of(enemy, own):
                    break
                actions.append(None)
                p = 3 - p
                continue
            a = rng.choice(W.squares(legal))
            actions.append(a)
            own, enemy = W.play(a, own, enemy)
            b, w = (own, enemy) if p == 1 else (enemy, own)
            p = 3 - p
        games.append((b0, w0, p0, actions))
    cfg = _python_config(1)
    net = ReversiNet(16, 1, 16).keras_init_(1).randomize_bn_(2)
    ga = GameAnalyzer(cfg, net, cfg.play, slots=64, device=DEV)
    exact, both = ga.analyze(games, exact_empties=12), ga.analyze(games, exact_empties=12, wld_empties=17)
    assert ga.analyze(games) == ga.analyze(games, wld_empties=None)
    added = {"solved_outcome", "outcome_move", "played_outcome", "outcome_kept"}
    solver, seen = ReversiSolver(DEV), {"solved": 0, "played": 0, "not kept": 0, "exact": 0}
    for gx, gb in zip(exact, both):
        assert len(gx) == len(gb)
        for i, (dx, db) in enumerate(zip(gx, gb)):
            assert {k: v for k, v in db.items() if k not in added} == dx
            e = 64 - bin(db["black"] | db["white"]).count("1")
            if db["state"] == "over" or e <= 12:
                assert not (added & set(db))
                seen["exact"] += "solved_score" in db
                continue
            mv, o = solver.solve_wld(db["black"], db["white"], db["player"])
            if mv is None:   # a pass entry whose side to move cannot move: the position after it, from this side's view
                assert db["state"] == "pass_entry" and db["outcome_move"] is None
                continue
            assert (db["outcome_move"], db["solved_outcome"]) == (mv, o)
            seen["solved"] += 1
            if db["played"] is None:
                continue
            own, enemy = (db["black"], db["white"]) if db["player"] == 1 else (db["white"], db["black"])
            no, ne = W.play(db["played"], own, enemy)   # the played move's outcome: the position after it, solved on its own
            other = 3 - db["player"]
            if W.moves_of(ne, no):
                want = -solver.solve_wld(*((ne, no) if other == 1 else (no, ne)), other)[1]
            elif W.moves_of(no, ne):
                want = solver.solve_wld(*((no, ne) if db["player"] == 1 else (ne, no)), db["player"])[1]
            else:
                want = W.sign(bin(no).count("1") - bin(ne).count("1"))
            assert db["played_outcome"] == want and db["outcome_kept"] is (want == o)
            seen["played"] += 1
            seen["not kept"] += not db["outcome_kept"]
    assert seen["solved"] >= 8 and seen["played"] >= 8 and seen["exact"] > 0, seen
    with pytest.raises(ValueError):
        ga.analyze(games, wld_empties=W.MAX_EMPTIES + 1)
