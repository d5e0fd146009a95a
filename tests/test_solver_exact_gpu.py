"""GPU: raz_solve_exact (include/raz.h; csrc/raz_solver_exact.hip) and ReversiSolver.solve_exact / solve_exact_batch against the
yardsticks of tests/solver_exact_cases.py - the reference's compiled Cython solver, the oracle at 1..12 empties, the recorded oracle
answers at 13 / 14, the recorded answers of tests/native/ab_check.c at 15..17 - against raz_solve_batch(exactly = 1) of the same
build, and against itself under every tuning.  Every comparison is exact equality of move, score and status; every round loop is
the library's own capped one."""
import numpy as np
import pytest

import solver_exact_cases as X

pytestmark = pytest.mark.gpu


def _dev(cases):
    import torch
    b, w, p = X.arrays(cases)
    return (torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda())


def solve(cases, tuning=0, ws_bytes=None, max_empties=X.MAX_EMPTIES, expect=X.RAZ_OK, stream=None, visits=None, batch=False):
    """(move, score, status) as numpy arrays; the outputs start as 0x55 so that an untouched byte shows.  batch=True:
    raz_solve_batch(exactly = 1) instead."""
    import torch
    from reversi_alpha_zero_amd._native import lib, last_error
    n = len(cases)
    b, w, p = _dev(cases) if n else (None, None, None)
    mv = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    sc = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    size = lib.raz_solve_batch_workspace_bytes if batch else lib.raz_solve_exact_workspace_bytes
    ws_bytes = size(n, 14 if batch else max_empties) + min(n * 65536, 1 << 30) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() if n else None for t in (b, w, p)] if n else [None, None, None]
    if batch:
        rc = lib.raz_solve_batch(*ptrs, n, 1, mv.data_ptr(), sc.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes, 0, s.cuda_stream)
    else:
        rc = lib.raz_solve_exact(*ptrs, n, mv.data_ptr(), sc.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes, tuning, s.cuda_stream)
    assert rc == expect, (rc, last_error())
    torch.cuda.synchronize()
    if visits is not None:
        visits.append(int(ws[:8].cpu().numpy().view(np.uint64)[0]))
    return mv.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _untouched(got):
    return all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)


def test_golden_and_random_positions():
    """G and R(1..12), each list one batch; the coverage conditions (tied maxima among them) hold over the lists."""
    X.assert_exact_coverage()
    for name, cases in X.gpu_lists().items():
        X.assert_answers(solve(cases, max_empties=14), cases, 1, name)


def test_deep_positions_of_the_batch_solver():
    cases = X.deep_cases()
    X.assert_answers(solve(cases, max_empties=14), cases, 1, "deep 13 / 14")


@pytest.mark.parametrize("empties", sorted(X.DEEP2_COUNTS))
def test_positions_beyond_14_empties(empties):
    """The recorded answers of ab_check at 15..17 empties: one batch per depth."""
    cases = [c for c in X.deep2_cases() if 64 - bin(c[0] | c[1]).count("1") == empties]
    assert len(cases) == X.DEEP2_COUNTS[empties]
    X.assert_answers(solve(cases, max_empties=empties), cases, 1, f"{empties} empties")


def test_the_mixed_list_against_the_batch_solver():
    cases = [c for c in X.mixed_exact() if 64 - bin(c[0] | c[1]).count("1") <= 14]
    mine, theirs = solve(cases, max_empties=14), solve(cases, batch=True)
    for a, b in zip(mine, theirs):
        assert a.tobytes() == b.tobytes()


def test_status_rows():
    cases = X.status_cases()
    X.assert_answers(solve(cases), cases, 1, "status rows")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_batch_edges(n):
    cases = X.cycled(X.mixed_exact(), n)
    got = solve(cases, max_empties=15)
    if n == 0:
        return
    X.assert_answers(got, cases, 1, f"n={n}")


def test_rows_alone_and_in_the_batch():
    cases = X.mixed_exact()[:40]
    together = solve(cases, max_empties=15)
    for i, c in enumerate(cases):
        alone = solve([c], max_empties=15)
        assert all(int(a[0]) == int(t[i]) for a, t in zip(alone, together)), i


_PARTITION = {}


def _partition_list():
    """257 mixed rows, one 15- and one 16-empties fixture row, answered once under tuning 0 (and checked): shared by the cases below."""
    if not _PARTITION:
        deep2 = X.deep2_cases()
        cases = X.mixed_exact(257) + deep2[:1] + deep2[8:9]
        assert [64 - bin(c[0] | c[1]).count("1") for c in cases[-2:]] == [15, 16]
        base = solve(cases, max_empties=16)
        X.assert_answers(base, cases, 1, "tuning 0")
        _PARTITION.update(cases=cases, base=base)
    return _PARTITION["cases"], _PARTITION["base"]


_VARIANTS = list(X.tunings()) + ["minimum workspace", "twice the minimum"]


@pytest.mark.parametrize("name", _VARIANTS)
def test_partition_independence(name):
    """EVERY tuning of tunings(), the minimum workspace and twice it, on the whole list - the deep rows included: a record of
    more than 12 empties is split whatever the tuning says - on a stream of its own: byte-identical to tuning 0."""
    import torch
    from reversi_alpha_zero_amd._native import lib
    cases, base = _partition_list()
    least = lib.raz_solve_exact_workspace_bytes(len(cases), 16)
    tuning = X.tunings().get(name, 0)
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


def test_a_budget_of_three_parks_thousands_of_times():
    """One 15- and one 16-empties fixture row beside 63 mixed rows at 3 node visits per lane and launch."""
    deep2 = X.deep2_cases()
    cases = X.mixed_exact(63) + deep2[:1] + deep2[8:9]
    visits = []
    X.assert_answers(solve(cases, tuning=X.TUNE_BUDGET[3], max_empties=16, visits=visits), cases, 1, "budget 3")
    assert visits[0] > 3000


def test_refusals_leave_the_outputs_alone():
    from reversi_alpha_zero_amd._native import lib
    cases = X.cycled(X.mixed_exact(), 65)
    n = len(cases)
    sizes = [lib.raz_solve_exact_workspace_bytes(n, e) for e in range(X.MAX_EMPTIES + 1)]
    for short in (sizes[15] - 1, sizes[0] - 1):
        assert _untouched(solve(cases, ws_bytes=short, expect=X.RAZ_EINVAL))
    for bad in (1 << 26, 1 << 31, X.TUNE_LEAF(1), X.TUNE_LEAF(19), 6 << 20):
        assert _untouched(solve(cases, tuning=bad, expect=X.RAZ_EINVAL))


def test_pruning_happens():
    """R(12): strictly fewer node visits than raz_solve_batch(exactly = 1) on the same rows."""
    cases = X.random_cases(12)
    mine, theirs = [], []
    a, b = solve(cases, max_empties=12, visits=mine), solve(cases, batch=True, visits=theirs)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert 0 < mine[0] < theirs[0], (mine, theirs)


def test_the_python_class():
    import torch
    from reversi_alpha_zero_amd.lib.reversi_solver import ReversiSolver, EXACT_MAX_EMPTIES
    assert EXACT_MAX_EMPTIES == X.MAX_EMPTIES
    s = ReversiSolver()
    cases = X.status_cases() + X.random_cases(9, 8)
    mv, sc, st = s.solve_exact_batch(*_dev(cases))
    assert mv.is_cuda and mv.dtype == torch.int8 and st.dtype == torch.uint8
    X.assert_answers((mv.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), cases, 1, "solve_exact_batch")
    for b, w, p, status, ans in cases:
        if status == 0:
            assert s.solve_exact(b, w, p) == ans[1]
        elif status == 1:
            assert s.solve_exact(b, w, p) == (None, None)
        elif status == 2:
            with pytest.raises(ValueError, match="17"):
                s.solve_exact(b, w, p)
        elif p in (1, 2):
            with pytest.raises(ValueError, match="not a position"):
                s.solve_exact(b, w, p)
    b15, w15, p15 = X.random_positions(15, 1, 9015)[0]
    with pytest.raises(ValueError, match="14"):
        s.solve(b15, w15, p15, exactly=True)
    with pytest.raises(ValueError):
        s.solve_exact_batch(*(t.cpu() for t in _dev(cases)))


def test_analyze_with_exact_empties():
    """GameAnalyzer.analyze(games, exact_empties=16) on two short mini-net games at 8 sims a move: every added field equals
    solve_exact called per position; without exact_empties the dictionaries are today's."""
    import random
    from test_analysis_gpu import _python_config
    from test_match_gpu import DEV
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.lib.analysis import GameAnalyzer
    from reversi_alpha_zero_amd.lib.reversi_solver import ReversiSolver
    rng, games = random.Random(11), []
    for b, w, p in X.random_positions(17, 2, 9317):   # two games from 17 empties to their ends (random moves, passes as None)
        b0, w0, p0, actions = b, w, p, []
        while True:
            own, enemy = (b, w) if p == 1 else (w, b)
            legal = X.moves_of(own, enemy)
            if not legal:
                if not X.moves_of(enemy, own):
                    break
                actions.append(None)
                p = 3 - p
                continue
            a = rng.choice(X.squares(legal))
            actions.append(a)
            own, enemy = X.play(a, own, enemy)
            b, w = (own, enemy) if p == 1 else (enemy, own)
            p = 3 - p
        games.append((b0, w0, p0, actions))
    cfg = _python_config(1)
    net = ReversiNet(16, 1, 16).keras_init_(1).randomize_bn_(2)
    ga = GameAnalyzer(cfg, net, cfg.play, slots=64, device=DEV)
    plain, exact = ga.analyze(games), ga.analyze(games, exact_empties=16)
    added = {"solved_move", "solved_score", "played_score", "played_loss"}
    solver, seen = ReversiSolver(DEV), {"solved": 0, "played": 0, "lost": 0, "above": 0}
    for gp, ge in zip(plain, exact):
        assert len(gp) == len(ge)
        for i, (dp, de) in enumerate(zip(gp, ge)):
            assert {k: v for k, v in de.items() if k not in added} == dp
            e = 64 - bin(de["black"] | de["white"]).count("1")
            if de["state"] == "over" or e > 16:
                assert not (added & set(de))
                seen["above"] += e > 16
                continue
            mv, sc = solver.solve_exact(de["black"], de["white"], de["player"])
            if mv is None:   # a pass entry whose side to move cannot move: the position after it, from this side's view
                assert de["state"] == "pass_entry" and de["solved_move"] is None
                continue
            assert (de["solved_move"], de["solved_score"]) == (mv, sc)
            seen["solved"] += 1
            if de["played"] is None:
                continue
            own, enemy = (de["black"], de["white"]) if de["player"] == 1 else (de["white"], de["black"])
            no, ne = X.play(de["played"], own, enemy)   # the played move's value: the position after it, solved on its own
            nxt = ge[i + 1]
            if nxt["state"] == "over":
                want = bin(no).count("1") - bin(ne).count("1")
            else:
                other = 3 - de["player"]
                if X.moves_of(ne, no):
                    want = -solver.solve_exact(*((ne, no) if other == 1 else (no, ne)), other)[1]
                else:
                    want = solver.solve_exact(*((no, ne) if de["player"] == 1 else (ne, no)), de["player"])[1]
            assert de["played_score"] == want and de["played_loss"] == sc - want >= 0
            assert (de["played_loss"] == 0) == (want == sc)
            seen["played"] += 1
            seen["lost"] += de["played_loss"] > 0
    assert seen["solved"] >= 20 and seen["played"] >= 20 and seen["lost"] > 0 and seen["above"] > 0, seen
    with pytest.raises(ValueError):
        ga.analyze(games, exact_empties=18)
