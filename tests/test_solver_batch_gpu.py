"""GPU: raz_solve_batch (include/raz.h; csrc/raz_solver_batch.hip) and lib/reversi_solver.py against the yardsticks of
tests/solver_batch_cases.py - the reference's compiled Cython solver (tests/golden/solver_kat.json), the oracle on seeded playout
positions of 1..12 empties, the recorded oracle answers at 13 and 14 empties - and against itself under every partition of the
work.  Every comparison is exact equality of move, score and status."""
import numpy as np
import pytest

import solver_batch_cases as C

pytestmark = pytest.mark.gpu


def _dev(cases):
    import torch
    b, w, p = C.arrays(cases)
    return (torch.from_numpy(b.view(np.int64)).cuda(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(p).cuda())


def solve(cases, exactly, tuning=0, ws_bytes=None, max_empties=14, expect=C.RAZ_OK, stream=None):
    """(move, score, status) as numpy arrays; the outputs start as 0x55 so that an untouched byte shows."""
    import torch
    from reversi_alpha_zero_amd._native import lib, last_error
    n = len(cases)
    b, w, p = _dev(cases) if n else (None, None, None)
    mv = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    sc = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    ws_bytes = lib.raz_solve_batch_workspace_bytes(n, max_empties) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()
    rc = lib.raz_solve_batch(b.data_ptr() if n else None, w.data_ptr() if n else None, p.data_ptr() if n else None, n, int(exactly),
                             mv.data_ptr(), sc.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes, tuning, s.cuda_stream)
    assert rc == expect, (rc, last_error())
    torch.cuda.synchronize()
    return mv.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _untouched(got):
    return all((np.asarray(a).view(np.uint8) == 0x55).all() for a in got)


@pytest.mark.parametrize("exactly", [0, 1])
def test_golden_and_random_positions(exactly):
    """G (3 known answers + 120 positions of the compiled Cython solver) and R(1..12): each list one batch."""
    for name, cases in C.gpu_lists().items():
        C.assert_answers(solve(cases, exactly), cases, exactly, name)


@pytest.mark.parametrize("exactly", [0, 1])
def test_deep_positions_are_split_over_the_chip(exactly):
    """Four positions of 13 and two of 14 empties in one batch: six plies of split, millions of leaf tasks."""
    cases = C.deep_cases()
    C.assert_answers(solve(cases, exactly), cases, exactly, "deep")


def test_status_rows():
    cases = C.status_cases()
    assert sorted({c[3] for c in cases}) == [1, 2, 3]
    for exactly in (0, 1):
        C.assert_answers(solve(cases, exactly), cases, exactly, "status rows")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_batch_edges(n):
    """The mixed list - empties 1..10 interleaved, status rows in between - cycled to n rows: every answer is the one the position
    gets alone (the oracle's), the rows beside refused rows included; n = 0 is RAZ_OK and writes nothing."""
    cases = C.cycled(C.mixed_list(), n)
    for exactly in (0, 1):
        C.assert_answers(solve(cases, exactly), cases, exactly, f"n={n}")


def test_a_row_alone_answers_what_it_answers_in_a_batch():
    cases = C.mixed_list()[:40]
    for exactly in (0, 1):
        whole = solve(cases, exactly)
        for i, c in enumerate(cases):
            one = solve((c,), exactly)
            assert [int(a[0]) for a in one] == [int(a[i]) for a in whole], (i, exactly)


def test_partition_independence():
    """The 257-row mixed list under every tuning there is - no split, every number of split plies at the default and at the
    smallest leaf size, every leaf size, a chunk of one row, the minimum workspace and twice it - and on two streams, twice:
    byte-identical to tuning = 0, which is right."""
    import torch
    cases = C.mixed_list()
    least = __import__("reversi_alpha_zero_amd._native", fromlist=["lib"]).lib.raz_solve_batch_workspace_bytes(len(cases), 10)
    for exactly in (0, 1):
        base = solve(cases, exactly)
        C.assert_answers(base, cases, exactly, "tuning 0")
        variants = [(C.TUNE_SPLIT(p), None) for p in range(0, 7)] + [(C.TUNE_SPLIT(p) | C.TUNE_LEAF(2), None) for p in range(1, 7)]
        variants += [(C.TUNE_LEAF(k), None) for k in range(2, 9)]
        variants += [(C.TUNE_CHUNK(1), None), (C.TUNE_CHUNK(7) | C.TUNE_LEAF(3), None), (0, least), (0, 2 * least)]
        for tuning, ws_bytes in variants:
            got = solve(cases, exactly, tuning=tuning, ws_bytes=ws_bytes)
            for a, b in zip(got, base):
                assert a.tobytes() == b.tobytes(), (hex(tuning), ws_bytes, exactly)
        for _ in range(2):
            for s in (torch.cuda.Stream(), torch.cuda.Stream()):
                got = solve(cases, exactly, stream=s)
                for a, b in zip(got, base):
                    assert a.tobytes() == b.tobytes(), ("stream", exactly)


def test_workspace_and_tuning_edges():
    from reversi_alpha_zero_amd._native import lib
    cases = C.mixed_list()
    n = len(cases)
    assert lib.raz_solve_batch_workspace_bytes(n, 15) == 0 and lib.raz_solve_batch_workspace_bytes(n, 14) > 0
    sizes = [lib.raz_solve_batch_workspace_bytes(n, e) for e in range(0, 15)]
    assert sizes == sorted(sizes)
    least = sizes[10]   # (the list's deepest row has 10 empties)
    C.assert_answers(solve(cases, 1, ws_bytes=least), cases, 1, "minimum workspace")
    for short in (least - 1, sizes[0] - 1):
        assert _untouched(solve(cases, 1, ws_bytes=short, expect=C.RAZ_EINVAL)), "an output byte was written"
    for bad in (1 << 24, 1 << 31, C.TUNE_LEAF(1), C.TUNE_LEAF(9), C.TUNE_SPLIT(7)):
        assert _untouched(solve(cases, 1, tuning=bad, expect=C.RAZ_EINVAL))


def test_reversi_solver_class():
    """lib/reversi_solver.py: the reference's three known answers (lib/reversi_solver.py:102-156), (None, None), the refusals,
    Player arguments, and solve_batch == solve row by row."""
    import torch
    from reversi_alpha_zero_amd.env.reversi_env import Player
    from reversi_alpha_zero_amd.lib.reversi_solver import ReversiSolver
    q = C.golden_cases()[:3]
    solver = ReversiSolver()
    assert solver.solve(q[0][0], q[0][1], Player.white, exactly=False) == (57, 2)
    assert solver.solve(q[1][0], q[1][1], Player.black, exactly=False) == (4, -2)
    assert solver.solve(q[2][0], q[2][1], 2, timeout=0, exactly=True) == (3, 2)
    assert [c[2] for c in q] == [2, 1, 2]
    st = C.status_cases()
    assert st[0][3] == 1 and solver.solve(st[0][0], st[0][1], st[0][2]) == (None, None)
    fifteen = [c for c in st if c[3] == 2][0]
    with pytest.raises(ValueError, match="14"):
        solver.solve(fifteen[0], fifteen[1], fifteen[2], exactly=True)
    both = [c for c in st if c[3] == 3][0]
    with pytest.raises(ValueError, match="both colours"):
        solver.solve(both[0], both[1], both[2])
    with pytest.raises(ValueError, match="next_player"):
        solver.solve(q[0][0], q[0][1], 0)
    cases = C.mixed_list()[:24]
    b, w, p = _dev(cases)
    with pytest.raises(ValueError, match="device-only"):
        solver.solve_batch(b.cpu(), w.cpu(), p.cpu())
    for exactly in (False, True):
        mv, sc, stt = (t.cpu().numpy() for t in solver.solve_batch(b, w, p, exactly=exactly))
        C.assert_answers((mv, sc, stt), cases, exactly, "solve_batch")
        for i, c in enumerate(cases):
            if c[3] == 0:
                assert solver.solve(c[0], c[1], c[2], exactly=exactly) == (int(mv[i]), int(sc[i])), i
            elif c[3] == 1:
                assert solver.solve(c[0], c[1], c[2], exactly=exactly) == (None, None)
    assert torch.cuda.is_available()
