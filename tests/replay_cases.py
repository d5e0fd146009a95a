"""Shared by tests/test_replay_rows_emu.py and tests/test_replay_rows_gpu.py: synthetic self-play outboxes for raz_train_rows_count /
raz_train_rows_fill (csrc/raz_replay.hip), two INDEPENDENT expectations of the trainer's packed rows, and the runner that puts a
case in front of a library (the wave emulator's, or the real one on a GPU) and compares every byte.

  (i)  pack_game_data(rows_of_game(...)) with engine.saved_policy: the Python restatement of the reference's row building;
  (ii) pack_game_data(json.loads("[" + game_rows_json(...) + "]")): the native text route (csrc/raz_emit.hip, host code) read back
       the way the `opt` worker reads a file.
Both must agree on the CPU before any kernel is looked at (test_replay_rows_emu.py).  Every comparison is exact: the policy as
uint32 views, everything else with array_equal.  Output buffers start as 0x55 and carry PAD_ROWS rows beyond their end, so an
untouched or overrun byte shows."""
import functools
import json

import numpy as np

RAZ_OK, RAZ_EINVAL, RAZ_EDEVICE = 0, -1, -2
SCAN_BLOCK = 256   # csrc/raz_replay.hip kScanBlock: the games one trip of k_rows_scan's loop takes
PAD_ROWS = 16
FILL = 0x55


def _dtypes():
    from reversi_alpha_zero_amd.engine import GAME_SUMMARY, PLY_HEADER
    assert PLY_HEADER.itemsize == 48 and GAME_SUMMARY.itemsize == 32
    return PLY_HEADER, GAME_SUMMARY


# ---- outboxes -------------------------------------------------------------------------------------------------------------------
def _random_counts(rng, top=3200):
    """Visit counts of a searched ply: a third of the squares visited, never all zero."""
    n = rng.integers(0, top + 1, size=64, dtype=np.uint32) * (rng.random(64) < 0.35)
    n[int(rng.integers(64))] += np.uint32(1 + rng.integers(top))
    return n.astype(np.uint32)


def _fill_game(rng, hdr, rn, plies, kind="mixed"):
    """Every one of the `plies` headers of a game, the ones beyond its n_plies included (a kernel that ignores n_plies then shows):
    asymmetric random boards, players alternating with passes (the same player twice running), has_row on most plies."""
    player = 1
    for j in range(plies):
        own = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(2))
        enemy = (int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(2))) & ~own
        hdr[j]["own"], hdr[j]["enemy"] = own, enemy
        hdr[j]["n"], hdr[j]["q"] = float(rng.integers(1, 100)), float(rng.random())
        hdr[j]["action"] = int(rng.integers(64))
        hdr[j]["player"] = player
        hdr[j]["turn"] = j % 256
        has_row = rng.random() < 0.8
        if kind == "no_rows":
            has_row = False
        elif kind == "white_only":
            has_row = player == 2
        elif kind == "black_only":
            has_row = player == 1
        elif kind == "all_rows":
            has_row = True
        hdr[j]["has_row"] = int(has_row)
        hdr[j]["sims"], hdr[j]["loops"] = 8, 1
        rn[j] = _random_counts(rng)
        if not (kind == "passes" and j % 3 == 1) and not (kind == "mixed" and rng.random() < 0.1):
            player = 3 - player   # (else a pass: the same side moves again)


def _outbox(name, plies, games, seed, change_tau_turn=10, save_policy_of_tau_1=0, done=None):
    """games: [(n_plies as the summary states it, kind, status)]."""
    PH, GS = _dtypes()
    rng = np.random.default_rng(seed)
    G = len(games)
    headers = np.zeros((G, plies), dtype=PH)
    root_n = np.zeros((G, plies, 64), dtype=np.uint32)
    summary = np.zeros(G, dtype=GS)
    for g, (n_plies, kind, status) in enumerate(games):
        _fill_game(rng, headers[g], root_n[g], plies, "mixed" if kind == "resigned" else kind)
        if kind == "resigned" and 0 < n_plies <= plies:
            headers[g, n_plies - 1]["action"] = -1
        summary[g]["n_plies"], summary[g]["status"], summary[g]["game_id"] = n_plies, status, 1000 + g
        summary[g]["final_black"], summary[g]["final_white"] = 0x1234, 0x4321
    return {"name": name, "plies": plies, "headers": headers, "root_n": root_n, "summary": summary,
            "done": None if done is None else np.ascontiguousarray(done, dtype=np.uint8),
            "change_tau_turn": change_tau_turn, "save_policy_of_tau_1": save_policy_of_tau_1}


STATUSES = (1, 2, 3, 0x21, 0x12, 0x23, 0x11)   # winner | flags above the low nibble (raz_env_step)


@functools.lru_cache(maxsize=None)
def ply_axis_case(plies):
    """The 64-wide ply loop takes one, two and three trips: games of n_plies 0, 1, plies - 1, plies, one beyond the array (clamped),
    one without any row, one of passes, one that ends in a resignation, one with only white's rows and one with only black's."""
    games = [(n, "mixed", STATUSES[i % len(STATUSES)]) for i, n in enumerate(sorted({0, 1, max(plies - 1, 0), plies}))]
    games += [(plies + 5, "all_rows", 2), (plies, "no_rows", 1), (plies, "passes", 3), (plies, "resigned", 0x21),
              (plies, "white_only", 1), (plies, "black_only", 2), (max(plies - 1, 1), "white_only", 2)]
    # tau: turns below 10 take the proportional policy, the rest the argmax - both branches wherever plies > 10
    return _outbox(f"plies={plies}", plies, games, seed=100 + plies, change_tau_turn=10, save_policy_of_tau_1=0)


PLY_AXIS = (1, 2, 63, 64, 65, 130)
GAME_AXIS = (1, 255, 256, 257, 1025)
assert max(GAME_AXIS) >= 3 * SCAN_BLOCK   # k_rows_scan's loop repeats, with a carry, more than twice


@functools.lru_cache(maxsize=None)
def game_axis_case(n_games, done_kind):
    """plies = 3.  done_kind: None (no flags), or "holes": zeros as first entry, as last entry and in the middle."""
    rng = np.random.default_rng(7000 + n_games)
    games = [(int(rng.integers(0, 5)), "mixed", STATUSES[int(rng.integers(len(STATUSES)))]) for _ in range(n_games)]
    done = None
    if done_kind == "holes":
        done = np.ones(n_games, dtype=np.uint8)
        done[[0, n_games - 1, n_games // 2]] = 0
        if n_games > 300:
            done[250:262] = 0   # (across the first boundary of the scan's chunks)
    return _outbox(f"games={n_games},done={done_kind}", 3, games, seed=7100 + n_games, change_tau_turn=2, done=done)


def _special(name, rows, change_tau_turn, save_policy_of_tau_1):
    """One game per entry of `rows`: [(turn, counts u32[64])], black and white alternating, every ply with a row."""
    plies = max(len(r) for r in rows)
    case = _outbox(name, plies, [(len(r), "all_rows", STATUSES[i % 3]) for i, r in enumerate(rows)], seed=42,
                   change_tau_turn=change_tau_turn, save_policy_of_tau_1=save_policy_of_tau_1)
    for g, r in enumerate(rows):
        for j, (turn, counts) in enumerate(r):
            case["headers"][g, j]["turn"] = turn
            case["root_n"][g, j] = counts
    return case


def _counts(**squares):
    n = np.zeros(64, dtype=np.uint32)
    for k, v in squares.items():
        n[int(k[1:])] = v
    return n


@functools.lru_cache(maxsize=None)
def counts_case():
    """The proportional policy at its edges: one visited square (p = 1.0 exactly); two squares of 0xC0000000, whose sum passes 2^32,
    alone and beside a square of 3; 2^24 + 1 beside 3, where a division in f32 gives other bits (F32_DIVISION_DIFFERS); random counts."""
    rng = np.random.default_rng(5)
    rows = [[(0, _counts(s17=5))],
            [(1, _counts(s3=0xC0000000, s60=0xC0000000)), (2, _counts(s3=0xC0000000, s60=0xC0000000, s33=3))],
            [(3, _counts(s9=2 ** 24 + 1, s54=3)), (4, _counts(s0=0xFFFFFFFF, s63=0xFFFFFFFF, s31=1))],
            [(5, _random_counts(rng)), (6, _random_counts(rng)), (7, _random_counts(rng))]]
    return _special("counts", rows, change_tau_turn=4, save_policy_of_tau_1=1)


F32_DIVISION_DIFFERS = (2 ** 24 + 1, 3)


@functools.lru_cache(maxsize=None)
def argmax_case(save_policy_of_tau_1):
    """change_tau_turn = 5, save_policy_of_tau_1 = 0: the same counts on both sides of turn == change_tau_turn, a tie at squares 5 and
    40, the maximum at square 63, a value >= 2^31 beside a larger signed one.  save_policy_of_tau_1 = 1 overrides the branch."""
    rng = np.random.default_rng(6)
    tie = _counts(s5=7, s40=7, s12=6, s63=1)
    last = _random_counts(rng, 100)
    last[63] = 5000
    big = _counts(s10=0x7FFFFFFF, s20=0x80000001, s30=0x80000000)
    mixed = _random_counts(rng)
    rows = [[(4, tie), (5, tie), (6, tie)], [(4, last), (5, last)], [(9, big), (2, big)], [(5, mixed), (4, mixed), (200, mixed)]]
    return _special(f"argmax,tau1={save_policy_of_tau_1}", rows, change_tau_turn=5, save_policy_of_tau_1=save_policy_of_tau_1)


@functools.lru_cache(maxsize=None)
def winner_case():
    """Black, white, a draw, statuses with flag bits above the low nibble, and a low nibble that names no winner."""
    statuses = (1, 2, 3, 0x21, 0x12, 0x13, 0x22, 0, 0x10, 4)
    case = _outbox("winner", 6, [(6, "passes", s) for s in statuses], seed=9, change_tau_turn=3)
    return case


def all_cases():
    cases = [ply_axis_case(p) for p in PLY_AXIS]
    cases += [game_axis_case(n, d) for n in GAME_AXIS for d in (None, "holes")]
    cases += [counts_case(), argmax_case(0), argmax_case(1), winner_case()]
    return cases


def case_names():
    """The names of all_cases() without building them (a test's parameters; case_by_name builds one)."""
    return ([f"plies={p}" for p in PLY_AXIS] + [f"games={n},done={d}" for n in GAME_AXIS for d in (None, "holes")]
            + ["counts", "argmax,tau1=0", "argmax,tau1=1", "winner"])


def case_by_name(name):
    if name.startswith("plies="):
        return ply_axis_case(int(name[6:]))
    if name.startswith("games="):
        n, d = name[6:].split(",done=")
        return game_axis_case(int(n), None if d == "None" else d)
    return {"counts": counts_case, "winner": winner_case, "argmax,tau1=0": lambda: argmax_case(0), "argmax,tau1=1": lambda: argmax_case(1)}[name]()


# ---- the two expectations ---------------------------------------------------------------------------------------------------------
def _live_plies(case, g):
    if case["done"] is not None and not case["done"][g]:
        return 0
    return min(int(case["summary"][g]["n_plies"]), case["plies"])


def _concat(parts):
    if not parts:
        return (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 64), np.float32), np.zeros(0, np.int8))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def expected_python(case):
    """(i): rows_of_game over plies whose saved policy is engine.saved_policy's.  Returns (own, enemy, policy, z, row_offset)."""
    from reversi_alpha_zero_amd.engine import saved_policy
    from reversi_alpha_zero_amd.lib.data_helper import pack_game_data
    from reversi_alpha_zero_amd.worker.self_play import rows_of_game
    parts, counts = [], []
    for g in range(len(case["summary"])):
        plies = []
        for j in range(_live_plies(case, g)):
            h = case["headers"][g, j]
            plies.append({"player": int(h["player"]), "own": int(h["own"]), "enemy": int(h["enemy"]), "has_row": bool(h["has_row"]),
                          "saved_policy": saved_policy(case["root_n"][g, j], int(h["turn"]), case["change_tau_turn"],
                                                       case["save_policy_of_tau_1"]) if h["has_row"] else None})
        rows = rows_of_game(plies, int(case["summary"][g]["status"]) & 0x0f)
        counts.append(len(rows))
        if rows:
            parts.append(pack_game_data(rows))
    return _concat(parts) + (np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32),)


def expected_text(case):
    """(ii): the native text of every game, read back the way the `opt` worker reads a file."""
    from reversi_alpha_zero_amd.lib.data_helper import pack_game_data
    from reversi_alpha_zero_amd.worker.self_play import game_rows_json
    parts, counts = [], []
    for g in range(len(case["summary"])):
        text, n_rows = game_rows_json(case["headers"][g], case["root_n"][g], _live_plies(case, g), int(case["summary"][g]["status"]) & 0x0f,
                                      case["change_tau_turn"], case["save_policy_of_tau_1"])
        rows = json.loads("[" + text + "]")
        assert len(rows) == n_rows
        counts.append(n_rows)
        if rows:
            parts.append(pack_game_data(rows))
    return _concat(parts) + (np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32),)


_expected = {}


def expected(case):
    """The expectation the kernels are held to: (ii), computed once per case and never modified (read-only arrays)."""
    if case["name"] not in _expected:
        out = expected_text(case)
        for a in out:
            a.setflags(write=False)
        _expected[case["name"]] = out
    return _expected[case["name"]]


def assert_same_rows(a, b, what):
    for name, x, y in zip(("own", "enemy", "policy", "z", "row_offset"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        if name == "policy":
            x, y = np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:4].tolist())


# ---- the kernels in front of a case ---------------------------------------------------------------------------------------------
class HostMemory:
    """The wave emulator: device memory is host memory."""
    stream = None

    def put(self, a):
        a = np.array(a, copy=True)
        return a, a.ctypes.data

    def get(self, handle):
        return handle


class DeviceMemory:
    """A GPU: torch is the allocator."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device = torch, device

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device)
        return t, t.data_ptr()

    def get(self, handle):
        self.torch.cuda.synchronize()
        return handle.cpu().numpy()


ROW_BYTES = (8, 8, 256, 1)   # own, enemy, policy, z


def run_case(lib, mem, case, capacity=None, host_total=True):
    """count + fill on `lib`.  Returns (row_offset u32[G + 1], total as the call reported it or None, the four output buffers as uint8
    arrays of (expected rows + PAD_ROWS) rows each, filled with 0x55 before the call)."""
    import ctypes
    G, plies = len(case["summary"]), case["plies"]
    total_expected = int(expected(case)[4][-1])
    cap = total_expected if capacity is None else capacity
    hdr = mem.put(case["headers"].view(np.uint8))
    rn = mem.put(case["root_n"])
    sm = mem.put(case["summary"].view(np.uint8))
    done = mem.put(case["done"]) if case["done"] is not None else (None, None)
    off = mem.put(np.full(G + 1 + 4, 0x55555555, dtype=np.uint32))
    total = ctypes.c_uint64(0xDEAD)
    rc = lib.raz_train_rows_count(hdr[1], sm[1], done[1], G, plies, off[1], ctypes.byref(total) if host_total else None, mem.stream)
    assert rc == RAZ_OK, (rc, (lib.raz_last_error() or b"").decode())
    outs = [mem.put(np.full((total_expected + PAD_ROWS) * b, FILL, dtype=np.uint8)) for b in ROW_BYTES]
    rc = lib.raz_train_rows_fill(hdr[1], rn[1], sm[1], done[1], G, plies, case["change_tau_turn"], case["save_policy_of_tau_1"], off[1], cap,
                                 outs[0][1], outs[1][1], outs[2][1], outs[3][1], mem.stream)
    assert rc == RAZ_OK, (rc, (lib.raz_last_error() or b"").decode())
    offsets = np.ascontiguousarray(mem.get(off[0])).view(np.uint32)
    assert (offsets[G + 1:] == 0x55555555).all(), "raz_train_rows_count wrote beyond d_row_offset[n_games]"
    return offsets[:G + 1].copy(), (int(total.value) if host_total else None), [np.ascontiguousarray(mem.get(o[0])).view(np.uint8) for o in outs]


def check_case(lib, mem, case, capacity=None, host_total=True):
    """Every row below the capacity is the expected row, bit for bit; every byte from the capacity on - the PAD_ROWS rows beyond the
    arrays' ends included - is still 0x55; row_offset is numpy's cumsum of the expected row counts."""
    exp = expected(case)
    offsets, total, outs = run_case(lib, mem, case, capacity, host_total)
    assert np.array_equal(offsets, exp[4]), (case["name"], "row_offset", np.argwhere(offsets != exp[4])[:4].tolist())
    if host_total:
        assert total == int(exp[4][-1]), (case["name"], total, int(exp[4][-1]))
    written = int(exp[4][-1]) if capacity is None else min(capacity, int(exp[4][-1]))
    for name, want, got, b in zip(("own", "enemy", "policy", "z"), exp[:4], outs, ROW_BYTES):
        want_bytes = np.ascontiguousarray(want[:written]).view(np.uint8).reshape(-1)
        head, tail = got[:written * b], got[written * b:]
        if not np.array_equal(head, want_bytes):
            bad = np.unique(np.argwhere(head != want_bytes).reshape(-1) // b)
            raise AssertionError((case["name"], name, "rows that differ", bad[:8].tolist(), len(bad)))
        assert (tail == FILL).all(), (case["name"], name, "bytes written at or beyond the capacity: rows",
                                      (written + np.unique(np.argwhere(tail != FILL).reshape(-1) // b))[:8].tolist())
    return written
