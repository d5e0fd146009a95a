"""Scenarios, numpy references and assertions for the engine's BOOKKEEPING kernels - the ones that start, count, prune, pack and
harvest games (csrc/raz_engine.hip: k_start, k_next_game, k_stats, k_gc, k_set_positions, k_records_extent, k_pack_records,
k_harvest_plan, k_harvest_apply) and for the capacity guards of csrc/raz_engine_core.h (pool_take, flag_error) - at the edges of
their launch shapes, which are multiples of the slot count B: k_harvest_plan scans B in chunks of 1024 with a carried base, k_stats
and k_records_extent reduce over 256 threads, k_gc scans a node directory 256 nodes per round.  Shared by
tests/test_engine_slots_gpu.py (SelfPlayEngine, on the GPU) and tests/test_engine_slots_emu.py (emu_util.EmuEngine, the wave
emulator); the functions below take an engine object, or a `make(n_games, **engine arguments)` factory, and nothing else that
differs between the two.  Every comparison is exact: integers and bit patterns, no tolerance.

What a check needs beyond the records - phase, node_count, pool_used, error, sims ... of every slot - comes from the control blocks
(raz_engine_debug_read(which = 3), 256 bytes per slot) read through a numpy dtype whose offsets tests/native/game_layout.cpp prints
from csrc/raz_engine.h itself.

References: the contract of include/raz.h restated in numpy (harvest, statistics, record packing); the same game in an engine with
room to spare (capacity guards); the same engine state without the call (pruning).  The lock-step path these are compared with does
not touch the harvest kernels and is pinned against the oracle game by game by the engine tests.

Error flags 2 (table full) and 8 (path overflow) cannot be reached through the ABI - raz_engine_create enforces table_slots >= 2 x
nodes_per_game, so the pool's node count binds first, and a path holds at most 60 moves - and have no test here."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 29
INIT_BLACK, INIT_WHITE = 0x0000000810000000, 0x0000001008000000
RAZ_EINVAL = -1


def sims_of(ids):
    """Simulations per move of game id i: 1 + i % 3, so that the games of a batch end at different steps."""
    return (1 + np.asarray(ids, dtype=np.int64) % 3).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- control blocks
@functools.lru_cache(maxsize=None)
def game_layout():
    """(numpy dtype of raz_game with the fields the checks read, {phase name: value}), from tests/native/game_layout.cpp."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "game_layout")
        r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "game_layout.cpp")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    names, formats, offsets, size, phases = [], [], [], None, None
    for line in out:
        w = line.split()
        if not w:
            continue
        if w[0] == "sizeof":
            size = int(w[1])
        elif w[0] == "phases":
            phases = dict(zip(("NEW_MOVE", "SEARCH", "DONE", "IDLE"), map(int, w[1:])))
        else:
            names.append(w[0])
            offsets.append(int(w[1]))
            formats.append((f"<u{int(w[2])}", (int(w[3]),)) if int(w[3]) > 1 else f"<u{int(w[2])}")
    assert size == 256 and phases is not None
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": size}), phases


def phase(name):
    return game_layout()[1][name]


# ---------------------------------------------------------------------------------------------------------------- the two engines
def _lib(e):
    return e.backend.lib   # (SelfPlayEngine on the device, EmuEngine - the same class - on the emulator's backend)


def _stream(e):
    return e.backend.stream()


def dev_from(e, a):
    """A host array as engine-side memory (u64 bit patterns travel as int64)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(e.device)


def host(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.asarray(x)   # (a copy on the emulator too, where .cpu() is the tensor itself)


def ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def clone(x):
    return x.clone() if hasattr(x, "clone") else x.copy()


def rows(x, idx):
    """Rows `idx` (host integer array) of an engine-side array, on the host."""
    idx = np.asarray(idx, dtype=np.int64)
    if hasattr(x, "cpu"):
        import torch
        return x[torch.from_numpy(idx).to(x.device)].cpu().numpy()
    return x[idx]


def same_rows(a, b, mask):
    """a[mask] == b[mask] everywhere (mask: host bool array over the rows)."""
    if hasattr(a, "cpu"):
        import torch
        m = torch.from_numpy(mask).to(a.device)
        return bool(torch.equal(a[m], b[m]))
    return bool(np.array_equal(a[mask], b[mask]))


def snapshot(e):
    """The engine's whole device state (its workspace): restore() puts an engine back where it was, which is what creating it and
    playing to the same point again would give - every result is a function of (seed, game id, parameters)."""
    return clone(e._ws)


def restore(e, snap):
    e.backend.synchronize(e.device)
    e._ws.copy_(snap)
    e.backend.synchronize(e.device)


def _ok(e, rc, what):
    assert rc == 0, (what, rc, (_lib(e).raz_last_error() or b"").decode())


def control_blocks(e):
    """The control block of every slot: (structured view, the raw bytes [B, 256])."""
    dt, _ = game_layout()
    buf = np.zeros((e.n_games, dt.itemsize), dtype=np.uint8)
    _ok(e, _lib(e).raz_engine_debug_read(e._h, 3, 0, buf.size, buf.ctypes.data), "raz_engine_debug_read")
    return buf.view(dt).reshape(e.n_games), buf


def raw_stats(e):
    """raz_engine_stats_sync as a dict (engine.stats() raises on a flag; this does not)."""
    from reversi_alpha_zero_amd import _native as N
    st = N.RazEngineStats()
    _ok(e, _lib(e).raz_engine_stats_sync(e._h, ctypes.byref(st), _stream(e)), "raz_engine_stats_sync")
    return {k: int(getattr(st, k)) for k in ("finished_games", "total_sims", "nn_leaves", "error_flags", "selections", "max_pool_used",
                                             "idle_or_done", "max_pool_bytes")}


def records_extent(e, first, n):
    out = ctypes.c_uint32(0xdeadbeef)
    rc = _lib(e).raz_engine_records_extent(e._h, first, n, ctypes.byref(out), _stream(e))
    return rc, out.value


def pack_records(e, first, n, plies):
    """(rc, headers [n, plies, 48] u8, root_n [n, plies, 64] u32, summary [n, 32] u8) on the host; the arrays are handed over
    filled with 0xa5 so that a byte the kernel does not write shows."""
    from reversi_alpha_zero_amd.engine import PLY_HEADER, GAME_SUMMARY
    shape_p = max(1, min(plies, 4096))
    hdr, rn, sm = (dev_from(e, np.full(s, 0xa5, dtype=np.uint8)) for s in ((max(n, 1), shape_p, 48), (max(n, 1), shape_p, 256), (max(n, 1), 32)))
    rc = _lib(e).raz_engine_pack_records(e._h, first, n, plies, ptr(hdr), ptr(rn), ptr(sm), _stream(e))
    if rc == 0:
        control_blocks(e)   # (synchronises)
    return rc, host(hdr).view(PLY_HEADER)[..., 0], host(rn).view(np.uint32), host(sm).view(GAME_SUMMARY)[..., 0]


def set_positions(e, first_slot, black, white, player, sims, one_move=False):
    b, w, p = (dev_from(e, np.asarray(black, dtype=np.uint64)), dev_from(e, np.asarray(white, dtype=np.uint64)),
               dev_from(e, np.asarray(player, dtype=np.uint8)))
    e.set_positions(first_slot, b, w, p, sims, enable_resign=True, one_move=one_move)
    control_blocks(e)   # (synchronises: the arrays above may go)


# ---------------------------------------------------------------------------------------------------------------- playing
def step_until(e, done, chunk=8, max_steps=4000):
    steps = 0
    while not done():
        assert steps < max_steps, "the engine did not get there"
        e.step(chunk)
        steps += chunk
    return steps


def play_to_end(e, first, endings=None, chunk=8):
    """Every slot plays game id first + slot to its end in lock step (no pruning, no harvest).  endings = (black, white, player)
    arrays: instead of whole games, slot g is put on position g % len two plies before a game's end (the wave emulator's way to a
    finished batch of a thousand slots)."""
    B = e.n_games
    begin(e, first, endings)
    step_until(e, lambda: raw_stats(e)["finished_games"] >= B, chunk)
    G, _ = control_blocks(e)
    assert ((G["phase"] == phase("DONE")) & (G["status"] != 0)).all()


def begin(e, first, endings=None):
    B = e.n_games
    ids = first + np.arange(B)
    if endings is None:
        e.start(first, sims_of(ids))
    else:
        e.start(first, sims_of(ids), n_active=0)
        k = np.arange(B) % len(endings[0])
        set_positions(e, 0, endings[0][k], endings[1][k], endings[2][k], sims=1, one_move=False)


def endings_of(e, first, back=2):
    """The position `back` plies before the end of every game of a finished lock-step batch."""
    raw = e.read_raw()
    n = raw["n_plies"].astype(np.int64)
    assert (n >= back).all()
    h = raw["headers"][np.arange(e.n_games), n - back]
    black = np.where(h["player"] == 1, h["own"], h["enemy"]).astype(np.uint64)
    white = np.where(h["player"] == 1, h["enemy"], h["own"]).astype(np.uint64)
    return black, white, h["player"].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- 1. harvest
def summary_fields(raw, sims):
    """(name in the packed game summary, the value per slot from read_raw() / the control blocks' sims) of every summary field."""
    return (("final_black", raw["final_black"]), ("final_white", raw["final_white"]), ("game_id", raw["game_id"]), ("n_plies", raw["n_plies"]),
            ("status", raw["status"]), ("resigned_black", raw["resigned"][:, 0]), ("resigned_white", raw["resigned"][:, 1]),
            ("enable_resign", raw["enable_resign"]), ("sims", (sims & 0xffffffff).astype(np.uint32)))


def harvest_reference(G, n_new, out_first, out_games):
    """include/raz.h raz_engine_harvest in numpy: (plan per slot, rank per slot, (harvested, restarted, skipped, playing))."""
    DONE, IDLE = phase("DONE"), phase("IDLE")
    finished = (G["phase"] == DONE) & (G["status"] != 0)
    in_window = (G["game_id"].astype(np.uint32) - np.uint32(out_first)).astype(np.uint32) < np.uint32(out_games)
    fin = finished & in_window
    rank = np.cumsum(fin) - fin
    plan = np.where(fin, np.where(rank < n_new, 2, 1), 0)
    harvested = int(fin.sum())
    restarted = min(harvested, int(n_new))
    in_progress = int(((G["phase"] != DONE) & (G["phase"] != IDLE)).sum())
    return plan, rank, (harvested, restarted, int((finished & ~in_window).sum()), in_progress + restarted)


def window_of(outbox, first, n):
    """The rows of ids [first, first + n) of an outbox as an outbox of its own (views: the call writes into the whole one)."""
    lo = first - outbox["first"]
    assert 0 <= lo and lo + n <= outbox["n"] and n > 0
    return dict({k: outbox[k][lo:lo + n] for k in ("headers", "root_n", "summary", "done")}, first=first, n=n)


def check_harvest(e, outbox, next_id, new_sims, window=None):
    """One raz_engine_harvest call against harvest_reference, computed from the control blocks and read_raw() taken right before
    it.  window = (first id, n ids): the call is given only those rows of `outbox`.  Returns the four result words."""
    from reversi_alpha_zero_amd.engine import GAME_SUMMARY
    new_sims = np.asarray(new_sims, dtype=np.uint32)
    G0, B0 = control_blocks(e)
    raw0 = e.read_raw()
    before = {k: clone(outbox[k]) for k in ("headers", "root_n", "summary", "done")}
    out_first, out_games = window if window is not None else (outbox["first"], outbox["n"])
    plan, rank, words = harvest_reference(G0, new_sims.size, out_first, out_games)
    got = e.harvest(window_of(outbox, out_first, out_games), next_id, new_sims)
    assert tuple(int(x) for x in got) == words, (got, words)
    G1, B1 = control_blocks(e)
    MP = e.max_plies
    # the outbox: harvested rows hold the slot's records, every other byte is what it was
    slots = np.nonzero(plan)[0]
    out_rows = (G0["game_id"][slots].astype(np.int64) - outbox["first"])
    assert len(set(out_rows.tolist())) == len(out_rows) and ((out_rows >= 0) & (out_rows < outbox["n"])).all()
    if len(slots):
        n = raw0["n_plies"][slots].astype(np.int64)
        live = np.arange(MP)[None, :] < n[:, None]
        hdr = raw0["headers"][slots].copy()
        hdr[~live] = np.zeros((), dtype=hdr.dtype)
        assert np.array_equal(rows(outbox["headers"], out_rows).reshape(len(slots), -1), hdr.view(np.uint8).reshape(len(slots), -1))
        rn = raw0["root_n"][slots] * live[:, :, None].astype(np.uint32)
        assert np.array_equal(rows(outbox["root_n"], out_rows).view(np.uint32), rn)
        sm = np.ascontiguousarray(rows(outbox["summary"], out_rows)).view(GAME_SUMMARY)[:, 0]
        for k, v in summary_fields(raw0, G0["sims"]):
            assert np.array_equal(sm[k], v[slots]), k
        assert (rows(outbox["done"], out_rows) == 1).all()
    untouched = np.ones(outbox["n"], dtype=bool)
    untouched[out_rows] = False
    for k in before:
        assert same_rows(outbox[k], before[k], untouched), k
    # the slots
    p2, p1, p0 = plan == 2, plan == 1, plan == 0
    assert np.array_equal(G1["game_id"][p2], (next_id + rank[p2]).astype(np.uint32))
    assert np.array_equal(G1["sims_per_move"][p2], new_sims[rank[p2]])
    for k, v in (("n_plies", 0), ("status", 0), ("phase", phase("NEW_MOVE")), ("pool_used", 1), ("node_count", 0), ("sims", 0),
                 ("root_black", INIT_BLACK), ("root_white", INIT_WHITE), ("player", 1)):
        assert (G1[k][p2] == v).all(), k
    assert np.array_equal(G1["error"][p2 | p1], G0["error"][p2 | p1])
    assert (G1["phase"][p1] == phase("IDLE")).all() and np.array_equal(G1["game_id"][p1], G0["game_id"][p1])
    assert np.array_equal(B1[p0], B0[p0])
    return words


def harvest_all_at_once(e, first, n_new):
    """1(a), 1(b): every game of the batch has finished; one call with n_new new ids."""
    B = e.n_games
    outbox = e.new_outbox(first, B + 1)
    nxt = first + B
    words = check_harvest(e, outbox, nxt, sims_of(nxt + np.arange(n_new)))
    assert words == (B, min(B, n_new), 0, min(B, n_new))
    done = host(outbox["done"])
    assert done[:B].all() and not done[B]
    G, _ = control_blocks(e)
    assert np.array_equal(G["game_id"][:n_new], (nxt + np.arange(min(B, n_new))).astype(np.uint32))
    return outbox


def harvest_windows(e, first):
    """1(c): windows that leave out the ids of slots {0, 1023, 1024, B - 1} (a window is one id range, so the slots between them
    are taken by one call each); the games left out are counted as skipped and stay; a window over everything then takes them."""
    B = e.n_games
    outbox = e.new_outbox(first, B + 1)   # (row B: an id nobody plays - the window of a call that must take nothing)
    left_out = sorted({0, B - 1} | ({1023} if B > 1023 else set()) | ({1024} if B > 1024 else set()))
    cuts = [-1] + left_out + [B]
    ranges = [(a + 1, b - a - 1) for a, b in zip(cuts[:-1], cuts[1:]) if b - a - 1 > 0 and a + 1 < B]
    nxt, taken = first + B, 0
    for lo, n in ranges or [(B, 1)]:
        words = check_harvest(e, outbox, nxt, sims_of(nxt + np.arange(2)), window=(first + lo, n))
        n = n if ranges else 0
        assert words[0] == n and words[2] == B - taken - n, words
        nxt, taken = nxt + words[1], taken + n
    G, _ = control_blocks(e)
    assert np.array_equal(G["game_id"][left_out], (first + np.array(left_out)).astype(np.uint32))
    assert ((G["phase"][left_out] == phase("DONE")) & (G["status"][left_out] != 0)).all()
    assert not host(outbox["done"])[left_out].any()
    words = check_harvest(e, outbox, nxt, sims_of(nxt + np.arange(0)))
    assert words[0] == len(left_out) and words[2] == 0
    assert host(outbox["done"])[:B].all()


def harvest_nothing_finished(e, first):
    """1(d): right after start nothing has finished: playing = B, the rest 0, nothing changes."""
    B = e.n_games
    e.start(first, sims_of(first + np.arange(B)))
    outbox = e.new_outbox(first, B + 1)
    _, blocks = control_blocks(e)
    words = check_harvest(e, outbox, first + B, sims_of(first + B + np.arange(B)))
    assert words == (0, 0, 0, B)
    assert np.array_equal(control_blocks(e)[1], blocks)
    assert not any(host(outbox[k]).any() for k in ("headers", "root_n", "summary", "done"))


def continuous_run(e, first, total, chunk=8):
    """1(e): ids first .. first + total - 1 through the engine's slots with continuous batching, the reference applied at every
    harvest call; 3: the statistics' totals include the harvested games.  Returns the outbox (host arrays)."""
    B = e.n_games
    e.start(first, sims_of(first + np.arange(B)))
    outbox = e.new_outbox(first, total)
    nxt, done, end, steps = first + B, 0, first + total, 0
    while done < total:
        assert steps < 20000
        e.step(chunk)
        steps += chunk
        k = min(B, end - nxt)
        words = check_harvest(e, outbox, nxt, sims_of(nxt + np.arange(k)))
        assert words[2] == 0
        nxt, done = nxt + words[1], done + words[0]
        if words[0]:
            check_stats(e, outbox)
    assert nxt == end and host(outbox["done"]).all()
    return {k: host(outbox[k]) for k in ("headers", "root_n", "summary", "done")}


def lock_step_outbox(make, first, total, batch):
    """The records of the same ids played as lock-step batches of `batch` slots and read with read_raw(), in the outbox's shape."""
    assert total % batch == 0
    e = make(batch)
    parts = []
    for lo in range(first, first + total, batch):
        play_to_end(e, lo)
        raw = e.read_raw()
        live = np.arange(e.max_plies)[None, :] < raw["n_plies"][:, None]
        hdr = raw["headers"].copy()
        hdr[~live] = np.zeros((), dtype=hdr.dtype)
        G, _ = control_blocks(e)
        parts.append((hdr, raw["root_n"] * live[:, :, None].astype(np.uint32), raw, G["sims"]))
    return parts


def check_outbox_equals_lock_step(out, parts):
    from reversi_alpha_zero_amd.engine import GAME_SUMMARY
    r = 0
    sm = np.ascontiguousarray(out["summary"]).view(GAME_SUMMARY)[:, 0]
    for hdr, rn, raw, sims in parts:
        n = len(hdr)
        assert np.array_equal(out["headers"][r:r + n].reshape(n, -1), hdr.view(np.uint8).reshape(n, -1))
        assert np.array_equal(out["root_n"][r:r + n].view(np.uint32), rn)
        for k, v in summary_fields(raw, sims):
            assert np.array_equal(sm[k][r:r + n], v), k
        r += n
    assert r == len(sm)


def check_outbox_rows_equal_oracle(out, first, ids, cfg, blob):
    """Outbox rows == the oracle's games of those ids (actions, root N, result)."""
    import oracle as O
    from reversi_alpha_zero_amd.engine import raw_from_packed
    raw = raw_from_packed(out["headers"], out["root_n"], out["summary"])
    ocfg = O.play_cfg_from_config(cfg)
    for gid in ids:
        plies, summ = O.selfplay_game(ocfg, blob, SEED, int(gid), int(sims_of(gid)))
        r = gid - first
        n = int(raw["n_plies"][r])
        assert int(raw["game_id"][r]) == gid and n == len(plies), (gid, n, len(plies))
        assert [int(a) for a in raw["headers"][r, :n]["action"]] == [p["action"] for p in plies], gid
        for i, p in enumerate(plies):
            assert [float(x) for x in raw["root_n"][r, i]] == p["root_n"], (gid, i)
        assert int(raw["status"][r]) & 0x0f == summ["winner"] and (int(raw["final_black"][r]), int(raw["final_white"][r])) == (summ["black"], summ["white"])


# ---------------------------------------------------------------------------------------------------------------- 2. record packing
def extent_ranges(B):
    return [(f, n) for f, n in ((0, B), (0, 255), (0, 256), (1, 256), (256, B - 256), (B - 1, 1)) if n > 0 and f + n <= B]


def check_records_extent(e):
    """raz_engine_records_extent over the issue's ranges, plus the range that ends on the batch's longest game: a reduction that
    misses its last element shows.  (In a batch at 1 + id % 3 simulations per move every run of 256 slots holds a game of the
    greatest length: the strides past the first are check_records_extent_far's.)"""
    B = e.n_games
    n_plies = e.read_raw()["n_plies"]
    for f, n in extent_ranges(B) + [(0, int(np.argmax(n_plies)) + 1)]:
        rc, got = records_extent(e, f, n)
        assert rc == 0 and got == int(n_plies[f:f + n].max()), (f, n, got, int(n_plies[f:f + n].max()))
    assert records_extent(e, 0, 0) == (0, 0)
    assert records_extent(e, 0, B + 1)[0] == RAZ_EINVAL and records_extent(e, B, 1)[0] == RAZ_EINVAL


def far_batch(e, first, K):
    """A finished batch whose longest games lie ONLY in slots K and B - 1: those two play at 3 simulations per move, every other
    slot at 1 - such a game is 2 plies long (nothing is visited, so it moves to square 0, which flips nothing, twice)."""
    B = e.n_games
    sims = np.ones(B, dtype=np.uint32)
    sims[[K, B - 1]] = 3
    e.start(first, sims)
    step_until(e, lambda: raw_stats(e)["finished_games"] >= B, chunk=8)


def check_records_extent_far(e, K):
    """raz_engine_records_extent on far_batch(K), K >= 256: the greatest length of a range is found only in the second or a later
    stride of the 256-thread loop - at index 256 of the range, in its last slot, in the third and the fourth stride where B allows
    - so a reduction that is right for the first 256 slots alone shows."""
    B = e.n_games
    n_plies = e.read_raw()["n_plies"].astype(np.int64)
    short = int(n_plies[:K].max())
    assert K >= 256 and short < n_plies[K] and short < n_plies[B - 1] and (B - 1 == K or int(n_plies[K + 1:B - 1].max(initial=0)) <= short), n_plies
    far = [(0, B), (0, K + 1), (K - 256, 257), (K - 255, 256 + min(255, B - 1 - K))]    # the longest game at index >= K, K (last), 256, 255 (first stride, last thread)
    if B - 1 > K:
        far += [(0, B - 1), (K + 1, B - K - 1)]                                         # ... only slot K; only slot B - 1, the last of the range
    if K >= 512:
        far += [(256, B - 1 - 256), (K - 512, 513)]                                     # ... only at index K - 256 / 512 of the range: the third stride
    strides = set()
    for f, n in far:
        want = int(n_plies[f:f + n].max())
        where = np.nonzero(n_plies[f:f + n] == want)[0]
        assert want > short and f + n <= B
        strides |= {int(i) // 256 for i in where} if where.min() >= 255 else set()
        rc, got = records_extent(e, f, n)
        assert rc == 0 and got == want, (f, n, got, want)
    assert strides >= {1} | ({2, 3} if K >= 768 else set()), strides
    for f, n in ((0, K), (0, 256), (K + 1, B - 2 - K)):
        if n > 0:
            assert records_extent(e, f, n) == (0, int(n_plies[f:f + n].max())) and int(n_plies[f:f + n].max()) <= short, (f, n)


def check_pack_records(e):
    """raz_engine_pack_records == read_raw() field by field for plies in {1, the range's shortest game, its longest, max_plies}: a cut
    game keeps its true n_plies in the summary, rows past min(n_plies, plies) are zero; the argument checks."""
    B, MP = e.n_games, e.max_plies
    raw = e.read_raw()
    G, _ = control_blocks(e)
    for f, n in extent_ranges(B):
        np_ = raw["n_plies"][f:f + n].astype(np.int64)
        for plies in sorted({1, int(np_.min()), int(np_.max()), MP}):
            rc, hdr, rn, sm = pack_records(e, f, n, plies)
            assert rc == 0
            live = np.arange(plies)[None, :] < np_[:, None]
            want = raw["headers"][f:f + n, :plies].copy()
            want[~live] = np.zeros((), dtype=want.dtype)
            assert np.array_equal(hdr.view(np.uint8).reshape(n, -1), np.ascontiguousarray(want).view(np.uint8).reshape(n, -1)), (f, n, plies)
            assert np.array_equal(rn, raw["root_n"][f:f + n, :plies] * live[:, :, None].astype(np.uint32)), (f, n, plies)
            for k, v in summary_fields(raw, G["sims"]):
                assert np.array_equal(sm[k], v[f:f + n]), (k, f, n, plies)
    rc, hdr, rn, sm = pack_records(e, 0, 0, 1)
    assert rc == 0 and (hdr.view(np.uint8) == 0xa5).all() and (sm.view(np.uint8) == 0xa5).all()   # n_slots = 0: OK, nothing written
    assert pack_records(e, 0, 1, 0)[0] == RAZ_EINVAL
    assert pack_records(e, 0, 1, MP + 1)[0] == RAZ_EINVAL
    assert pack_records(e, B - 1, 2, 1)[0] == RAZ_EINVAL and pack_records(e, B, 1, 1)[0] == RAZ_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 3. statistics
def check_stats(e, outbox=None):
    """Every field of raz_engine_stats == the numpy reduction of the control blocks (max_pool_* over the games in progress only).
    With an outbox: the run harvests - finished_games and total_sims include the games that left their slots (their leaves and
    selections are not in the outbox: those two fields are not compared then)."""
    from reversi_alpha_zero_amd.engine import GAME_SUMMARY
    st = raw_stats(e)
    G, _ = control_blocks(e)
    running = G["status"] == 0
    want = {"finished_games": int((G["status"] != 0).sum()), "total_sims": int(G["sims"].sum()), "nn_leaves": int(G["leaves"].sum()),
            "selections": int(G["selections"].sum()), "error_flags": int(np.bitwise_or.reduce(G["error"])),
            "max_pool_used": int(G["node_count"][running].max()) if running.any() else 0,
            "max_pool_bytes": 8 * int(G["pool_used"][running].max()) if running.any() else 0,
            "idle_or_done": int(((G["phase"] == phase("IDLE")) | (G["phase"] == phase("DONE"))).sum())}
    if outbox is not None:
        done = host(outbox["done"]).astype(bool)
        sm = np.ascontiguousarray(host(outbox["summary"])).view(GAME_SUMMARY)[:, 0]
        want["finished_games"] += int(done.sum())
        want["total_sims"] += int(sm["sims"][done].astype(np.int64).sum())
        del want["nn_leaves"], want["selections"]
    assert {k: st[k] for k in want} == want
    return st


# ---------------------------------------------------------------------------------------------------------------- 4. capacity guards
def _same_game(raw_a, a, raw_b, b):
    """Slot a of raw_a and slot b of raw_b hold the same game, bit for bit."""
    n = int(raw_a["n_plies"][a])
    assert n == int(raw_b["n_plies"][b]) and n > 0
    assert raw_a["headers"][a, :n].tobytes() == raw_b["headers"][b, :n].tobytes()
    assert np.array_equal(raw_a["root_n"][a, :n], raw_b["root_n"][b, :n])
    assert raw_a["root_w"][a, :n].tobytes() == raw_b["root_w"][b, :n].tobytes()
    for k in ("status", "game_id", "enable_resign", "final_black", "final_white"):
        assert raw_a[k][a] == raw_b[k][b], k
    assert np.array_equal(raw_a["resigned"][a], raw_b["resigned"][b])


def _record_positions(raw, slot):
    """(black, white, player to move) of every recorded ply of a slot."""
    out = []
    for h in raw["headers"][slot, :int(raw["n_plies"][slot])]:
        own, enemy, p = int(h["own"]), int(h["enemy"]), int(h["player"])
        out.append((own, enemy, p) if p == 1 else (enemy, own, p))
    return out


def _node_bits(e, slot, black, white, player, owner):
    found, w, n, p = e.read_node(slot, black, white, next_player=player, owner=owner)
    return found, w.tobytes(), n.tobytes(), p.tobytes()


def pool_full(make, first, roomy, **tight):
    """Two slots, slot 0 at 20 simulations per move in a pool it overruns, slot 1 at 1: flag 1; slot 0 stands still from then on,
    within its pool; slot 1's game and the tree behind it - the memory right after slot 0's pool - are those of the same id in an
    engine with room (`roomy`: that engine, played to the end).  Returns the tight engine."""
    e = make(2, **tight)
    sims = np.array([20, 1], dtype=np.uint32)
    e.start(first, sims)
    step_until(e, lambda: raw_stats(e)["error_flags"] != 0, chunk=4, max_steps=400)
    assert raw_stats(e)["error_flags"] == 1
    G0, _ = control_blocks(e)
    assert G0["error"][0] == 1 and G0["error"][1] == 0
    e.step(200)
    step_until(e, lambda: control_blocks(e)[0]["status"][1] != 0, chunk=8)
    G1, _ = control_blocks(e)
    for k in ("sims", "n_plies", "node_count", "pool_used", "status"):
        assert G1[k][0] == G0[k][0], k
    assert G1["status"][0] == 0 and G1["node_count"][0] <= e.cfg.nodes_per_game and 8 * int(G1["pool_used"][0]) <= e.pool_bytes
    assert raw_stats(e)["error_flags"] == 1 and G1["error"][1] == 0
    raw, raw_r = e.read_raw(), roomy.read_raw()
    _same_game(raw, 1, raw_r, 1)
    for b, w, p in _record_positions(raw, 1):
        for owner in (0, 1):
            assert _node_bits(e, 1, b, w, p, owner) == _node_bits(roomy, 1, b, w, p, owner), (hex(b), hex(w), p, owner)
    return e


def roomy_pair(make, first):
    e = make(2, nodes_per_game=512)
    e.start(first, np.array([20, 1], dtype=np.uint32))
    step_until(e, lambda: control_blocks(e)[0]["status"][1] != 0, chunk=8)
    assert raw_stats(e)["error_flags"] == 0
    return e


def _one_game(make, first, sims, **kw):
    e = make(1, **kw)
    e.start(first, np.array([sims], dtype=np.uint32))
    step_until(e, lambda: (lambda s: s["finished_games"] >= 1 or s["error_flags"] != 0)(raw_stats(e)), chunk=8, max_steps=8000)
    return e, raw_stats(e)["error_flags"]


def exact_fit(make, first, sims=6):
    """A game that needs C0 nodes and U0 pool units fits nodes_per_game = C0 / pool_bytes_per_game = 8 U0 exactly (same game, no
    flag) and does not fit one node / one unit less (flag 1)."""
    roomy, flag = _one_game(make, first, sims, nodes_per_game=1024)
    assert flag == 0
    G, _ = control_blocks(roomy)
    C0, U0 = int(G["node_count"][0]), int(G["pool_used"][0])
    assert 64 < C0 < 1024
    raw = roomy.read_raw()
    ample = 1 << 20
    for kw, fits in ((dict(nodes_per_game=C0, pool_bytes_per_game=ample), True), (dict(nodes_per_game=C0 - 1, pool_bytes_per_game=ample), False),
                     (dict(nodes_per_game=1024, pool_bytes_per_game=8 * U0), True), (dict(nodes_per_game=1024, pool_bytes_per_game=8 * U0 - 8), False)):
        e, flag = _one_game(make, first, sims, **kw)
        assert int(e.cfg.nodes_per_game) == kw["nodes_per_game"] and e.pool_bytes == kw["pool_bytes_per_game"]
        g, _ = control_blocks(e)
        assert int(g["node_count"][0]) <= kw["nodes_per_game"] and 8 * int(g["pool_used"][0]) <= kw["pool_bytes_per_game"], kw
        if fits:
            assert flag == 0, kw
            assert (int(g["node_count"][0]), int(g["pool_used"][0])) == (C0, U0)
            _same_game(e.read_raw(), 0, raw, 0)
        else:
            assert flag == 1, kw


def flag_survives_harvest(make_shared, first):
    """A game whose error flag is raised stands still, so a flagged slot is harvested only if the flag came up in the step that ended
    its game.  On a shared tree (mirror keys) at ONE simulation per move that is what happens with room for two nodes: the third
    node is the mirror of the second move's root, the move is decided all the same - no visits: square 0, which flips nothing - and
    the game is over, flag 1 raised.  The harvest that restarts the slots must leave the flag raised (the new control block
    inherits it)."""
    e = make_shared(2, nodes_per_game=2)
    e.start(first, np.array([1, 1], dtype=np.uint32))
    step_until(e, lambda: (control_blocks(e)[0]["phase"] == phase("DONE")).all(), chunk=1, max_steps=64)
    G, _ = control_blocks(e)
    assert (G["error"] == 1).all() and (G["status"] != 0).all() and (G["node_count"] == 2).all() and raw_stats(e)["error_flags"] == 1
    outbox = e.new_outbox(first, 3)
    words = check_harvest(e, outbox, first + 2, np.array([1], dtype=np.uint32))
    assert words == (2, 1, 0, 1)
    G, _ = control_blocks(e)
    assert list(G["error"]) == [1, 1] and list(G["game_id"]) == [first + 2, first + 1]
    assert list(G["phase"]) == [phase("NEW_MOVE"), phase("IDLE")]
    assert raw_stats(e)["error_flags"] == 1
    e.step(8)
    assert raw_stats(e)["error_flags"] == 1


def flag_survives_next_game(make_shared, first):
    """On a carried tree (share_mtcs_info: raz_engine_next_game keeps nodes, pool and flag)."""
    e = make_shared(2, nodes_per_game=40)
    e.start(first, np.array([20, 1], dtype=np.uint32))
    step_until(e, lambda: raw_stats(e)["error_flags"] != 0, chunk=4, max_steps=400)
    G0, _ = control_blocks(e)
    assert raw_stats(e)["error_flags"] == 1 and G0["error"][0] == 1
    e.next_game(first + 2, 1)
    G1, _ = control_blocks(e)
    assert list(G1["game_id"]) == [first + 2, first + 3] and (G1["n_plies"] == 0).all() and (G1["sims"] == 0).all()
    assert np.array_equal(G1["error"], G0["error"]) and np.array_equal(G1["node_count"], G0["node_count"]) and np.array_equal(G1["pool_used"], G0["pool_used"])
    assert raw_stats(e)["error_flags"] == 1


def stats_raises(e):
    import pytest
    with pytest.raises(RuntimeError, match=r"flags 0x1\b"):
        e.stats()


def records_full(make, first):
    """max_plies = 64: a finished game's slot is put back on the initial position at one simulation per move, so that recording goes
    on behind the plies it holds: flag 4 when the 65th ply is due, the slot DONE, the neighbour's records untouched."""
    e = make(2, max_plies=64)
    play_to_end(e, first)
    assert raw_stats(e)["error_flags"] == 0
    raw0 = e.read_raw()
    n0 = int(raw0["n_plies"][0])
    assert 4 < n0 <= 64
    for _ in range(64):   # (at one simulation per move a game is a few plies long: as many games as it takes to reach the 65th ply)
        e.set_position(0, INIT_BLACK, INIT_WHITE, 1, 1, enable_resign=True, one_move=False)
        step_until(e, lambda: control_blocks(e)[0]["phase"][0] == phase("DONE"), chunk=4, max_steps=2000)
        if raw_stats(e)["error_flags"]:
            break
    assert raw_stats(e)["error_flags"] == 4
    G, _ = control_blocks(e)
    assert G["error"][0] == 4 and G["error"][1] == 0 and G["phase"][0] == phase("DONE") and G["n_plies"][0] == 64
    raw1 = e.read_raw()
    assert raw1["headers"][0, :n0].tobytes() == raw0["headers"][0, :n0].tobytes()
    for k in ("headers", "root_n", "root_w"):
        assert raw1[k][1].tobytes() == raw0[k][1].tobytes(), k
    e.step(16)
    assert raw_stats(e)["error_flags"] == 4 and control_blocks(e)[0]["n_plies"][0] == 64
    assert e.read_raw()["root_n"][1].tobytes() == raw0["root_n"][1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. pruning
def _discs(b, w):
    return bin(b).count("1") + bin(w).count("1")


def _tree_snapshot(e, positions):
    return {(b, w, p, owner): _node_bits(e, 0, b, w, p, owner) for b, w, p in positions for owner in (0, 1)}


def _positions_around(raw, G):
    """Record positions of slot 0 (fewer discs than the root), the root, and every position one and two moves below it."""
    from reversi_alpha_zero_amd.lib.bitboard import find_correct_moves, calc_flip
    root = (int(G["root_black"][0]), int(G["root_white"][0]), int(G["player"][0]))
    out, frontier = set(_record_positions(raw, 0)) | {root}, [root]
    for _ in range(2):
        nxt = []
        for b, w, p in frontier:
            own, enemy = (b, w) if p == 1 else (w, b)
            legal = find_correct_moves(own, enemy)
            for sq in range(64):
                if (legal >> sq) & 1:
                    f = calc_flip(sq, own, enemy)
                    o2, e2 = own | f | (1 << sq), enemy & ~f
                    q = (o2, e2, 2) if p == 1 else (e2, o2, 1)
                    if not find_correct_moves(*((q[1], q[0]) if q[2] == 2 else (q[0], q[1]))):
                        q = (q[0], q[1], p)   # the opponent passes
                    nxt.append(q)
        out |= set(nxt)
        frontier = nxt
    return sorted(out), root


def pruning(make, first, crossing, sims=40):
    """k_gc on one game whose node directory has just crossed `crossing` nodes (a scan round is 256 nodes): below the threshold
    nothing changes; at it every node that the game can still reach (discs >= the root's) stays bit for bit, the others are gone,
    count and bytes drop, and the game ends as the unpruned one does."""
    e = make(1, nodes_per_game=None, sims_hint=sims)
    e.start(first, np.array([sims], dtype=np.uint32))
    step_until(e, lambda: control_blocks(e)[0]["node_count"][0] >= crossing, chunk=1, max_steps=20000)
    G0, B0 = control_blocks(e)
    assert G0["status"][0] == 0
    count, used = int(G0["node_count"][0]), int(G0["pool_used"][0])
    raw0 = e.read_raw()
    positions, root = _positions_around(raw0, G0)
    snap = _tree_snapshot(e, positions)
    state = snapshot(e)
    step_until(e, lambda: raw_stats(e)["finished_games"] >= 1, chunk=16, max_steps=40000)
    unpruned = e.read_raw()
    restore(e, state)
    e.gc(count + 1)
    assert np.array_equal(control_blocks(e)[1], B0) and _tree_snapshot(e, positions) == snap
    e.gc(count)
    G1, _ = control_blocks(e)
    after = _tree_snapshot(e, positions)
    dmin = _discs(root[0], root[1])
    kept = [k for k in snap if _discs(k[0], k[1]) >= dmin and snap[k][0]]
    gone = [k for k in snap if _discs(k[0], k[1]) < dmin and snap[k][0]]
    assert len(kept) >= 4 and len(gone) >= 4, (len(kept), len(gone))
    for k in kept:
        assert after[k] == snap[k], k
    for k in gone:
        assert not after[k][0], k
    assert int(G1["node_count"][0]) < count and int(G1["pool_used"][0]) < used
    assert 0 < int(G1["node_count"][0])
    for k in ("sims", "n_plies", "phase", "root_black", "root_white"):
        assert G1[k][0] == G0[k][0], k
    step_until(e, lambda: raw_stats(e)["finished_games"] >= 1, chunk=16, max_steps=40000)
    _same_game(e.read_raw(), 0, unpruned, 0)
    return count
