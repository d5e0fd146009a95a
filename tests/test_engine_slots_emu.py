"""CPU twin of tests/test_engine_slots_gpu.py: the scenarios of tests/slot_cases.py - harvest, record packing, statistics, the
capacity guards and the error flag, pruning at a scan-round boundary - on the wave emulator (emu_util.EmuEngine), so that the
bookkeeping kernels' LOGIC is checked where there is no GPU.  The emulator plays a simulation of one game in about two milliseconds:
whole games on a thousand slots take minutes, so batches of more than 8 slots are brought to their end from positions two plies
before the end of 8 games played once (start(n_active=0) + set_positions(one_move=False, sims=1): slot g gets position g % 8), and
B = 1023 / 2049 and the slot-count edges of the continuous run 1(e) are left to the GPU file (here it runs at 5 slots).  Measured:
48 s for this file in one process (37 tests), the largest shares being the 1025-slot batch whose two long games are whole games
(8 s) and the five 1024 / 1025-slot batches at 3 s each."""
import pytest

import slot_cases as S
from emu_util import EmuEngine
from oracle_util import load_mcts_golden, golden_net_blob, config_of

FIRST = 1000


@pytest.fixture(scope="module")
def gold():
    return load_mcts_golden()


@pytest.fixture(scope="module")
def blob(gold):
    return golden_net_blob(gold["net"])


def _cfg(gold, variant):
    return config_of(next(g for g in gold["games"] if g["variant"] == variant))


@pytest.fixture(scope="module")
def make(gold, blob):
    cfg = _cfg(gold, "agz_resign")

    def make(n, nodes_per_game=512, max_plies=72, pool_bytes_per_game=0, sims_hint=None, config=None):
        return EmuEngine(config or cfg, blob, n_games=n, seed=S.SEED, nodes_per_game=nodes_per_game, sims_hint=sims_hint, max_plies=max_plies,
                         record_root_w=True, pool_bytes_per_game=pool_bytes_per_game)
    return make


@pytest.fixture(scope="module")
def endings(make):
    """Positions two plies before the end of 8 whole games (ids FIRST ..)."""
    e = make(8)
    S.play_to_end(e, FIRST)
    return S.endings_of(e, FIRST)


@pytest.fixture(scope="module")
def batch(request, make, endings):
    """An engine of request.param slots whose games have all just finished, and its state to go back to."""
    e = make(request.param)
    S.play_to_end(e, FIRST, endings if request.param > 8 else None)
    return e, S.snapshot(e)


def _fresh(batch):
    e, snap = batch
    S.restore(e, snap)
    return e


HARVEST_B = [1, 257, 1024, 1025]


@pytest.mark.parametrize("batch", HARVEST_B, indirect=True)
def test_harvest_of_a_whole_finished_batch(batch):
    """1(a): all B games finished, n_new = B."""
    e = _fresh(batch)
    S.harvest_all_at_once(e, FIRST, e.n_games)


@pytest.mark.parametrize("batch", HARVEST_B, indirect=True)
def test_harvest_restart_idle_split_around_the_scan_chunk(batch):
    """1(b): n_new in {0, 1, min(B, 1023), min(B, 1024)}: the last restarted slot falls before, on and after the 1024-slot chunk."""
    B = batch[0].n_games
    for n_new in sorted({0, 1, min(B, 1023), min(B, 1024)}):
        S.harvest_all_at_once(_fresh(batch), FIRST, n_new)


@pytest.mark.parametrize("batch", HARVEST_B, indirect=True)
def test_harvest_leaves_games_outside_the_outbox_in_place(batch):
    """1(c)."""
    S.harvest_windows(_fresh(batch), FIRST)


@pytest.mark.parametrize("B", HARVEST_B)
def test_harvest_before_anything_has_finished(make, B):
    """1(d)."""
    S.harvest_nothing_finished(make(B), FIRST)


def test_continuous_run_against_the_harvest_contract(make):
    """1(e) at 5 slots and the harvested totals of 3 (counters 8 .. 11 of k_stats): 15 ids through 5 slots, 8 steps between
    harvests, the numpy contract and the statistics checked at every call.  (The slot-count edges of 1(e): the GPU file.)"""
    S.continuous_run(make(5), FIRST, 15, chunk=8)


@pytest.mark.parametrize("batch", [257, 1025], indirect=True)
def test_records_extent_and_pack_records(batch):
    """2."""
    e = _fresh(batch)
    S.check_records_extent(e)
    S.check_pack_records(e)


@pytest.mark.parametrize("B,K", [(257, 256), (1025, 805)])
def test_records_extent_beyond_the_first_stride(make, B, K):
    """2, the longest game at an index >= 256 of the range: only slots K and B - 1 play more than 2 plies, so the greatest length
    lies in the second (B = 257), third or fourth (B = 1025) stride of the reduction's loop and nowhere else."""
    e = make(B)
    S.far_batch(e, FIRST, K)
    S.check_records_extent_far(e, K)


@pytest.mark.parametrize("batch", [1, 255, 256, 257, 1025], indirect=True)
def test_stats_at_the_end(batch):
    """3, at the end of the batch."""
    st = S.check_stats(_fresh(batch))
    assert st["finished_games"] == batch[0].n_games


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1025])
def test_stats_mid_run(make, B):
    """3, mid-run, on whole games: after 40 steps (B = 1), after 3 steps otherwise (a step of 1025 emulated slots takes a second) -
    every game has simulated, at 1, 2 or 3 simulations per move, and the one-simulation games, a third of the batch, have finished
    (they end with the second step), so the statistics' status == 0 filter has games on both sides."""
    e = make(B)
    S.begin(e, FIRST)
    e.step(40 if B <= 8 else 3)
    st = S.check_stats(e)
    assert st["total_sims"] >= B and (B < 3 or 0 < st["finished_games"]) and st["finished_games"] < B and st["max_pool_used"] > 0


@pytest.fixture(scope="module")
def roomy(make):
    return S.roomy_pair(make, FIRST)


def test_pool_full_by_node_count_and_stats_raises(make, roomy):
    """4: pool full by node count; engine.stats() raises."""
    e = S.pool_full(make, FIRST, roomy, nodes_per_game=40)
    S.stats_raises(e)


def test_pool_full_by_bytes(make, roomy):
    e = S.pool_full(make, FIRST, roomy, nodes_per_game=4096, pool_bytes_per_game=40 * 232)
    assert S.control_blocks(e)[0]["node_count"][0] < 4096


def test_pool_exact_fit(make):
    S.exact_fit(make, FIRST + 7)


def test_flag_survives_harvest_and_next_game(gold, make):
    """4, stickiness: k_harvest_apply and k_next_game hand the flag on to the slot's next game."""
    shared = _cfg(gold, "mini_shared")
    S.flag_survives_harvest(lambda n, **kw: make(n, config=shared, **kw), FIRST)
    S.flag_survives_next_game(lambda n, **kw: make(n, config=shared, **kw), FIRST)


def test_records_full(make):
    S.records_full(make, FIRST)


def test_pruning_at_the_first_scan_round_boundary(make):
    """5, first crossing of 257 nodes (513: the GPU file)."""
    assert S.pruning(make, FIRST + 3, 257) >= 257
