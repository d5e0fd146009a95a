"""GPU: the engine's bookkeeping kernels at their slot-count edges (tests/slot_cases.py holds the scenarios, the numpy references
and the assertions; tests/test_engine_slots_emu.py is the CPU twin on the wave emulator).  k_harvest_plan walks the B slots in
chunks of 1024 with a carried base, k_stats and k_records_extent reduce over 256 threads, k_gc scans a game's node directory 256
nodes per round: B in {1, 255, 256, 257, 1023, 1024, 1025, 2049} and pools that cross 257 / 513 nodes put one slot before, on and
after each of those edges.  Whole games of the golden mini net at 1 + id % 3 simulations per move, played in lock step; a batch is
played once per B and the engine put back to that state (its workspace) for every scenario.  Everything is exact."""
import pytest

import slot_cases as S
from oracle_util import load_mcts_golden, golden_net_blob, config_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
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
    from reversi_alpha_zero_amd.engine import DeviceNet, SelfPlayEngine
    cfg, dnet = _cfg(gold, "agz_resign"), DeviceNet(blob, DEV)

    def make(n, nodes_per_game=512, max_plies=72, pool_bytes_per_game=0, sims_hint=None, config=None):
        return SelfPlayEngine(config or cfg, dnet, n_games=n, seed=S.SEED, nodes_per_game=nodes_per_game, sims_hint=sims_hint, max_plies=max_plies,
                              record_root_w=True, pool_bytes_per_game=pool_bytes_per_game)
    return make


@pytest.fixture(scope="module")
def batch(request, make):
    """An engine of request.param slots whose games have all just finished, and its state to go back to."""
    e = make(request.param)
    S.play_to_end(e, FIRST, chunk=16)
    return e, S.snapshot(e)


def _fresh(batch):
    e, snap = batch
    S.restore(e, snap)
    return e


HARVEST_B = [1, 257, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("batch", HARVEST_B, indirect=True)
def test_harvest_of_a_whole_finished_batch(batch):
    """1(a): all B games finished, n_new = B."""
    e = _fresh(batch)
    lens = e.read_raw()["n_plies"]
    assert e.n_games == 1 or lens.min() < lens.max()
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


@pytest.mark.parametrize("B", HARVEST_B)
def test_continuous_run_against_the_harvest_contract(gold, blob, make, B):
    """1(e) and the harvested totals of 3: 3 B ids through B slots, 8 steps between harvests, the numpy contract applied at every
    call.  B = 1025: the whole outbox == the same ids as lock-step batches of 205 slots read with read_raw(), and six of its games -
    the ids first played in slots 0, 1023, 1024 and three refilled ones - == the oracle's."""
    out = S.continuous_run(make(B), FIRST, 3 * B, chunk=8)
    if B == 1025:
        S.check_outbox_equals_lock_step(out, S.lock_step_outbox(make, FIRST, 3 * B, 205))
        S.check_outbox_rows_equal_oracle(out, FIRST, [FIRST, FIRST + 1023, FIRST + 1024, FIRST + B, FIRST + 2 * B + 1, FIRST + 3 * B - 1],
                                         _cfg(gold, "agz_resign"), blob)


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
    """3, mid-run: after 40 steps - the one-simulation games, a third of the batch, have finished, the others have not."""
    e = make(B)
    S.begin(e, FIRST)
    e.step(40)
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


@pytest.mark.parametrize("crossing", [257, 513])
def test_pruning_at_a_scan_round_boundary(make, crossing):
    """5: k_gc on a directory that has just crossed one / two scan rounds of 256 nodes."""
    assert S.pruning(make, FIRST + 3, crossing) >= crossing
