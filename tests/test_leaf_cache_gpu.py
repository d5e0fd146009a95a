"""GPU: the cross-game evaluation cache (csrc/raz_leaf_cache.hip, raz_engine_set_leaf_cache).  The net is a pure,
batch-invariant function of the position, so serving a repeated position from the table must leave every game exactly as
it is without the cache - actions, root N, root W (f64 bits), resignation flags - while the net sees fewer rows.

Whole games cannot reach the guards that make a served answer the answer of THAT position (played positions never share a tag, no
game leaves a claim unfinished): the second half of this file drives the three kernels row by row through raz_leaf_cache_probe
with the cases of tests/leaf_cache_cases.py, and runs three slices on three streams against one table with no host
synchronisation."""
import types

import numpy as np
import pytest

import leaf_cache_cases as C
from oracle_util import load_mcts_golden, load_par_golden, golden_net_blob, config_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return load_mcts_golden()


@pytest.fixture(scope="module")
def blob(gold):
    return golden_net_blob(gold["net"])


def _play(cfg, dnet, n, seed, sims, cache, first=0, **kw):
    from reversi_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(cfg, dnet, n_games=n, seed=seed, sims_hint=sims, record_root_w=True, leaf_cache_log2=cache, **kw)
    eng.start(first, sims)
    st = eng.run(chunk=64)
    return eng.read_raw(), st, eng.leaf_cache_stats()


def _same(a, b):
    for k in ("n_plies", "status", "resigned", "final_black", "final_white"):
        assert np.array_equal(a[k], b[k]), k
    for g in range(len(a["n_plies"])):   # (record rows beyond a game's plies are never written: compare the plies played)
        n = int(a["n_plies"][g])
        assert np.array_equal(a["headers"][g, :n], b["headers"][g, :n]), g
        assert np.array_equal(a["root_n"][g, :n], b["root_n"][g, :n]), g
        assert np.array_equal(a["root_w"][g, :n].view(np.uint64), b["root_w"][g, :n].view(np.uint64)), g


@pytest.mark.parametrize("variant,n", [("mini_shared", 64), ("agz_resign", 300)])
def test_games_unchanged_by_the_cache_narrow_net(gold, blob, variant, n):
    """mini net (rows served by the cache leave the batch through the `active` mask); 300 games = 3 slices on 3 streams
    sharing one table."""
    from reversi_alpha_zero_amd.engine import DeviceNet
    g0 = next(g for g in gold["games"] if g["variant"] == variant)
    cfg = config_of(g0)
    dnet = DeviceNet(blob, DEV)
    plain, st0, c0 = _play(cfg, dnet, n, 7, 12, None)
    cached, st1, c1 = _play(cfg, dnet, n, 7, 12, 20)
    _same(plain, cached)
    assert c0 == {"hits": 0, "in_batch_duplicates": 0, "evaluated": 0, "no_room": 0}
    assert st1["nn_leaves"] == st0["nn_leaves"] == c1["hits"] + c1["in_batch_duplicates"] + c1["evaluated"]
    # (a leaf is evaluated under a random D4 symmetry, agent/player.py:300-305: a position has 8 keys, so short runs of few
    #  games share little; the openings of thousands of 800-simulation searches share a lot - tools/whole_games_config3.py)
    assert c1["hits"] > 0 and c1["in_batch_duplicates"] > 0 and c1["no_room"] == 0, c1
    print(variant, c1, "of", st1["nn_leaves"], "leaves")


@pytest.mark.parametrize("par", [1, 4])
def test_games_unchanged_by_the_cache_wide_net_compacted(par):
    """128-filter net on the split-f16 trunk: the rows still to evaluate are compacted (conv0 / heads go through the index
    list, the convolutions see a device-side row count).  Also with the slot kernel (4 simulations in flight per game) and a
    table far too small for the run (2^10 entries: most claims find no room and are simply evaluated)."""
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.engine import DeviceNet
    blob = ReversiNet(128, 1, 64).keras_init_(7).randomize_bn_(8).to_blob()
    play = types.SimpleNamespace(
        simulation_num_per_move=14, share_mtcs_info_in_self_play=True, thinking_loop=1, required_visit_to_decide_action=400,
        start_rethinking_turn=8, c_puct=5, noise_eps=0.25, dirichlet_alpha=0.5, change_tau_turn=4, virtual_loss=3,
        parallel_search_num=par, resign_threshold=-0.9, allowed_resign_turn=50, disable_resignation_rate=0.1,
        use_solver_turn=0, use_solver_turn_in_simulation=0)
    cfg = types.SimpleNamespace(play=play, play_data=types.SimpleNamespace(save_policy_of_tau_1=True))
    dnet = DeviceNet(blob, DEV, kernel="f16x3")
    plain, st0, _ = _play(cfg, dnet, 40, 3, 14, None)
    cached, st1, c1 = _play(cfg, dnet, 40, 3, 14, 18)
    tiny, st2, c2 = _play(cfg, dnet, 40, 3, 14, 10)
    _same(plain, cached)
    _same(plain, tiny)
    assert c1["hits"] + c1["in_batch_duplicates"] + c1["evaluated"] == st1["nn_leaves"] == st0["nn_leaves"]
    assert c1["evaluated"] < st1["nn_leaves"] and c1["hits"] > 0 and c1["no_room"] == 0, c1
    assert c2["no_room"] > 0 and c2["evaluated"] > c1["evaluated"], c2
    assert dnet.range_ok()
    print("par", par, c1, c2, "of", st1["nn_leaves"], "leaves")


def test_continuous_batching_with_the_cache(gold, blob):
    """Refilled slots replay the openings the table already holds: 48 ids on 12 slots, outbox == the run without a cache."""
    from reversi_alpha_zero_amd.engine import DeviceNet, SelfPlayEngine
    g0 = next(g for g in gold["games"] if g["variant"] == "agz_resign")
    cfg = config_of(g0)
    dnet = DeviceNet(blob, DEV)
    out = []
    for cache in (None, 16):
        eng = SelfPlayEngine(cfg, dnet, n_games=12, seed=11, sims_hint=10, leaf_cache_log2=cache)
        outbox, st = eng.play_continuous(500, 48, lambda gid: 10, chunk=32)
        out.append(({k: outbox[k].cpu().numpy() for k in ("headers", "root_n", "summary")}, eng.leaf_cache_stats()))
    for k in ("headers", "root_n", "summary"):
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    assert out[1][1]["hits"] > 0


def test_games_unchanged_by_a_cache_with_a_disc_threshold(gold, blob):
    """leaf_cache_max_discs = 12: positions of more than 12 discs go past the table - the games are those without a cache, some
    leaves are still served, and more rows are evaluated than with every position admitted."""
    from reversi_alpha_zero_amd.engine import DeviceNet
    g0 = next(g for g in gold["games"] if g["variant"] == "mini_shared")
    cfg = config_of(g0)
    dnet = DeviceNet(blob, DEV)
    plain, st0, _ = _play(cfg, dnet, 64, 7, 12, None)
    shallow, st1, c1 = _play(cfg, dnet, 64, 7, 12, 20, leaf_cache_max_discs=12)
    _, st2, c2 = _play(cfg, dnet, 64, 7, 12, 20, leaf_cache_max_discs=0)
    _same(plain, shallow)
    assert st1["nn_leaves"] == st0["nn_leaves"] == c1["hits"] + c1["in_batch_duplicates"] + c1["evaluated"]
    assert 0 < c1["hits"] and c1["evaluated"] > c2["evaluated"] and c1["no_room"] == 0, (c1, c2)


# ---------------------------------------------------------------------------------------------------------------- row by row
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def _back(t, a):
    np.copyto(a.view(np.uint8).reshape(-1), t.cpu().numpy())


@pytest.fixture(scope="module")
def run():
    """leaf_cache_cases' `run`: the rig's arrays go to the device, the calls are enqueued back to back on the current stream, and
    the arrays come back."""
    import torch
    from reversi_alpha_zero_amd import _native as N
    names = {"cache": "buf", "own": "own", "enemy": "enemy", "active": "active", "policy": "policy", "value": "value"}

    def run(rig, calls, **ov):
        t = {k: _dev(getattr(rig, a)) for k, a in names.items()}
        ptr = {k: v.data_ptr() for k, v in t.items()}
        assert ptr["cache"] % 256 == 0 and ptr["own"] % 8 == 0 and ptr["enemy"] % 8 == 0
        stream = N.current_stream_ptr()
        rcs = [N.lib.raz_leaf_cache_probe(*C.call_args(rig, ptr, call, ov), stream) for call in calls]
        torch.cuda.synchronize()
        for k, a in names.items():
            _back(t[k], getattr(rig, a))
        return rcs
    return run


def test_the_restated_layout_is_the_tables():
    from reversi_alpha_zero_amd import _native as N
    C.check_layout(N.lib.raz_leaf_cache_bytes)


@pytest.mark.parametrize("case", list(C.CASES))
def test_leaf_cache_rows(run, case):
    C.CASES[case](run)


SLICES = ((0, 256), (256, 257), (513, 87))   # (p0, pn) of the three streams' slices; part = the stream's number
STEPS = 6


def _concurrent_positions():
    """own, enemy [STEPS][600] and active: about half of every slice's rows hold one of 150 positions that all slices and steps
    share, the others a position of their own; one row in 16 is inactive."""
    r = np.random.default_rng([20250311, 50])
    po, pe, _ = C.pool()
    rows = SLICES[-1][0] + SLICES[-1][1]
    idx = 1000 + np.arange(STEPS * rows).reshape(STEPS, rows)
    shared = r.random((STEPS, rows)) < 0.5
    idx[shared] = r.integers(0, 150, int(shared.sum()))
    active = (r.random((STEPS, rows)) >= 1 / 16).astype(np.uint8)
    for p0, pn in SLICES:                                                      # what the test is about is there
        mine = idx[:, p0:p0 + pn]
        other = np.delete(idx, np.s_[p0:p0 + pn], axis=1)
        rep = np.isin(mine, other)
        assert 0.3 < rep.mean() < 0.7 and np.isin(mine[1:], mine[:-1]).mean() > 0.2
    return po[idx], pe[idx], active


@pytest.mark.parametrize("mode", C.MODES)
def test_concurrent_slices_on_three_streams(mode):
    """Three slices of 256, 257 and 87 rows on three streams against one table of 2^10 entries, 6 steps each with distinct step
    values.  prefilled: every row holds its answer beforehand and nothing synchronises until the end, so one stream's fill overlaps
    another's resolve - the RELEASE / ACQUIRE pair on `ready`.  poison: the host plays the net between the halves (one
    synchronisation each), so a copy that never happens shows.  Every assertion is independent of the order of execution."""
    import torch
    from reversi_alpha_zero_amd import _native as N
    own, enemy, active = _concurrent_positions()
    rows = own.shape[1]
    want = np.stack([C.net(own[t], enemy[t]) for t in range(STEPS)])          # [STEPS][rows][65]
    rig = C.Rig(10, rows)
    cache = _dev(rig.buf)
    d_own, d_enemy, d_active = [[_dev(a[t]) for t in range(STEPS)] for a in (own, enemy, active)]
    start = want if mode == "prefilled" else np.full_like(want, C.POISON)
    d_policy = [_dev(start[t, :, :64]) for t in range(STEPS)]
    d_value = [_dev(start[t, :, 64]) for t in range(STEPS)]
    streams = [torch.cuda.Stream(device=DEV) for _ in SLICES]
    assert cache.data_ptr() % 256 == 0

    def call(phase, t, s):
        p0, pn = SLICES[s]
        with torch.cuda.stream(streams[s]):
            N.check(N.lib.raz_leaf_cache_probe(phase, cache.data_ptr(), rig.bytes, 10, 0, rows, d_own[t].data_ptr(), d_enemy[t].data_ptr(),
                                               d_active[t].data_ptr(), d_policy[t].data_ptr(), d_value[t].data_ptr(), p0, pn, s,
                                               1 + len(SLICES) * t + s, streams[s].cuda_stream), "raz_leaf_cache_probe")

    N.check(N.lib.raz_leaf_cache_probe(C.CLEAR, cache.data_ptr(), rig.bytes, 10, 0, rows, d_own[0].data_ptr(), d_enemy[0].data_ptr(),
                                       d_active[0].data_ptr(), d_policy[0].data_ptr(), d_value[0].data_ptr(), 0, 0, 0, 0, N.current_stream_ptr()),
            "raz_leaf_cache_probe")
    torch.cuda.synchronize()
    listed_total = 0
    for t in range(STEPS):
        for s in range(len(SLICES)):
            call(C.BEFORE, t, s)
            if mode == "prefilled":
                call(C.AFTER, t, s)
        if mode == "poison":
            torch.cuda.synchronize()
            _back(cache, rig.buf)
            pol, val = np.full((rows, 64), C.POISON, dtype=np.uint32), np.full(rows, C.POISON, dtype=np.uint32)
            _back(d_policy[t], pol)
            _back(d_value[t], val)
            for s, (p0, pn) in enumerate(SLICES):
                n = int(rig.n_compact[s])
                lst = p0 + rig.list[p0:p0 + n].astype(np.int64)
                assert len(np.unique(lst)) == n and (lst < p0 + pn).all() and active[t][lst].all()
                pol[lst], val[lst] = want[t, lst, :64], want[t, lst, 64]
                listed_total += n
            d_policy[t].copy_(_dev(pol))
            d_value[t].copy_(_dev(val))
            torch.cuda.synchronize()
            for s in range(len(SLICES)):
                call(C.AFTER, t, s)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    _back(cache, rig.buf)
    for t in range(STEPS):
        pol, val = np.zeros((rows, 64), dtype=np.uint32), np.zeros(rows, dtype=np.uint32)
        _back(d_policy[t], pol)
        _back(d_value[t], val)
        a = active[t] != 0
        bad = np.flatnonzero(a & ((pol != want[t, :, :64]).any(axis=1) | (val != want[t, :, 64])))
        assert len(bad) == 0, f"step {t}: rows {bad[:8].tolist()} do not hold the answer of their position"
        assert (pol[~a] == start[t, ~a, :64]).all() and (val[~a] == start[t, ~a, 64]).all()
    ready = C.check_ready_entries(rig)
    used = np.flatnonzero(rig.tags)
    assert (rig.tags[used] == C.leaf_tag(rig.keys[used, 0], rig.keys[used, 1])).all()
    assert len(ready) > 100 and len(set(map(tuple, rig.keys[used].tolist()))) == len(used)
    hits, dups, evaluated, no_room = rig.counters.tolist()[:4]
    assert hits + dups + evaluated == int(active.sum()) and hits > 0 and dups > 0 and no_room <= evaluated, rig.counters
    assert rig.counters.tolist()[4:] == [0, 0, 0, 0]
    if mode == "poison":
        assert evaluated == listed_total
