"""GPU: raznet-forward-v3, the plain-f16 trunk (DeviceNet(kernel="f16"), raz_net.reserved = 8; csrc/raz_net_f16x3.hip with
SPLIT = false).  The cases and their reasoning are in tests/net_f16_cases.py; tests/test_net_f16_emu.py runs the cheap ones on the
wave emulator.

  1. integer nets, where nothing in v3 rounds: equal to the exact-f32 kernels on every row and to the C oracle, bit for bit;
  2. sharp float nets: the distance from the f64 graph is the quantisation's (the f64 restatement of the specification) and no more;
  3. rows out of the f16 range are repaired by the exact-f32 chains, too many of them raise the sticky flag;
  4. games: the engine on this net == the oracle fed with this net's outputs, with and without a leaf cache (the compacted path)."""
import numpy as np
import pytest
import torch

import net_cases as C
import net_f16_cases as K
import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _net(blob, kernel):
    from reversi_alpha_zero_amd.engine import DeviceNet
    return DeviceNet(blob, DEV, kernel=kernel)


def _run(dn, own, enemy, active=None):
    p, v = dn.predict_bitboards(_dev(own), _dev(enemy), None if active is None else torch.from_numpy(active).to(DEV))
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy()


_EXACT = {}


ORACLE_ROWS = (0, 7, K.POOL - 1)   # three rows per shape for the C oracle, as net_cases.oracle_rows picks them: first, last, one between


def _exact(shape):
    """(blob, the exact-f32 kernels' policy and value over the whole pool, the C oracle's over ORACLE_ROWS): computed once per
    shape, shared by the batch sizes."""
    if shape not in _EXACT:
        blob, maxima = K.integer_net(*shape)
        print(f"{shape}: layer maxima {maxima}")
        own, enemy = K.positions()
        p, v = _run(_net(blob, "f32"), own, enemy)
        C.assert_sharp(p, v, str(shape))
        o = O.load_ext()
        orc = {}
        for i in ORACLE_ROWS:
            op, ov = np.zeros(64, np.float32), np.zeros(1, np.float32)
            assert o.orc_net_forward(blob, len(blob), int(own[i]), int(enemy[i]), op.ctypes.data, ov.ctypes.data) == 0
            orc[i] = (op, ov)
        _EXACT[shape] = (blob, p, v, orc)
    return _EXACT[shape]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 67])
@pytest.mark.parametrize("shape", K.INTEGER_CASES, ids=lambda s: "x".join(map(str, s)))
def test_plain_f16_trunk_equals_the_exact_kernels_bit_for_bit_on_integer_nets(shape, n):
    """The test that carries the kernel (net_f16_cases.integer_net: nothing in v3 rounds on such a net): v3 == kernel="f32" on every
    row and == the C oracle on ORACLE_ROWS, policy and value, at a single row, a partly filled group of 8 positions, a
    full one, one row more, and more than 8 groups (n = 67: the second round of the block -> (oc tile, position group) mapping); F = 256
    has two output-channel tiles per group.  With an `active` mask the skipped rows come back untouched; the range flag stays
    clear; a row alone == the same row inside the batch."""
    blob, xp, xv, orc = _exact(shape)
    own, enemy = K.positions(n)
    dn = _net(blob, "f16")
    assert dn.form(n) == "f16_repair"
    p, v = _run(dn, own, enemy)
    assert np.array_equal(_bits(p), _bits(xp[:n])) and np.array_equal(_bits(v), _bits(xv[:n])), (shape, n)
    for i, (op, ov) in orc.items():
        if i < n:
            assert np.array_equal(_bits(p[i]), _bits(op)) and _bits(v)[i] == _bits(ov)[0], (shape, n, i)
    if n > 1:
        active = (np.arange(n) % 5 != 1).astype(np.uint8)
        on = active.astype(bool)
        pm, vm = _run(dn, own, enemy, active)   # (predict_bitboards hands zeroed outputs to a masked forward)
        assert np.array_equal(_bits(pm[on]), _bits(xp[:n][on])) and np.array_equal(_bits(vm[on]), _bits(xv[:n][on]))
        assert (pm[~on] == 0).all() and (vm[~on] == 0).all()
        i = n - 1
        pa, va = _run(dn, own[i:i + 1], enemy[i:i + 1])
        assert np.array_equal(_bits(pa[0]), _bits(p[i])) and _bits(va)[0] == _bits(v)[i]
    assert dn.range_stats() == (True, 0)


@pytest.mark.parametrize("shape", [(128, 1, 64), (256, 2, 64)], ids=lambda s: "x".join(map(str, s)))
def test_plain_f16_trunk_error_is_the_quantisations_and_no_more(shape):
    """On sharp float nets over net_cases.inputs() (random positions, the edge boards, the overlap rows): E_k, the kernel's (max, mean)
    distance from the f64 graph, against E_q, that of the f64 restatement of v3's specification (net_f16_cases.quantised_reference):
    E_k <= (4, 2.5) x E_q (+ within_fp32_rule's floors), and E_k[mean] > 1e-5 - the form runs on single products, it is not v2 under
    another name.  A row alone == the row inside the batch."""
    F, R, V = shape
    own, enemy, names = C.inputs()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = C.sharp_net(F, R, V, F + R, own, enemy, device=DEV)
    rp, rv = C.reference(net, own, enemy, device=DEV)
    C.assert_sharp(rp, rv, str(shape))
    e_q = C.errors(*K.quantised_reference(net, own, enemy, device=DEV), rp, rv)
    dn = _net(net.to_blob(), "f16")
    p, v = _run(dn, own, enemy)
    e_k = C.errors(p, v, rp, rv)
    print(f"{shape} v3: E_k max {e_k[0]:.3g} mean {e_k[1]:.3g}; E_q max {e_q[0]:.3g} mean {e_q[1]:.3g}")
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert K.within_quantisation_rule(e_k, e_q), (shape, e_k, e_q)
    assert e_k[1] > K.MIN_MEAN_ERROR, (shape, e_k)
    for i in C.oracle_rows(names):
        pa, va = _run(dn, own[i:i + 1], enemy[i:i + 1])
        assert np.array_equal(_bits(pa[0]), _bits(p[i])) and _bits(va)[0] == _bits(v)[i], (shape, i)
    assert dn.range_stats() == (True, 0)


def test_plain_f16_range_flag():
    """tests/test_engine_gpu.py test_net_f16x3_range_flag's construction with kernel="f16": a net whose activations leave the f16
    range never returns garbage silently - 8 such rows are evaluated by the exact-f32 chains inside the forward (== the f32 kernels,
    bit for bit; range_stats == (True, 8)), 40 in one forward raise the sticky flag while every row is still answered exactly."""
    blob = K.net_that_overflows(128, 1, 64)
    v1 = _net(blob, "f32")
    for n, in_range in ((8, True), (40, False)):
        own, enemy = K.harvested_positions(n, 2)
        v3 = _net(blob, "f16")
        assert v3.range_ok()
        p3, q3 = _run(v3, own, enemy)
        p1, q1 = _run(v1, own, enemy)
        assert np.array_equal(_bits(p3), _bits(p1)) and np.array_equal(_bits(q3), _bits(q1))
        assert v3.range_stats() == (in_range, n) and v3.range_ok() == in_range


def _compare_game(tag, eng_plies, eng_sum, ref_plies, ref_winner):
    """tests/test_engine_gpu.py _compare_game: actions, root N and W (the records carry the device's doubles), the saved policies."""
    assert [p["action"] for p in eng_plies] == [p["action"] for p in ref_plies], tag
    assert eng_sum["winner"] == ref_winner, tag
    for i, (a, b) in enumerate(zip(eng_plies, ref_plies)):
        assert a["player"] == b["player"] and a["own"] == b["own"] and a["enemy"] == b["enemy"], (tag, i)
        assert a["root_n"] == b["root_n"], (tag, i)
        assert a["root_w"] == b["root_w"], (tag, i)
        assert a["has_row"] == b["has_row"], (tag, i)
        if a["action"] >= 0:
            assert a["n"] == b["n"] and a["q"] == b["q"], (tag, i)
        if b["has_row"]:
            assert a["saved_policy"] == b["saved_policy"], (tag, i)


@pytest.mark.parametrize("par,cache", [(1, None), (4, None), (4, 12)])
def test_engine_on_plain_f16_net_equals_oracle_given_the_nets_outputs(par, cache):
    """tests/test_engine_gpu.py test_engine_on_f16x3_net_equals_oracle_given_the_nets_outputs' construction with kernel="f16" (par =
    parallel_search_num: k_tree / the slot kernel k_tree_par), and once more with a leaf cache attached - the engine then compacts the
    rows still to evaluate and the forward runs its list / n_ptr path (raz_net_forward_compact): the engine's games == the CPU
    oracle's when the oracle evaluates its leaves through the SAME device net - a row's answer is a function of its position alone -
    every action, root N and W, bit for bit."""
    import types
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    from reversi_alpha_zero_amd.engine import SelfPlayEngine
    blob = ReversiNet(128, 1, 64).keras_init_(7).randomize_bn_(8).to_blob()
    play = types.SimpleNamespace(
        simulation_num_per_move=14, share_mtcs_info_in_self_play=True, thinking_loop=1, required_visit_to_decide_action=400,
        start_rethinking_turn=8, c_puct=5, noise_eps=0.25, dirichlet_alpha=0.5, change_tau_turn=4, virtual_loss=3,
        parallel_search_num=par, resign_threshold=-0.9, allowed_resign_turn=50, disable_resignation_rate=0.1,
        use_solver_turn=0, use_solver_turn_in_simulation=0)
    cfg = types.SimpleNamespace(play=play, play_data=types.SimpleNamespace(save_policy_of_tau_1=True))
    dnet = _net(blob, "f16")
    n = 12
    eng = SelfPlayEngine(cfg, dnet, n_games=n, seed=3, sims_hint=14, record_root_w=True, leaf_cache_log2=cache)
    eng.start(first_game_id=40, sims_per_move=14)
    eng.run(chunk=64)
    recs = eng.records()
    if cache:
        st = eng.leaf_cache_stats()
        print(f"par {par} leaf cache: {st}")
        assert st["evaluated"] > 0 and st["hits"] + st["in_batch_duplicates"] > 0   # some rows were served, so batches were compacted

    def nn(own, enemy):
        to = lambda v: torch.tensor([v - (1 << 64) if v >= 1 << 63 else v], dtype=torch.int64, device=DEV)
        p, v = dnet.predict_bitboards(to(own), to(enemy))
        return p[0].cpu().numpy(), float(v[0].item())
    ocfg = O.play_cfg_from_config(cfg, parallel_search_num=par)
    for i in (0, 5, 11):
        plies, summ = O.selfplay_game(ocfg, None, 3, 40 + i, 14, nn=nn)
        _compare_game(f"f16/par{par}/cache{cache}/{40 + i}", recs[i][0], recs[i][1], plies, summ["winner"])
    assert dnet.range_ok()
