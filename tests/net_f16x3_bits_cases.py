"""Cases of tests/test_net_f16x3_bits_gpu.py and of the script that records its fixture (tests/golden/make_golden_f16x3_bits.py):
the bits of raznet-forward-v2 (split-f16 trunk) and v3 (plain f16) at the smallest shapes where the trunk's epilogue, the first-layer
kernel and the compacted forward can go wrong.

Nets (F, R, V), ReversiNet.keras_init_(0): (128, 1, 16) - one output-channel tile, no second residual block; (256, 2, 16) - two tiles
(the block -> (tile, position group) mapping) and a second block, whose skip path reads what the first block's epilogue wrote.
Rows: 1, 7, 8, 9 (8 rows make a workgroup of the trunk kernel; the first-layer kernel takes them in pairs), 63, 64, 65 (8 workgroups
make a run on one XCD).  Each count three ways: plain; with an `active` mask that switches off rows 0 and n - 1; and through the
compacted form - n self-play games with an evaluation cache, where the rows still to evaluate are listed on the device and their
count stays below n (all games start from one opening, which has two images under the eight symmetries: most rows of the first
step are duplicates), so surplus workgroups of every kernel exit.

A kernel's answer is a function of the row's position alone (batch invariance, tested elsewhere), so the plain and masked cases of
all counts share one table of answers per (net, version); the recording script checks that before it writes one."""
import types

import numpy as np

NETS = ((128, 1, 16), (256, 2, 16))
COUNTS = (1, 7, 8, 9, 63, 64, 65)
VERSIONS = {"v2": "f16x3", "v3": "f16"}       # fixture key -> DeviceNet(kernel=...)
POOL = max(COUNTS)
STEPS = 8                                     # engine steps of a compacted case
SIMS = 12
DEV = "cuda:0"


def key(shape):
    return "x".join(map(str, shape))


def blob(shape):
    from reversi_alpha_zero_amd.agent.model import ReversiNet
    return ReversiNet(*shape).keras_init_(0).to_blob()


def positions():
    """The first POOL boards of net_cases.inputs(): 48 random positions of random density, the empty board, a full one, and single
    discs from the corner on (every off-board tap of the first squares)."""
    import net_cases
    own, enemy, _ = net_cases.inputs()
    return own[:POOL].copy(), enemy[:POOL].copy()


def mask(n):
    a = np.ones(n, np.uint8)
    a[0] = a[n - 1] = 0
    return a


def forward(dn, own, enemy, active=None):
    """(policy, value) as uint32 bit patterns."""
    import torch
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)
    p, v = dn.predict_bitboards(to(own), to(enemy), None if active is None else torch.from_numpy(active).to(DEV))
    torch.cuda.synchronize()
    return p.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)


def digest(policy_bits, value_bits):
    """uint64 [rows, 2]: a position-weighted sum of the row's 64 policy words (any changed bit changes it, and so does a swap of two
    unequal words) and the value word."""
    w = np.arange(1, 65, dtype=np.uint64)[None, :]
    return np.stack([(policy_bits.astype(np.uint64) * w).sum(axis=1, dtype=np.uint64), value_bits.astype(np.uint64)], axis=1)


def play_config():
    play = types.SimpleNamespace(
        simulation_num_per_move=SIMS, share_mtcs_info_in_self_play=True, thinking_loop=1, required_visit_to_decide_action=400,
        start_rethinking_turn=8, c_puct=5, noise_eps=0.25, dirichlet_alpha=0.5, change_tau_turn=4, virtual_loss=3,
        parallel_search_num=1, resign_threshold=-0.9, allowed_resign_turn=50, disable_resignation_rate=0.1,
        use_solver_turn=0, use_solver_turn_in_simulation=0)
    return types.SimpleNamespace(play=play, play_data=types.SimpleNamespace(save_policy_of_tau_1=True))


def compacted(dn, n):
    """n games from the opening with an evaluation cache of 2^12 entries, STEPS steps.  -> (uint64 [STEPS, n, 4]: per step and
    exchange row the position shown to the net (own, enemy) and the digest of the answer the row holds after the step;
    the cache's counters)."""
    from reversi_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(play_config(), dn, n_games=n, seed=5, sims_hint=SIMS, leaf_cache_log2=12)
    eng.start(700, SIMS)
    ex = eng.leaf_exchange()
    for name in ("own", "enemy", "policy", "value"):   # the workspace is not initialised: a row no step writes reads as zeros
        ex[name].zero_()
    out = np.zeros((STEPS, n, 4), np.uint64)
    for t in range(STEPS):
        eng.step(1)
        ex = eng.leaf_exchange()
        out[t, :, 0] = ex["own"].cpu().numpy().view(np.uint64)
        out[t, :, 1] = ex["enemy"].cpu().numpy().view(np.uint64)
        out[t, :, 2:] = digest(ex["policy"].cpu().numpy().view(np.uint32), ex["value"].cpu().numpy().view(np.uint32))
    return out, eng.leaf_cache_stats()
