"""Host-side driver objects over the C ABI (include/raz.h): DeviceNet (raz_net_*), SelfPlayEngine (raz_engine_*), DeviceMatch
(raz_match_*), DeviceLeague (raz_league_*) and DeviceAnalysis (raz_analysis_*).  torch is used only to own HBM buffers and the HIP stream.
How a wrapper reaches its library - the device guard, the call, the stream - is _native.Wrapper._launch over a _native.Backend: HIP for
the product (there is no CPU fallback: nothing here makes another), the wave emulator's for the CPU tests, which drive these same classes.

SelfPlayEngine replaces, for a batch of concurrent games, the reference's
SelfPlayWorker.start_game loop (worker/self_play.py:139-175) with two ReversiPlayers per game
(agent/player.py); `records()` returns, per game, exactly the per-ply facts the reference worker
keeps (ReversiPlayer.moves rows are derived from them in worker/self_play.py of this package).
"""
import ctypes
import os

import numpy as np

from . import _native as N
from ._native import lib, check, current_stream_ptr as _stream  # noqa: F401  (tools and tests take them from here)

NODE_POOL_BYTES_PER_NODE = 232   # csrc/raz_engine.h RAZ_NODE_DEFAULT_BYTES: a game's default pool budget per node of nodes_per_game
NODE_MAX_BYTES = 704             # RAZ_NODE_MAX_BYTES: 40 B header + 20 B x 33 legal moves
WHOLE_GAME_BYTES_PER_NODE = 320  # byte budget per node of a pool sized for whole games (never pruned)

PLY_HEADER = np.dtype([("own", "<u8"), ("enemy", "<u8"), ("n", "<f8"), ("q", "<f8"), ("action", "i1"),
                       ("player", "u1"), ("turn", "u1"), ("has_row", "u1"), ("sims", "<u4"),
                       ("loops", "<u4"), ("flags", "<u4")])
assert PLY_HEADER.itemsize == 48


# include/raz.h RAZ_NET_FORM_*
FORMS = {1: "mfma", 2: "mfma_wave", 3: "wave_lds", 4: "wave_scratch", 5: "wide", 6: "f16x3_repair", 7: "f16x3_no_repair",
         8: "f16_repair", 9: "f16_no_repair"}


class DeviceNet(N.Wrapper):
    """The policy/value net resident in HBM (agent/api.py ReversiModelAPI role, device side)."""

    def __init__(self, blob: bytes, device="cuda:0", force_valu_kernel=False, kernel=None, *, backend=None):
        """kernel: None / "f32" = the exact-f32 kernels chosen by shape (raznet-forward-v1, bit-identical to the CPU oracle);
        "f16x3" = raznet-forward-v2 for filters % 128 == 0: the 3x3 trunk on the f16 matrix cores with split operands, within
        1e-5 of the fp32 graph (include/raz.h raz_net_range_check); "auto" = "f16x3" where supported, else "f32".
        "f16" = raznet-forward-v3 for filters % 128 == 0, opt-in only ("auto" never picks it): the same trunk on plain f16 operands,
        one matrix instruction per product instead of three.  The trade: a faster trunk for f16's own accuracy - activations and
        weights rounded to 11 bits, outputs NOT within 1e-5 of the graph - which self-play under root noise tolerates and a
        comparison against a reference does not.
        Test variants: "valu" = k_net_wave; "mfma_wave" = one single-wave workgroup per position.
        backend: the build of the C ABI to run on (None: _native.HIP, the only one the product makes)."""
        import torch
        import struct
        self.backend = backend or N.HIP
        magic, ver, F, R, V = struct.unpack_from("<5i", blob, 0)
        nbytes = self.lib.raz_net_weight_bytes(F, R, V)
        if nbytes == 0:
            raise ValueError(f"unsupported net shape F={F} R={R} V={V}")
        self.device = torch.device(device)
        self.filters, self.res_layers, self.value_fc = F, R, V
        self._weights = self.backend.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.c = N.RazNet()
        kernel = "valu" if force_valu_kernel else kernel
        if kernel == "auto":
            kernel = "f16x3" if (F >= 128 and F % 128 == 0) else "f32"
        self.kernel_name = {None: "f32", "f32": "f32", "f16x3": "f16x3 split-operand MFMA trunk",
                            "f16": "plain-f16 MFMA trunk (raznet-forward-v3)"}.get(kernel, kernel)
        self.c.reserved = {None: 0, "f32": 0, "valu": 1, "mfma_wave": 2, "f16x3": 4, "f16": 8}[kernel]
        self._launch("raz_net_load", ctypes.byref(self.c), blob, len(blob), self._weights.data_ptr(), nbytes)
        self._scratch = None

    def scratch(self, n):
        import torch
        need = self.lib.raz_net_scratch_bytes(self.filters, self.value_fc, n)
        if need and (self._scratch is None or self._scratch.numel() < need):
            self._scratch = self.backend.empty(need, dtype=torch.uint8, device=self.device)
        return (self._scratch.data_ptr(), self._scratch.numel()) if need else (None, 0)

    def form(self, n=1):
        """The kernel form a forward of n positions runs on (include/raz.h raz_net_form): one of FORMS' names."""
        f = self.lib.raz_net_form(ctypes.byref(self.c), n)
        if f < 0:
            raise RuntimeError(f"raz_net_form failed (code {f}): {self.backend.last_error()}")
        return FORMS[f]

    def range_ok(self):
        """False when a split-f16 activation left the f16 range since the net was loaded (raz_net_range_check)."""
        v = ctypes.c_int(0)
        self._launch("raz_net_range_check", ctypes.byref(self.c), ctypes.byref(v))
        return v.value == 0

    def range_stats(self):
        """(in range, rows repaired): rows of split-f16 forwards since the net was loaded whose activations left the f16 range and
        were evaluated on the exact-f32 chains instead (include/raz.h raz_net_range_stats)."""
        v, r = ctypes.c_int(0), ctypes.c_ulonglong(0)
        self._launch("raz_net_range_stats", ctypes.byref(self.c), ctypes.byref(v), ctypes.byref(r))
        return v.value == 0, int(r.value)

    def predict_bitboards(self, own, enemy, active=None):
        """own/enemy: int64 device tensors (side to move's view).  -> (policy (n,64), value (n,)).
        active (uint8 device tensor, optional): positions with 0 are skipped, their outputs stay 0."""
        import torch
        n = own.numel()
        alloc = torch.zeros if active is not None else torch.empty
        policy = alloc((n, 64), dtype=torch.float32, device=self.device)
        value = alloc((n,), dtype=torch.float32, device=self.device)
        sp, sb = self.scratch(n)
        self._launch("raz_net_forward", ctypes.byref(self.c), own.data_ptr(), enemy.data_ptr(), active.data_ptr() if active is not None else None,
                     policy.data_ptr(), value.data_ptr(), n, sp, sb)
        return policy, value


def _tuning_env(name):
    """A tuning knob from the environment - honoured ONLY under RAZ_TUNING=1 (GPU tuning sessions, tools/sessions/): a stray variable in a
    production environment must not reach an engine's configuration."""
    return int(os.environ.get(name, "0") or 0) if os.environ.get("RAZ_TUNING") == "1" else 0


CONTINUOUS_SOLVER_POOL_EVERY = 3   # play_continuous: tree launches per round of the solver pool (tools/sessions/r5_s19.sh: 2: 27.2, 3: 30.3, 4: 30.0, 6: 28.7 M)


def engine_config_from(config, n_games, seed, nodes_per_game, max_plies=72, mirror_updates=None,
                       record_root_w=False, phase_profile=False, single_stream=False, parts=0, inner_max=0, solver_memo_slots=1 << 16,
                       force_slot_kernel=False, pool_bytes_per_game=0, fused=False, solver_budget=0, solver_pool_waves=0, solver_pool_every=0):
    """raz_engine_config from a Config-like object with `.play` / `.play_data` (reference names).
    play.parallel_search_num (config.py:142): 1 = the reference's reproducible mode (k_tree); 2..16 =
    that many simulations in flight per game on the raz-sched-v1 schedule (k_tree_par).
    solver_budget: iterations a worker lane of the end-game solver's pool runs between two tree launches (rounded up to 64; 0 = the library's default, 96);
    solver_pool_waves: worker wavefronts of that pool (0 = one per four games, at most 1280); solver_pool_every: tree launches per round
    of the pool (0 = the library's default, 1 = every step waits for the round, n > 1 = the round runs beside the next n - 1 steps on its
    own stream).  None of them changes a result."""
    p = config.play
    par = int(getattr(p, "parallel_search_num", 1) or 1)
    if not 1 <= par <= 16:
        raise ValueError("parallel_search_num must be 1..16 (prediction_queue_size, config.py:141)")
    # agent/player.py:411: temperature = min(exp(1 - (turn / policy_decay_turn) ** policy_decay_power), 1) is 1 - i.e. inert - for every
    # turn <= policy_decay_turn when the power is >= 0 (config.py:150 "not used": 60, 3).  Anything else would change the search's
    # priors; the engine does not implement it and says so instead of ignoring the value.
    pdt, pdp = getattr(p, "policy_decay_turn", 60), getattr(p, "policy_decay_power", 3)
    if pdt is not None and pdp is not None and (float(pdt) < 60 or float(pdp) < 0):
        raise ValueError(f"policy_decay_turn={pdt} / policy_decay_power={pdp} would decay the policy inside a game (agent/player.py:411); "
                         "only the inert setting (turn >= 60, power >= 0) is supported")
    ust = int(getattr(p, "use_solver_turn", 0) or 0)
    usts = int(getattr(p, "use_solver_turn_in_simulation", 0) or 0)
    share = bool(p.share_mtcs_info_in_self_play)
    mirror = share if mirror_updates is None else bool(mirror_updates)
    slots = 16
    while slots < 2 * nodes_per_game:
        slots *= 2
    c = N.RazEngineConfig(
        thinking_loop=p.thinking_loop, required_visit_to_decide_action=p.required_visit_to_decide_action,
        start_rethinking_turn=p.start_rethinking_turn, change_tau_turn=p.change_tau_turn,
        virtual_loss=p.virtual_loss, allowed_resign_turn=p.allowed_resign_turn,
        has_resign_threshold=int(p.resign_threshold is not None), share_mtcs_info=int(share),
        mirror_updates=int(mirror), record_root_w=int(record_root_w), c_puct=float(p.c_puct),
        noise_eps=float(p.noise_eps), dirichlet_alpha=float(p.dirichlet_alpha),
        resign_threshold=float(p.resign_threshold if p.resign_threshold is not None else 0.0),
        disable_resignation_rate=float(p.disable_resignation_rate), n_games=n_games,
        nodes_per_game=nodes_per_game, table_slots=slots, max_plies=max_plies, seed=seed,
        reserved=(1 if phase_profile else 0) | (2 if single_stream else 0) | (8 if force_slot_kernel else 0)
        | (16 if fused else 0) | ((parts & 0xf) << 8) | ((inner_max & 0xf) << 12) | ((min(255, (int(solver_budget) + 63) // 64) & 0xff) << 16) | ((int(solver_pool_every or _tuning_env("RAZ_SOLVER_POOL_EVERY")) & 0xf) << 24),
        use_solver_turn=ust, use_solver_turn_in_simulation=usts,
        solver_memo_slots=(solver_memo_slots if (ust or usts) else 0), parallel_search_num=par,
        pool_bytes_per_game=int(pool_bytes_per_game or 0), solver_pool_waves=int(solver_pool_waves or 0))
    return c


class SelfPlayEngine(N.Wrapper):
    def __init__(self, config, net: DeviceNet, n_games, seed=0, nodes_per_game=None, sims_hint=None,
                 max_plies=72, mirror_updates=None, record_root_w=False, phase_profile=False, single_stream=False, parts=0, inner_max=0,
                 force_slot_kernel=False, leaf_cache_log2=None, leaf_cache_max_discs=0, pool_bytes_per_game=0, fused=False, solver_budget=0,
                 solver_pool_waves=0, solver_pool_every=0):
        """fused: 16-filter nets - tree and net in ONE kernel, every game's wave evaluating its own leaves (csrc/raz_engine_fused.hip:
        k_tree_net, k_tree_par_net for parallel_search_num > 1; the same results bit for bit, +40 % on BASELINE configs[1]; what
        BatchedSelfPlayWorker selects for 16-filter nets).  No evaluation cache in that form.
        nodes_per_game: most tree nodes a game's pool may hold; pool_bytes_per_game: its bytes (0 = nodes_per_game x 232 + 64 x 704:
        nodes are compact - 40 B + 20 B per legal move, ~212 B on average - include/raz.h).
        leaf_cache_log2: attach a cross-game evaluation cache of 2**leaf_cache_log2 entries (320 B each; include/raz.h
        raz_engine_set_leaf_cache): repeated positions are served from it, bit-identically.  None: no cache.
        leaf_cache_max_discs: cache only positions with at most that many discs (0 = all)."""
        import torch
        self.net = net
        self.backend, self.device = net.backend, net.device
        self.n_games = n_games
        if inner_max == 0 and net.filters >= 128 and int(getattr(config.play, "parallel_search_num", 1) or 1) <= 1:
            # a wide net's forward dwarfs the tree kernel: let a game whose simulations end on finished positions (no net
            # evaluation needed) keep simulating inside the launch until it has a leaf for the batch, instead of idling a
            # batch row (results do not depend on this budget)
            inner_max = 8
        if nodes_per_game is None:
            s = sims_hint or config.play.simulation_num_per_move
            loops = max(1, config.play.thinking_loop)
            share = bool(config.play.share_mtcs_info_in_self_play)
            mirror = share if mirror_updates is None else bool(mirror_updates)
            # every simulation adds at most one node (two with mirror keys); ~62 searched plies
            nodes_per_game = (s * loops * 62 + 128) * (2 if mirror else 1)
            if not pool_bytes_per_game:
                # a pool that is never pruned must hold the whole game whatever its mobility: 320 B per node (14 legal moves
                # on average; a game's average is ~8.5) instead of the 232 B default of pruned pools, capped at the link range
                want = nodes_per_game * WHOLE_GAME_BYTES_PER_NODE + 64 * NODE_MAX_BYTES
                pool_bytes_per_game = min(want, 255 << 20)
                if pool_bytes_per_game < want:
                    # the link range (25-bit offsets in 8-byte units) caps a pool at 256 MB: keep the node count consistent with the
                    # bytes that are there, so that the directory / table are sized for what can exist and an overflow shows up as
                    # "pool full" at the count the constructor states, not deep into a run
                    nodes_per_game = (pool_bytes_per_game - 64 * NODE_MAX_BYTES) // WHOLE_GAME_BYTES_PER_NODE
                    import warnings
                    warnings.warn(f"never-pruned node pool capped at 255 MB per game: {nodes_per_game} nodes instead of the {want // WHOLE_GAME_BYTES_PER_NODE} "
                                  "a whole game at this simulations x thinking_loop could create", RuntimeWarning)
        self.cfg = engine_config_from(config, n_games, seed, nodes_per_game, max_plies, mirror_updates,
                                      record_root_w, phase_profile, single_stream, parts, inner_max,
                                      force_slot_kernel=force_slot_kernel, pool_bytes_per_game=pool_bytes_per_game, fused=fused,
                                      solver_budget=solver_budget, solver_pool_waves=solver_pool_waves, solver_pool_every=solver_pool_every)
        self.fused = bool(fused)
        self.pool_bytes = int(pool_bytes_per_game) or (int(nodes_per_game) * NODE_POOL_BYTES_PER_NODE + 64 * NODE_MAX_BYTES)
        self.slots = int(self.cfg.parallel_search_num) or 1   # simulation slots (leaf-exchange rows) per game
        # most nodes one step can add to a game's pool: k_tree completes <= inner_max (default 2) simulations,
        # each adding a leaf and its mirror; k_tree_par starts <= slots + inner_max simulations, wakes <= slots
        # sleepers (a leaf node each) and finishes <= slots expansions (a mirror node each)
        self.nodes_per_step = 2 * (inner_max or 2) if (self.slots == 1 and not force_slot_kernel) \
            else 3 * self.slots + (inner_max or 2)
        nbytes = self.lib.raz_engine_workspace_bytes(ctypes.byref(self.cfg))
        if nbytes == 0:
            raise ValueError("invalid engine config: " + self.backend.last_error())
        self.workspace_bytes = nbytes
        self._ws = self.backend.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (self._ws.data_ptr() + 255) // 256 * 256
        # the engine's own net scratch: DeviceNet.scratch() may re-allocate its buffer for a later, larger predict call
        need = self.lib.raz_net_scratch_bytes(net.filters, net.value_fc, n_games * self.slots)
        self._scratch = self.backend.empty(need, dtype=torch.uint8, device=self.device) if need else None
        sp, sb = (self._scratch.data_ptr(), need) if need else (None, 0)
        self._h = ctypes.c_void_p()
        self.backend.call("raz_engine_create", ctypes.byref(self.cfg), ctypes.byref(net.c), base, nbytes, sp, sb, ctypes.byref(self._h))
        self.record_root_w = record_root_w
        self.max_plies = max_plies
        self._cache = None
        if leaf_cache_log2:
            self.attach_leaf_cache(leaf_cache_log2, leaf_cache_max_discs)

    def attach_leaf_cache(self, log2_entries, max_discs=0):
        """(Re-)attach a cleared evaluation cache; call again after the net's weights changed."""
        import torch
        need = self.lib.raz_leaf_cache_bytes(log2_entries, self.n_games * self.slots)
        if need == 0:
            raise ValueError("leaf_cache_log2 must be 10..28")
        if self._cache is None or self._cache.numel() < need + 256:
            self._cache = self.backend.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = (self._cache.data_ptr() + 255) // 256 * 256
        self._launch("raz_engine_set_leaf_cache", self._h, base, need, log2_entries, max_discs)

    def leaf_cache_stats(self):
        """{hits, in_batch_duplicates, evaluated, no_room} since the cache was attached (zeros without a cache)."""
        out = (ctypes.c_uint64 * 4)()
        self._launch("raz_engine_leaf_cache_stats", self._h, out)
        return {"hits": out[0], "in_batch_duplicates": out[1], "evaluated": out[2], "no_room": out[3]}

    def solver_stats(self):
        """The end-game solver pool's counters since start() (include/raz.h raz_engine_solver_stats)."""
        out = (ctypes.c_uint64 * 15)()
        self._launch("raz_engine_solver_stats", self._h, out)
        tk_slow, tk_pop, tk_all = (int(x) for x in out[:3])
        out = out[3:]
        self._solver_ticks = {"slow_phase_share_of_worker_time": tk_slow / tk_all if tk_all else None, "pops_share": tk_pop / tk_all if tk_all else None,
                              "ticks_per_wave_iteration": None}
        req, ans, rounds, busy, wave_iters, done, skipped, wave_launches, posted, posted_max, listed, listed_max = (int(x) for x in out)
        self._solver_ticks["ticks_per_wave_iteration"] = tk_all / wave_iters if wave_iters else None
        return {"ticks": self._solver_ticks, "requests_posted": posted, "most_requests_of_one_game": posted_max, "rounds_listed_all_games": listed, "most_rounds_listed_of_one_game": listed_max,
                "solves": req, "answers": ans, "pool_rounds_per_answer": rounds / ans if ans else None,
                "lane_utilisation": busy / (64.0 * wave_iters) if wave_iters else None, "busy_lane_iterations": busy,
                "wave_iterations": wave_iters, "subtrees_finished": done, "subtrees_skipped": skipped, "worker_wave_launches": wave_launches}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.raz_engine_destroy(h)
            self._h = None

    def start(self, first_game_id, sims_per_move, n_active=None):
        sims = np.full(self.n_games, sims_per_move, dtype=np.uint32) if np.isscalar(sims_per_move) \
            else np.ascontiguousarray(sims_per_move, dtype=np.uint32)
        assert sims.size == self.n_games
        self._launch("raz_engine_start", self._h, first_game_id, sims.ctypes.data, self.n_games if n_active is None else n_active)
        self.n_active = self.n_games if n_active is None else n_active

    def next_game(self, first_game_id, sims_per_move, n_active=None):
        """The next game of every slot on the slot's tree (reset_mtcs_info_per_game > 1, include/raz.h)."""
        sims = np.full(self.n_games, sims_per_move, dtype=np.uint32) if np.isscalar(sims_per_move) \
            else np.ascontiguousarray(sims_per_move, dtype=np.uint32)
        assert sims.size == self.n_games
        self._launch("raz_engine_next_game", self._h, first_game_id, sims.ctypes.data, self.n_games if n_active is None else n_active)
        self.n_active = self.n_games if n_active is None else n_active

    def step(self, n=1):
        self._launch("raz_engine_step", self._h, n)

    def set_parts(self, parts):
        self.backend.synchronize(self.device)
        self.backend.call("raz_engine_set_parts", self._h, parts)

    def set_solver_pool_every(self, n):
        """Tree launches per round of the end-game solver's pool (include/raz.h raz_engine_set_solver_pool_every): 1 = every step
        waits for the round, n > 1 = the round runs beside the next n - 1 steps, 0 = the library's default.  Between steps only."""
        self.backend.synchronize(self.device)
        self.backend.call("raz_engine_set_solver_pool_every", self._h, int(n))

    def step_timed(self, n=1):
        """step(n) with HIP events around each kernel; returns (tree_ms, net_ms) summed over n."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._launch("raz_engine_step_timed", self._h, n, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def phase_profile(self):
        """Per-phase shader-clock ticks summed over games (engine created with phase_profile=True)."""
        ptr = self.lib.raz_engine_device_ptr(self._h, 5)
        off = ptr - self._ws.data_ptr()
        self.backend.synchronize(self.device)
        a = self._ws[off:off + self.n_games * 64].cpu().numpy().view(np.uint64).reshape(self.n_games, 8)
        names = ["backup", "controller", "select", "root_noise", "first_arrival_probe", "active_launches",
                 "node_load_wait", "expand_part_of_backup"]
        return {n: int(a[:, i].sum()) for i, n in enumerate(names)}

    def leaf_exchange(self):
        """Views (no copy) of the leaf exchange between the tree kernels and the net as the LAST step left it (include/raz.h
        raz_engine_device_ptr 10-14; the reference's prediction queue, agent/player.py:329-346): {"active" u8 [rows], "own" / "enemy"
        i64 [rows] (as shown to the net), "policy" f32 [rows, 64], "value" f32 [rows]}, rows = n_games x parallel_search_num."""
        import torch
        rows = self.n_games * self.slots
        self.backend.synchronize(self.device)

        def view(which, nbytes, dtype):
            off = self.lib.raz_engine_device_ptr(self._h, which) - self._ws.data_ptr()
            return self._ws[off:off + nbytes].view(dtype)
        return {"active": view(10, rows, torch.uint8), "own": view(11, rows * 8, torch.int64), "enemy": view(12, rows * 8, torch.int64),
                "policy": view(13, rows * 256, torch.float32).view(rows, 64), "value": view(14, rows * 4, torch.float32)}

    def stats(self):
        st = N.RazEngineStats()
        self._launch("raz_engine_stats_sync", self._h, ctypes.byref(st))
        if st.error_flags:
            raise RuntimeError(f"engine error flags {st.error_flags:#x} (1 node pool full, 2 table full, "
                               f"4 records full, 8 path overflow): enlarge nodes_per_game/max_plies")
        return {"finished_games": st.finished_games, "total_sims": st.total_sims, "nn_leaves": st.nn_leaves,
                "selections": st.selections, "max_pool_used": st.max_pool_used, "idle_or_done": st.idle_or_done,
                "max_pool_bytes": st.max_pool_bytes}

    def pool_nearly_full(self, st, steps):
        """True when the fullest running game's pool could overflow within `steps` more steps: a step adds at most
        nodes_per_step nodes of at most 704 B to a game (a pool is full when EITHER its node count reaches nodes_per_game
        or its bytes reach pool_bytes_per_game)."""
        n = self.nodes_per_step * steps + 64
        return st["max_pool_used"] + n > int(self.cfg.nodes_per_game) or st["max_pool_bytes"] + n * NODE_MAX_BYTES > self.pool_bytes

    def set_position(self, slot, black, white, player, sims, enable_resign=True, one_move=True):
        """Arm one move for `slot` on an arbitrary position, keeping the slot's tree (include/raz.h)."""
        self._launch("raz_engine_set_position", self._h, slot, black, white, player, sims, int(enable_resign), int(one_move))

    def set_positions(self, first_slot, black, white, player, sims, enable_resign=True, one_move=True):
        """set_position for len(black) consecutive slots in one launch; black / white: int64 device tensors, player: uint8."""
        import torch
        assert black.is_contiguous() and white.is_contiguous() and player.is_contiguous() and player.dtype == torch.uint8
        self._launch("raz_engine_set_positions", self._h, first_slot, black.numel(), black.data_ptr(), white.data_ptr(), player.data_ptr(), sims,
                     int(enable_resign), int(one_move))

    def stop_thinking(self, slot):
        self._launch("raz_engine_stop_thinking", self._h, slot)

    def adopt_tree(self, slot, player_index):
        self._launch("raz_engine_adopt_tree", self._h, slot, player_index)

    def read_node(self, slot, black, white, next_player=1, owner=0):
        """(found, W f64[64], N u32[64], P f32[64]) of one key of one slot's tree (include/raz.h)."""
        w = np.zeros(64, dtype=np.float64)
        n = np.zeros(64, dtype=np.uint32)
        p = np.zeros(64, dtype=np.float32)
        found = ctypes.c_int(0)
        self._launch("raz_engine_read_node", self._h, slot, black, white, next_player, owner, w.ctypes.data, n.ctypes.data, p.ctypes.data,
                     ctypes.byref(found))
        return bool(found.value), w, n, p

    def set_resign_threshold(self, threshold):
        """config.play.resign_threshold changed (worker/self_play.py:250-260); None = no resignation rule."""
        self.backend.call("raz_engine_set_resign_threshold", self._h, int(threshold is not None),
                          float(threshold if threshold is not None else 0.0))

    def pack_records(self, first_slot=0, n_slots=None, plies=None):
        """The records of slots [first_slot, first_slot + n_slots) cut to `plies` plies (None: the largest n_plies
        among them), as dense DEVICE tensors (uint8 views) a collective can move as they are (include/raz.h
        raz_engine_pack_records): {"headers": [n, plies, 48] u8, "root_n": [n, plies, 64] i32, "summary": [n, 32] u8}."""
        import torch
        n = self.n_games - first_slot if n_slots is None else n_slots
        if plies is None:
            mp = ctypes.c_uint32(0)
            self._launch("raz_engine_records_extent", self._h, first_slot, n, ctypes.byref(mp))
            plies = max(1, mp.value)
        hdr = torch.empty((n, plies, 48), dtype=torch.uint8, device=self.device)
        rn = torch.empty((n, plies, 64), dtype=torch.int32, device=self.device)
        sm = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        self._launch("raz_engine_pack_records", self._h, first_slot, n, plies, hdr.data_ptr(), rn.data_ptr(), sm.data_ptr())
        return {"headers": hdr, "root_n": rn, "summary": sm}

    # ---- continuous batching (include/raz.h raz_engine_harvest) -------------------------------------------------
    def new_outbox(self, first_game_id, n_games):
        """Device arrays that receive finished games in id order (row = game id - first_game_id)."""
        import torch
        mp = self.max_plies
        return {"first": first_game_id, "n": n_games,
                "headers": torch.zeros((n_games, mp, 48), dtype=torch.uint8, device=self.device),
                "root_n": torch.zeros((n_games, mp, 64), dtype=torch.int32, device=self.device),
                "summary": torch.zeros((n_games, 32), dtype=torch.uint8, device=self.device),
                "done": torch.zeros(n_games, dtype=torch.uint8, device=self.device)}

    def harvest(self, outbox, next_game_id, sims_per_move, resign_threshold=None):
        """Move every finished game into `outbox` and restart the freed slots on ids next_game_id, next_game_id + 1, ...
        (len(sims_per_move) of them at most).  resign_threshold: None = the engine's run-time value; else one value per
        new id (None entries / NaN = no resignation rule).  Returns (harvested, restarted, skipped, playing)."""
        sims = np.ascontiguousarray(sims_per_move, dtype=np.uint32)
        thr = None
        if resign_threshold is not None:
            thr = np.array([np.nan if t is None else float(t) for t in resign_threshold], dtype=np.float64)
            assert thr.size == sims.size
        res = N.RazHarvestResult()
        self._launch("raz_engine_harvest", self._h, next_game_id, sims.size, sims.ctypes.data if sims.size else None,
                     thr.ctypes.data if thr is not None and thr.size else None, outbox["first"], outbox["n"],
                     outbox["headers"].data_ptr(), outbox["root_n"].data_ptr(), outbox["summary"].data_ptr(),
                     outbox["done"].data_ptr(), ctypes.byref(res))
        return res.harvested, res.restarted, res.skipped, res.playing

    def play_continuous(self, first_game_id, total_games, sims_of, chunk=64, resign_threshold_of=None, max_steps=100_000_000,
                        on_chunk=None):
        """Play global game ids first_game_id .. first_game_id + total_games - 1 with continuous batching: the batch's
        slots are refilled with the next unplayed id as games finish (worker/self_play.py:95-137: a reference worker
        starts its next game the moment one ends), finished games land in an id-ordered device outbox.
        sims_of(id) -> simulations per move of that game (the reference's per-game-index schedule, self_play.py:145); or an array
        with one entry per id of the call (entry i = id first_game_id + i): what the worker passes - a Python call per id and poll was
        3 M calls per 65 536-id block.
        resign_threshold_of(id) (optional) -> the threshold that game is played under.
        on_chunk(steps, games_done, stats, outbox) (optional) is called after every chunk's harvest (progress reporting; the worker
        ships the finished prefix of the outbox to its file writer from it).
        Returns (outbox, stats): outbox = device tensors in id order (pack/gather them as they are, or
        raw_from_packed(...) on the host); stats adds steps, leaf_slot_occupancy and gc_runs."""
        B = self.n_games
        n0 = min(B, total_games)
        # with slots at every stage of a game only some of them wait for the end-game solver at any time: its pool's round runs beside
        # three tree launches instead of holding every step up (mini.yml as shipped: 22.7 M -> 30.3 M sims/s; a value given at
        # construction - solver_pool_every, or RAZ_SOLVER_POOL_EVERY under RAZ_TUNING=1 - stays)
        solver_on = bool(self.cfg.use_solver_turn or self.cfg.use_solver_turn_in_simulation)
        tuned = solver_on and not ((int(self.cfg.reserved) >> 24) & 0xf)
        if tuned:
            self.set_solver_pool_every(CONTINUOUS_SOLVER_POOL_EVERY)
        import time
        t_begin = time.perf_counter()
        try:
            if not callable(sims_of):
                table = np.ascontiguousarray(sims_of, dtype=np.uint32)
                assert table.size == total_games
                sims_at = lambda lo, n: table[lo - first_game_id: lo - first_game_id + n]
            else:
                sims_at = lambda lo, n: np.array([sims_of(i) for i in range(lo, lo + n)], dtype=np.uint32)
            sims0 = np.ones(B, dtype=np.uint32)
            sims0[:n0] = sims_at(first_game_id, n0)
            if resign_threshold_of is not None:
                self.set_resign_threshold(resign_threshold_of(first_game_id))
            self.start(first_game_id, sims0, n_active=n0)
            if resign_threshold_of is not None and len({resign_threshold_of(first_game_id + i) for i in range(n0)}) > 1:
                raise ValueError("the first batch of ids must share one resign threshold (raz_engine_start takes the engine's run-time value)")
            outbox = self.new_outbox(first_game_id, total_games)
            nxt, done, steps, cap = first_game_id + n0, 0, 0, int(self.cfg.nodes_per_game)
            end = first_game_id + total_games
            self.gc_runs = 0
            host = {"steps_and_stats": 0.0, "harvest": 0.0, "before_the_first_step": time.perf_counter() - t_begin}
            while done < total_games:
                t0 = time.perf_counter()
                self.step(chunk)
                steps += chunk
                st = self.stats()
                if self.pool_nearly_full(st, chunk):
                    self.gc(threshold=min(cap // 4, st["max_pool_used"] // 2))
                    self.gc_runs += 1
                t1 = time.perf_counter()
                k = min(B, end - nxt)
                ids = range(nxt, nxt + k)
                h, r, skipped, playing = self.harvest(outbox, nxt, sims_at(nxt, k),
                                                      [resign_threshold_of(i) for i in ids] if resign_threshold_of else None)
                assert skipped == 0
                nxt += r
                done += h
                host["steps_and_stats"] += t1 - t0
                host["harvest"] += time.perf_counter() - t1
                if on_chunk is not None:
                    on_chunk(steps, done, st, outbox)
                if steps >= max_steps:
                    raise RuntimeError("engine did not finish within max_steps")
            st = self.stats()
            host["whole_call"] = time.perf_counter() - t_begin
            st.update(steps=steps, leaf_slot_occupancy=st["nn_leaves"] / max(1, steps * B * self.slots), gc_runs=self.gc_runs,
                      seconds=host)
        finally:
            if tuned:   # (also when a step raised: the engine may be used again by the caller)
                self.set_solver_pool_every(0)
        return outbox, st

    def gc(self, threshold=0):
        """Prune unreachable nodes in every game whose pool holds >= threshold nodes."""
        self._launch("raz_engine_gc", self._h, threshold)

    def run(self, chunk=64, max_steps=10_000_000, allow_gc=True):
        """Step until every active game has finished.  Returns the final stats.  Pools are pruned
        whenever the fullest one could overflow before the next poll (<= nodes_per_step new nodes per step).
        allow_gc=False: never prune (a tree that the NEXT game of the slot will search again must keep its
        early positions: reset_mtcs_info_per_game > 1); a pool that fills up then raises from stats()."""
        steps = 0
        cap = int(self.cfg.nodes_per_game)
        self.gc_runs = 0
        while True:
            self.step(chunk)
            steps += chunk
            st = self.stats()
            if allow_gc and self.pool_nearly_full(st, chunk):
                self.gc(threshold=min(cap // 4, st["max_pool_used"] // 2))
                self.gc_runs += 1
            if st["finished_games"] >= self.n_active:
                st["steps"] = steps
                return st
            if steps >= max_steps:
                raise RuntimeError("engine did not finish within max_steps")

    def read_raw(self):
        B, MP = self.n_games, self.max_plies
        hdr = np.zeros((B, MP), dtype=PLY_HEADER)
        root_n = np.zeros((B, MP, 64), dtype=np.uint32)
        root_w = np.zeros((B, MP, 64), dtype=np.float64) if self.record_root_w else None
        n_plies = np.zeros(B, dtype=np.uint32)
        status = np.zeros(B, dtype=np.uint8)
        resigned = np.zeros((B, 2), dtype=np.uint8)
        game_id = np.zeros(B, dtype=np.uint32)
        enable_resign = np.zeros(B, dtype=np.uint8)
        fb = np.zeros(B, dtype=np.uint64)
        fw = np.zeros(B, dtype=np.uint64)
        self._launch("raz_engine_read_records", self._h, hdr.ctypes.data, root_n.ctypes.data, root_w.ctypes.data if root_w is not None else None,
                     n_plies.ctypes.data, status.ctypes.data, resigned.ctypes.data, game_id.ctypes.data,
                     enable_resign.ctypes.data, fb.ctypes.data, fw.ctypes.data)
        return dict(headers=hdr, root_n=root_n, root_w=root_w, n_plies=n_plies, status=status, resigned=resigned,
                    game_id=game_id, enable_resign=enable_resign, final_black=fb, final_white=fw)

    def records(self, save_policy_of_tau_1=True, change_tau_turn=None):
        """Per game: (plies, summary) in the same shape oracle.selfplay_game returns."""
        raw = self.read_raw()
        ctt = self.cfg.change_tau_turn if change_tau_turn is None else change_tau_turn
        out = []
        for g in range(self.n_active):
            plies = []
            for i in range(int(raw["n_plies"][g])):
                h = raw["headers"][g, i]
                n = raw["root_n"][g, i].astype(np.float64)
                plies.append({"player": int(h["player"]), "turn": int(h["turn"]), "own": int(h["own"]),
                              "enemy": int(h["enemy"]), "action": int(h["action"]), "has_row": bool(h["has_row"]), "solved": bool(int(h["flags"]) & 1),
                              "sims": int(h["sims"]), "loops": int(h["loops"]), "n": float(h["n"]), "q": float(h["q"]),
                              "root_n": [float(v) for v in n],
                              "root_w": [float(v) for v in raw["root_w"][g, i]] if raw["root_w"] is not None else None,
                              "saved_policy": saved_policy(n, int(h["turn"]), ctt, save_policy_of_tau_1)})
            st = int(raw["status"][g])
            out.append((plies, {"winner": st & 0x0f, "status": st, "plies": len(plies),
                                "game_id": int(raw["game_id"][g]), "enable_resign": int(raw["enable_resign"][g]),
                                "resigned_black": int(raw["resigned"][g, 0]), "resigned_white": int(raw["resigned"][g, 1]),
                                "black": int(raw["final_black"][g]), "white": int(raw["final_white"][g])}))
        return out


MATCH_GAME = np.dtype([("black", "<u8"), ("white", "<u8"), ("player", "u1"), ("best_is_black", "u1"), ("searching", "u1"),
                       ("winner", "u1"), ("blacks", "u1"), ("whites", "u1"), ("n_plies", "u1"), ("flags", "u1"), ("pad", "<u4", (2,))])
MATCH_PLY = np.dtype([("who", "u1"), ("action", "i1"), ("turn", "u1"), ("pad", "u1")])
assert MATCH_GAME.itemsize == 32 and MATCH_PLY.itemsize == 4
MATCH_MAX_PLIES = 64   # include/raz.h RAZ_MATCH_MAX_PLIES


# ---- what DeviceMatch, DeviceLeague and DeviceAnalysis share: the engine hand-off of csrc/raz_handoff.h seen from the host ----------
def _error_text(what, error, rest):
    return (f"{what} error word {error:#x} (1 node pool full, 2 table full, 4 records full, 8 path overflow: a slot's engine error; "
            f"0x100 a slot left the one-move protocol, {rest}")


def _lies_on(t, device):
    """t is a tensor in the memory of `device` (an index the device does not name is not compared)."""
    import torch
    return isinstance(t, torch.Tensor) and t.device.type == device.type and device.index in (None, t.device.index)


def _workspace(given, need, device, what="workspace_bytes"):
    """(tensor, base address): `given`, or the caller's own where it is None, with `need` bytes behind its first 256-byte boundary."""
    import torch
    ws = given if given is not None else torch.zeros(need + 256, dtype=torch.uint8, device=device)
    base = (ws.data_ptr() + 255) // 256 * 256
    if not (_lies_on(ws, device) and ws.dtype == torch.uint8 and ws.is_contiguous() and need and base + need <= ws.data_ptr() + ws.numel()):
        raise ValueError(f"workspace: a contiguous uint8 device tensor with {what} behind its first 256-byte boundary")
    return ws, base


def _positions(who, positions, n, device, leading=(), dtypes="positions: int64, int64, uint8"):
    """The (black, white, player) pointers raz_*_start takes, three None for positions None; `leading` tensors are held to n entries too."""
    import torch
    if positions is not None and len(positions) != 3:
        raise ValueError("positions is (black, white, player)")
    for t in list(leading) + list(positions or ()):
        if not (_lies_on(t, device) and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"{who}.start takes contiguous device tensors of n_games entries (no CPU tensors)")
    if positions is None:
        return None, None, None
    if positions[0].dtype != torch.int64 or positions[1].dtype != torch.int64 or positions[2].dtype != torch.uint8:
        raise ValueError(dtypes)
    return tuple(t.data_ptr() for t in positions)


def _log_arrays(n, log):
    """Host arrays for a log of n games and their addresses: (MATCH_PLY [n, 64], visit counts i32 [n, 64, 64]), or None where not log."""
    if not log:
        return None, None, None, None
    plies, root_n = np.zeros((n, MATCH_MAX_PLIES), dtype=MATCH_PLY), np.zeros((n, MATCH_MAX_PLIES, 64), dtype=np.int32)
    return plies, root_n, plies.ctypes.data, root_n.ctypes.data


def _ply_lists(games, log, log_n, who=int):
    """Per game its plies as dictionaries, from raz_*_read's host arrays."""
    log, log_n = log.reshape(len(games), MATCH_MAX_PLIES), log_n.reshape(len(games), MATCH_MAX_PLIES, 64)
    return [[{"who": who(log[g, i]["who"]), "action": int(log[g, i]["action"]), "root_n": log_n[g, i].copy()} for i in range(int(r["n_plies"]))]
            for g, r in enumerate(games)]


def match_error_text(error):
    return _error_text("match", error, "0x200 a game's log is full): the games it hit ended undecided")


def match_results(games):
    """Per game (ng_win: 1 / 0 / None for a draw, best_is_black, (blacks, whites)) - what EvaluateWorker.play_games returns - from the
    MATCH_GAME records of a finished match."""
    out = []
    for r in games:
        w, bib = int(r["winner"]), bool(r["best_is_black"])
        out.append((int((w == 1) != bib) if w in (1, 2) else None, bib, (int(r["blacks"]), int(r["whites"]))))
    return out


def match_games(games, log, log_n, first_game_id=0):
    """The match ply by ply, in the dictionaries of EvaluateWorker.last_games, from raz_match_read's host arrays."""
    plies = _ply_lists(games, log, log_n, who=lambda side: "ng" if side else "best")
    return [{"game_id": first_game_id + g, "best_is_black": bool(r["best_is_black"]), "plies": plies[g]} for g, r in enumerate(games)]


class DeviceMatch(N.Wrapper):
    """A match of two started engines of the same n_games on the device (include/raz.h raz_match_*): slot g of `best_engine` is the
    best model's player in game g, slot g of `challenger_engine` the challenger's.  The caller steps the engines; turn() hands every
    decided move to the other side's slot where it lies, without a host round trip."""

    def __init__(self, best_engine, challenger_engine, workspace=None):
        """workspace: a uint8 device tensor of at least workspace_bytes + 255 bytes to keep the match in (None: the match's own)."""
        if best_engine.n_games != challenger_engine.n_games:
            raise ValueError("the two engines of a match need the same n_games")
        self.best, self.challenger = best_engine, challenger_engine
        self.backend, self.device, self.n_games = best_engine.backend, best_engine.device, best_engine.n_games
        self.workspace_bytes = self.lib.raz_match_workspace_bytes(self.n_games)
        self._ws, self.workspace_base = _workspace(workspace, self.workspace_bytes, self.device)
        self._h = ctypes.c_void_p()
        self.backend.call("raz_match_create", best_engine._h, challenger_engine._h, self.workspace_base, self.workspace_bytes, ctypes.byref(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.raz_match_destroy(h)
            self._h = None

    def start(self, best_is_black, positions=None, sims_best=None, sims_challenger=None, enable_resign=True):
        """best_is_black: uint8 / bool device tensor [n_games].  positions: None (the initial position, black to move) or
        (black int64, white int64, player uint8) device tensors [n_games], playable positions.  sims_*: simulations a move."""
        import torch
        dtypes = "best_is_black: uint8 / bool; positions: int64, int64, uint8"
        b, w, p = _positions("DeviceMatch", positions, self.n_games, self.device, leading=[best_is_black], dtypes=dtypes)
        if best_is_black.dtype not in (torch.uint8, torch.bool):
            raise ValueError(dtypes)
        if not sims_best:
            raise ValueError("sims_best: simulations a move")
        self._args = [best_is_black] + list(positions or ())   # (kept alive until the launch has run)
        self._launch("raz_match_start", self._h, best_is_black.data_ptr(), b, w, p, int(sims_best), int(sims_challenger or sims_best),
                     int(enable_resign))

    def turn(self):
        self._launch("raz_match_turn", self._h)

    def stats(self, raise_on_error=True):
        """{"live", "searching_best", "searching_challenger", "searching": [best, challenger], "plies", "error"}; raises on the match's
        error word.  Synchronises."""
        st = N.RazMatchStats()
        self._launch("raz_match_stats_sync", self._h, ctypes.byref(st))
        if st.error and raise_on_error:
            raise RuntimeError(match_error_text(st.error))
        return {"live": st.live, "searching_best": st.searching_best, "searching_challenger": st.searching_challenger,
                "searching": [st.searching_best, st.searching_challenger], "plies": st.plies, "error": st.error}

    def read(self, log=True):
        """(MATCH_GAME [n], MATCH_PLY [n, 64] or None, root visit counts i32 [n, 64, 64] or None) on the host."""
        games = np.zeros(self.n_games, dtype=MATCH_GAME)
        plies, root_n, plies_ptr, root_n_ptr = _log_arrays(self.n_games, log)
        self._launch("raz_match_read", self._h, games.ctypes.data, plies_ptr, root_n_ptr)
        return games, plies, root_n

    def results(self):
        return match_results(self.read(log=False)[0])

    def games(self, first_game_id=0):
        return match_games(*self.read(), first_game_id=first_game_id)


LEAGUE_PAIRING = np.dtype([("black_model", "u1"), ("white_model", "u1"), ("pad0", "<u2"), ("black_slot", "<u4"), ("white_slot", "<u4"),
                           ("pad1", "<u4")])
LEAGUE_GAME = np.dtype([("black", "<u8"), ("white", "<u8"), ("player", "u1"), ("black_model", "u1"), ("white_model", "u1"),
                        ("searching", "u1"), ("winner", "u1"), ("blacks", "u1"), ("whites", "u1"), ("n_plies", "u1"), ("flags", "u1"),
                        ("pad8", "u1", (3,)), ("pad", "<u4")])
LEAGUE_PLY = MATCH_PLY   # (`who` is a model index)
LEAGUE_STATS = np.dtype([("live", "<u4"), ("plies", "<u4"), ("error", "<u4"), ("n_models", "<u4"), ("searching", "<u4", (16,)),
                         ("pad", "<u4", (12,))])
assert LEAGUE_PAIRING.itemsize == 16 and LEAGUE_GAME.itemsize == 32 and LEAGUE_PLY.itemsize == 4 and LEAGUE_STATS.itemsize == 128
LEAGUE_MAX_MODELS, LEAGUE_MAX_PLIES = 16, MATCH_MAX_PLIES   # include/raz.h RAZ_LEAGUE_MAX_*
LEAGUE_GAME_NOT_STARTED = 0x40
LEAGUE_ERR_SLOT, LEAGUE_ERR_LOG_FULL, LEAGUE_ERR_PAIRING = 0x100, 0x200, 0x800


def league_error_text(error):
    return _error_text("league", error, "0x200 a game's log is full: the games it hit ended undecided; "
                       "0x800 a pairing was unsound or lost its slot to a lower game index: the game was not started)")


def league_pairings(pairings):
    """LEAGUE_PAIRING records from (black_model, black_slot, white_model, white_slot) tuples."""
    out = np.zeros(len(pairings), dtype=LEAGUE_PAIRING)
    for g, (bm, bs, wm, ws) in enumerate(pairings):
        out[g]["black_model"], out[g]["black_slot"], out[g]["white_model"], out[g]["white_slot"] = bm, bs, wm, ws
    return out


def league_results(games):
    """Per game (winner model or None - a draw, undecided or not started -, black_model, white_model, (blacks, whites)) from the
    LEAGUE_GAME records of a finished league."""
    out = []
    for r in games:
        w, bm, wm = int(r["winner"]), int(r["black_model"]), int(r["white_model"])
        out.append((bm if w == 1 else wm if w == 2 else None, bm, wm, (int(r["blacks"]), int(r["whites"]))))
    return out


def league_games(games, log, log_n, game_ids=None):
    """The league ply by ply, in the shape of match_games with black_model / white_model and `who` a model index, from
    raz_league_read's host arrays.  game_ids: per game (None: the game's index)."""
    plies = _ply_lists(games, log, log_n)
    return [{"game_id": g if game_ids is None else game_ids[g], "black_model": int(r["black_model"]), "white_model": int(r["white_model"]),
             "started": not int(r["flags"]) & LEAGUE_GAME_NOT_STARTED, "plies": plies[g]} for g, r in enumerate(games)]


class DeviceLeague(N.Wrapper):
    """A league of 2..16 started engines, one per model, on the device (include/raz.h raz_league_*): game g names its two models and the
    slot of each model's engine that plays it.  The engines may differ in n_games.  The caller steps the engines; turn() hands every
    decided move to the next mover's slot where it lies, without a host round trip."""

    def __init__(self, engines, workspace=None):
        """workspace: a uint8 device tensor of at least workspace_bytes(n_games) + 255 bytes to keep the league in (None: the league's
        own, sized by every start)."""
        self.engines = list(engines)
        if not 2 <= len(self.engines) <= LEAGUE_MAX_MODELS:
            raise ValueError(f"a league has 2..{LEAGUE_MAX_MODELS} engines, one per model")
        if len({id(e) for e in self.engines}) != len(self.engines):
            raise ValueError("every model of a league needs an engine of its own")
        self.backend, self.device = self.engines[0].backend, self.engines[0].device
        self._given, self._ws, self._h = workspace, None, ctypes.c_void_p()
        self.n_games = 0

    def workspace_bytes(self, n_games):
        slots = (ctypes.c_uint32 * len(self.engines))(*[e.n_games for e in self.engines])
        return int(self.lib.raz_league_workspace_bytes(len(self.engines), slots, int(n_games)))

    def _destroy(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.raz_league_destroy(h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self._destroy()

    def start(self, pairings, positions=None, sims=None, enable_resign=True):
        """pairings: uint8 device tensor [n_games, 16] of LEAGUE_PAIRING records (league_pairings).  positions: None (the initial
        position, black to move) or (black int64, white int64, player uint8) device tensors [n_games], playable positions.
        sims: simulations a move, one number or one per model."""
        import torch
        if not (_lies_on(pairings, self.device) and pairings.is_contiguous() and pairings.dtype == torch.uint8
                and pairings.numel() and pairings.numel() % LEAGUE_PAIRING.itemsize == 0):
            raise ValueError("DeviceLeague.start takes the pairings as a contiguous uint8 device tensor [n_games, 16] (no CPU tensors)")
        n = pairings.numel() // LEAGUE_PAIRING.itemsize
        b, w, p = _positions("DeviceLeague", positions, n, self.device)
        if not sims:
            raise ValueError("sims: simulations a move, one number or one per model")
        per_model = [int(sims)] * len(self.engines) if np.isscalar(sims) else [int(s) for s in sims]
        if len(per_model) != len(self.engines):
            raise ValueError("sims: one entry per model")
        if n != self.n_games or not self._h:
            self._destroy()
            need = self.workspace_bytes(n)
            ws, base = _workspace(self._given, need, self.device, what="workspace_bytes(n_games)")
            handles = (ctypes.c_void_p * len(self.engines))(*[e._h.value for e in self.engines])
            self.backend.call("raz_league_create", handles, len(self.engines), base, need, n, ctypes.byref(self._h))
            self._ws, self.workspace_base, self.n_games = ws, base, n
        self._args = [pairings] + list(positions or ())   # (kept alive until the launches have run)
        self._launch("raz_league_start", self._h, pairings.data_ptr(), b, w, p, (ctypes.c_uint32 * len(per_model))(*per_model),
                     int(enable_resign))

    def _started(self, what):
        if not self._h:
            raise RuntimeError(f"DeviceLeague.{what}: call start first (raz_league_start)")

    def turn(self):
        self._started("turn")
        self._launch("raz_league_turn", self._h)

    def stats(self, raise_on_error=True):
        """{"live", "plies", "error", "n_models", "searching": [per model]}; raises on the league's error word.  Synchronises."""
        self._started("stats")
        st = N.RazLeagueStats()
        self._launch("raz_league_stats_sync", self._h, ctypes.byref(st))
        if st.error and raise_on_error:
            raise RuntimeError(league_error_text(st.error))
        return {"live": st.live, "plies": st.plies, "error": st.error, "n_models": st.n_models,
                "searching": [int(x) for x in st.searching[:len(self.engines)]]}

    def read(self, log=True):
        """(LEAGUE_GAME [n], LEAGUE_PAIRING [n], LEAGUE_PLY [n, 64] or None, root visit counts i32 [n, 64, 64] or None) on the host."""
        self._started("read")
        games, pairings = np.zeros(self.n_games, dtype=LEAGUE_GAME), np.zeros(self.n_games, dtype=LEAGUE_PAIRING)
        plies, root_n, plies_ptr, root_n_ptr = _log_arrays(self.n_games, log)
        self._launch("raz_league_read", self._h, games.ctypes.data, pairings.ctypes.data, plies_ptr, root_n_ptr)
        return games, pairings, plies, root_n

    def results(self):
        return league_results(self.read(log=False)[0])

    def games(self, game_ids=None):
        g, _, plies, root_n = self.read()
        return league_games(g, plies, root_n, game_ids=game_ids)


ANALYSIS_GAME = np.dtype([("positions", "<u4"), ("ended", "u1"), ("winner", "u1"), ("blacks", "u1"), ("whites", "u1"), ("errors", "<u4"),
                          ("searched", "<u4")])
ANALYSIS_POS = np.dtype([("black", "<u8"), ("white", "<u8"), ("player", "u1"), ("state", "u1"), ("moves_made", "u1"), ("played", "i1"),
                         ("pad", "<u4")])
ANALYSIS_TOP = 8         # include/raz.h RAZ_ANALYSIS_TOP
ANALYSIS_MAX_MOVES = 127
ANALYSIS_EVAL = np.dtype([("state", "u1"), ("action", "i1"), ("n_top", "u1"), ("played", "i1"), ("sum_n", "<u4"),
                          ("top_q", "<f8", (ANALYSIS_TOP,)), ("top_n", "<u4", (ANALYSIS_TOP,)), ("top_square", "i1", (ANALYSIS_TOP,)),
                          ("played_q", "<f8"), ("played_n", "<u4"), ("flags", "<u4")])
assert ANALYSIS_GAME.itemsize == 16 and ANALYSIS_POS.itemsize == 24 and ANALYSIS_EVAL.itemsize == 128
ANALYSIS_ENTRY_PASS, ANALYSIS_ENTRY_END = -1, -2                                     # list entries beside the moves 0..63
POS_NONE, POS_SEARCH, POS_PASS_ENTRY, POS_OVER = 0, 1, 2, 3                           # RAZ_ANALYSIS_POS_*
EVAL_NONE, EVAL_PENDING, EVAL_SEARCHED, EVAL_SOLVED, EVAL_ERROR = 0, 1, 2, 3, 4      # RAZ_ANALYSIS_EVAL_*
ANALYSIS_ERR_SLOT, ANALYSIS_ERR_BAD_CODE = 0x100, 0x400


def analysis_error_text(error):
    return _error_text("analysis", error, "0x400 a list entry outside -2..63)")


class DeviceAnalysis(N.Wrapper):
    """The retrograde analysis of whole games on one started engine created with record_root_w (include/raz.h raz_analysis_*):
    position j of game g - the position after j list entries - is searched by slot first_slot + g * (max_moves + 1) + j.  The caller
    steps the engine; collect() reduces every decided search where it lies, without a host round trip."""

    def __init__(self, engine, first_slot=0, workspace=None):
        """workspace: a uint8 device tensor to keep the analysis in (None: the analysis's own, sized by every start)."""
        self.engine, self.backend, self.device, self.first_slot = engine, engine.backend, engine.device, int(first_slot)
        self._given, self._ws, self._h = workspace, None, ctypes.c_void_p()
        self.n_games = self.max_moves = 0

    def _destroy(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.raz_analysis_destroy(h)
            self._h = ctypes.c_void_p()

    __del__ = _destroy

    def start(self, moves, positions=None, sims=None):
        """moves: int8 device tensor [n_games, max_moves] (0..63 a move, -1 a pass entry, -2 the end of the list).  positions: None
        (the initial position, black to move) or (black int64, white int64, player uint8) device tensors [n_games].  sims:
        simulations a move."""
        import torch
        if not (_lies_on(moves, self.device) and moves.is_contiguous() and moves.dtype == torch.int8 and moves.dim() == 2):
            raise ValueError("DeviceAnalysis.start takes a contiguous int8 device tensor [n_games, max_moves] (no CPU tensors)")
        n, mm = int(moves.shape[0]), int(moves.shape[1])
        b, w, p = _positions("DeviceAnalysis", positions, n, self.device)
        if not sims:
            raise ValueError("sims: simulations a move")
        if (n, mm) != (self.n_games, self.max_moves) or not self._h:
            self._destroy()
            need = self.lib.raz_analysis_workspace_bytes(n, mm)
            if not need:
                raise ValueError("DeviceAnalysis.start: " + self.backend.last_error())
            own = self._ws if self._ws is not None and self._ws.numel() >= need + 256 else None   # (its own, kept while it is large enough)
            ws, base = _workspace(self._given if self._given is not None else own, need, self.device)
            self._ws, self.workspace_base, self.workspace_bytes = ws, base, need
            self.backend.call("raz_analysis_create", self.engine._h, self.first_slot, base, need, n, mm, ctypes.byref(self._h))
            self.n_games, self.max_moves = n, mm
        self._args = [moves] + list(positions or ())   # (kept alive until the launch has run)
        self._launch("raz_analysis_start", self._h, b, w, p, moves.data_ptr(), int(sims))

    def collect(self):
        self._launch("raz_analysis_collect", self._h)

    def stats(self, raise_on_error=True):
        """{"games", "positions", "armed", "pending", "searched", "solved", "failed", "error"}; raises on the error word.  Synchronises."""
        st = N.RazAnalysisStats()
        self._launch("raz_analysis_stats_sync", self._h, ctypes.byref(st))
        if st.error and raise_on_error:
            raise RuntimeError(analysis_error_text(st.error))
        return {k: getattr(st, k) for k, _ in N.RazAnalysisStats._fields_}

    def results(self):
        """(ANALYSIS_GAME [n], ANALYSIS_POS [n, max_moves + 1], ANALYSIS_EVAL [n, max_moves + 1]) on the host.  Synchronises."""
        n, P = self.n_games, self.max_moves + 1
        games, pos, evals = np.zeros(n, dtype=ANALYSIS_GAME), np.zeros((n, P), dtype=ANALYSIS_POS), np.zeros((n, P), dtype=ANALYSIS_EVAL)
        self._launch("raz_analysis_read", self._h, games.ctypes.data, pos.ctypes.data, evals.ctypes.data)
        return games, pos, evals


GAME_SUMMARY = np.dtype([("final_black", "<u8"), ("final_white", "<u8"), ("game_id", "<u4"), ("n_plies", "<u4"),
                         ("status", "u1"), ("resigned_black", "u1"), ("resigned_white", "u1"), ("enable_resign", "u1"),
                         ("sims", "<u4")])
assert GAME_SUMMARY.itemsize == 32


def raw_from_packed(headers_u8, root_n_i32, summary_u8):
    """Host numpy views of packed record arrays (SelfPlayEngine.pack_records, possibly concatenated over ranks)
    in the dict shape SelfPlayEngine.read_raw returns (minus root_w)."""
    hdr = np.ascontiguousarray(headers_u8).view(PLY_HEADER).reshape(headers_u8.shape[0], headers_u8.shape[1])
    sm = np.ascontiguousarray(summary_u8).view(GAME_SUMMARY).reshape(-1)
    return dict(headers=hdr, root_n=np.ascontiguousarray(root_n_i32).view(np.uint32), root_w=None,
                **bookkeeping_from_summaries(sm), sims=sm["sims"].copy(),
                final_black=sm["final_black"].copy(), final_white=sm["final_white"].copy())


def bookkeeping_from_summaries(summary_u8):
    """What the worker's resignation bookkeeping (BatchedSelfPlayWorker.bookkeep_raw) reads of finished games, from their 32-byte
    summaries alone ([n, 32] u8, or GAME_SUMMARY records): raw_from_packed's n_plies, status, resigned, game_id, enable_resign."""
    sm = np.ascontiguousarray(summary_u8).view(GAME_SUMMARY).reshape(-1)
    return dict(n_plies=sm["n_plies"].copy(), status=sm["status"].copy(),
                resigned=np.stack([sm["resigned_black"], sm["resigned_white"]], axis=1),
                game_id=sm["game_id"].copy(), enable_resign=sm["enable_resign"].copy())


def packed_to_host(pk):
    """Packed DEVICE records (SelfPlayEngine.pack_records, an outbox of play_continuous, or a cut of one: tensors under "headers",
    "root_n", "summary") copied to the host in read_raw's shape."""
    return raw_from_packed(*(pk[k].cpu().numpy() for k in ("headers", "root_n", "summary")))


def saved_policy(root_n, turn, change_tau_turn, save_policy_of_tau_1):
    """The policy stored with a training row (agent/player.py:132, 366-385), from the root visit
    counts, with the reference's own numpy expressions."""
    n = np.asarray(root_n, dtype=np.float64)
    if save_policy_of_tau_1 or turn < change_tau_turn:
        return list(n / np.sum(n))
    ret = np.zeros(64)
    ret[int(np.argmax(n))] = 1
    return list(ret)
