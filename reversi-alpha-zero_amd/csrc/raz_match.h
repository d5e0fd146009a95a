// raz_match.h — evaluation matches on the device: the hand-off between two engines (include/raz.h raz_match_*).
//
// Reference objects this replaces, per game: EvaluateWorker.play_game's loop state (worker/evaluate.py:66-96) - one ReversiEnv,
// the colour draw, and the `env.step(player.action(own, enemy))` hand-off between two ReversiPlayer objects.  The players are
// slot g of two engines; match_ctx makes seats of them, and start_game / turn_game (raz_handoff.h) keep the game's real board in
// absolute colours and arm the next mover's slot where the state lies.
//
// Part of raz_engine.hip's translation unit, behind raz_handoff.h.  One thread per game; plain vector stores, no floating point,
// integer atomics for the five counters only.
#pragma once

namespace {

enum { kMatchLive = 0, kMatchSearching = 1 /* + side */, kMatchPlies = 3, kMatchError = 4 };

struct raz_match_dev {
    uint32_t n;
    uint32_t* counters;       // raz_match_stats
    raz_match_game* game;     // [n]
    raz_match_ply* log;       // [n][RAZ_MATCH_MAX_PLIES]
    uint32_t* log_n;          // [n][RAZ_MATCH_MAX_PLIES][64]
};
static_assert(sizeof(raz_match_game) == 32 && sizeof(raz_match_ply) == 4 && sizeof(raz_match_stats) == 32, "raz_match layouts");

inline size_t match_carve(uint32_t n, unsigned char* base, raz_match_dev* M) {
    carver ws{base, 0};
    raz_match_dev d;
    d.n = n;
    d.counters = (uint32_t*)ws.take(sizeof(raz_match_stats));
    d.game = (raz_match_game*)ws.take((size_t)n * sizeof(raz_match_game));
    d.log = (raz_match_ply*)ws.take((size_t)n * RAZ_MATCH_MAX_PLIES * sizeof(raz_match_ply));
    d.log_n = (uint32_t*)ws.take((size_t)n * RAZ_MATCH_MAX_PLIES * 64 * 4);
    if (M) *M = d;
    return ws.off;
}

// The side (0 the best model, 1 the challenger) that moves for colour `player` in a game.
__device__ __forceinline__ uint32_t match_side(uint32_t player, uint32_t best_is_black) {
    return ((player == RAZ_PLAYER_BLACK) == (best_is_black != 0)) ? 0u : 1u;
}

// The match's seats: slot g of the two engines, which stay kernel arguments (a match reads no descriptor from HBM).
struct match_ctx {
    const raz_match_dev& D;
    const raz_engine_dev &Eb, &Ec;
    uint32_t sims_b, sims_c, enable_resign;
    enum { live = kMatchLive, plies = kMatchPlies, error = kMatchError, searching = kMatchSearching };
    __device__ __forceinline__ handoff_seat seat(uint32_t g, const raz_match_game& mg, uint32_t colour) const {
        const uint32_t side = match_side(colour, mg.best_is_black);
        return handoff_seat{side ? Ec : Eb, g, side, side ? sims_c : sims_b};
    }
    __device__ __forceinline__ uint32_t code(const raz_match_game& mg, uint32_t colour) const { return 1u + match_side(colour, mg.best_is_black); }
};

// Every game on its start position, the log empty, the side to move armed.  (The counters and the log headers were cleared by
// the memset ahead of this launch.)
__global__ __launch_bounds__(256) void k_match_start(raz_match_dev M, raz_engine_dev Eb, raz_engine_dev Ec, const uint8_t* best_is_black,
                                                     const unsigned long long* black, const unsigned long long* white, const uint8_t* player,
                                                     uint32_t sims_b, uint32_t sims_c, uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M.n) return;
    raz_match_game mg;
    init_game(mg, g, black, white, player);
    mg.best_is_black = best_is_black[g] ? 1 : 0;
    mg.pad[0] = mg.pad[1] = 0;
    start_game(match_ctx{M, Eb, Ec, sims_b, sims_c, enable_resign}, g, mg);
}

// The hand-off (raz_handoff.h turn_game) for every game that has not ended.
__global__ __launch_bounds__(256) void k_match_turn(raz_match_dev M, raz_engine_dev Eb, raz_engine_dev Ec, uint32_t sims_b, uint32_t sims_c,
                                                    uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M.n) return;
    raz_match_game mg = M.game[g];
    if (mg.searching == 0) return;   // the game has ended
    turn_game(match_ctx{M, Eb, Ec, sims_b, sims_c, enable_resign}, g, mg);
}

}  // namespace

struct raz_match {
    raz_engine *best, *challenger;
    raz_match_dev dev;
    uint32_t sims[2], enable_resign;
    bool started;
};

extern "C" size_t raz_match_workspace_bytes(uint32_t n_games) {
    if (n_games == 0) {
        raz_fail(RAZ_EINVAL, "raz_match_workspace_bytes: n_games must be > 0");
        return 0;
    }
    return match_carve(n_games, nullptr, nullptr);
}

extern "C" int raz_match_create(raz_engine* best_engine, raz_engine* challenger_engine, void* d_workspace, size_t workspace_bytes,
                                raz_match** out) {
    if (!best_engine || !challenger_engine || !d_workspace || !out) return raz_fail(RAZ_EINVAL, "raz_match_create: NULL argument");
    if (best_engine == challenger_engine) return raz_fail(RAZ_EINVAL, "raz_match_create: the two sides need an engine each");
    if (best_engine->dev.B != challenger_engine->dev.B) return raz_fail(RAZ_EINVAL, "raz_match_create: the engines differ in n_games");
    if (!best_engine->started || !challenger_engine->started)
        return raz_fail(RAZ_ESTATE, "raz_match_create: call raz_engine_start on both engines first");
    const size_t need = match_carve(best_engine->dev.B, nullptr, nullptr);
    if (int rc = handoff_check_workspace("raz_match_create", "raz_match_workspace_bytes()", d_workspace, workspace_bytes, need)) return rc;
    raz_match* m = new (std::nothrow) raz_match();
    if (!m) return raz_fail(RAZ_ENOMEM, "raz_match_create: out of host memory");
    m->best = best_engine;
    m->challenger = challenger_engine;
    match_carve(best_engine->dev.B, (unsigned char*)d_workspace, &m->dev);
    m->started = false;
    *out = m;
    return RAZ_OK;
}

extern "C" void raz_match_destroy(raz_match* m) { delete m; }

extern "C" int raz_match_start(raz_match* m, const uint8_t* d_best_is_black, const uint64_t* d_black, const uint64_t* d_white,
                               const uint8_t* d_player, uint32_t sims_best, uint32_t sims_challenger, int enable_resign,
                               raz_stream_t stream) {
    if (!m || !d_best_is_black) return raz_fail(RAZ_EINVAL, "raz_match_start: NULL argument");
    if (int rc = handoff_check_positions("raz_match_start", d_black, d_white, d_player)) return rc;
    if (sims_best == 0 || sims_challenger == 0) return raz_fail(RAZ_EINVAL, "raz_match_start: sims must be > 0");
    if (!m->best->started || !m->challenger->started) return raz_fail(RAZ_ESTATE, "raz_match_start: an engine is not started");
    hipStream_t s = (hipStream_t)stream;
    const raz_match_dev& d = m->dev;
    // the counters, the games and the log's headers (the visit counts of a ply are written with its header)
    RAZ_HIP_TRY(hipMemsetAsync(d.counters, 0, (size_t)((unsigned char*)d.log_n - (unsigned char*)d.counters), s), "raz_match_start: clear");
    m->sims[0] = sims_best;
    m->sims[1] = sims_challenger;
    m->enable_resign = enable_resign != 0;
    hipLaunchKernelGGL(k_match_start, dim3((d.n + 255) / 256), dim3(256), 0, s, d, m->best->dev, m->challenger->dev, d_best_is_black,
                       (const unsigned long long*)d_black, (const unsigned long long*)d_white, d_player, sims_best, sims_challenger,
                       m->enable_resign);
    int rc = raz_check_launch("raz_match_start");
    m->started = rc == RAZ_OK;
    return rc;
}

extern "C" int raz_match_turn(raz_match* m, raz_stream_t stream) {
    if (!m) return raz_fail(RAZ_EINVAL, "raz_match_turn: NULL match");
    if (!m->started) return raz_fail(RAZ_ESTATE, "raz_match_turn: call raz_match_start first");
    const raz_match_dev& d = m->dev;
    hipLaunchKernelGGL(k_match_turn, dim3((d.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, m->best->dev, m->challenger->dev,
                       m->sims[0], m->sims[1], m->enable_resign);
    return raz_check_launch("raz_match_turn");
}

extern "C" int raz_match_stats_sync(raz_match* m, raz_match_stats* out, raz_stream_t stream) {
    if (!m || !out) return raz_fail(RAZ_EINVAL, "raz_match_stats_sync: NULL argument");
    if (!m->started) return raz_fail(RAZ_ESTATE, "raz_match_stats_sync: call raz_match_start first");
    RAZ_HIP_TRY(hipMemcpyAsync(out, m->dev.counters, sizeof *out, hipMemcpyDeviceToHost, (hipStream_t)stream), "raz_match_stats_sync: copy");
    RAZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "raz_match_stats_sync: sync");
    return RAZ_OK;
}

extern "C" int raz_match_read(raz_match* m, raz_match_game* games, raz_match_ply* log, uint32_t* log_root_n, raz_stream_t stream) {
    if (!m) return raz_fail(RAZ_EINVAL, "raz_match_read: NULL match");
    if (!m->started) return raz_fail(RAZ_ESTATE, "raz_match_read: call raz_match_start first");
    hipStream_t s = (hipStream_t)stream;
    const raz_match_dev& d = m->dev;
    const size_t n = d.n;
    if (games) RAZ_HIP_TRY(hipMemcpyAsync(games, d.game, n * sizeof(raz_match_game), hipMemcpyDeviceToHost, s), "raz_match_read: games");
    if (int rc = handoff_read_log("raz_match_read", n, log, d.log, log_root_n, d.log_n, s)) return rc;
    RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_match_read: sync");
    return RAZ_OK;
}
