// raz_match.h — evaluation matches on the device: the hand-off between two engines (include/raz.h raz_match_*).
//
// Reference objects this replaces, per game: EvaluateWorker.play_game's loop state (worker/evaluate.py:66-96) - one ReversiEnv,
// the colour draw, and the `env.step(player.action(own, enemy))` hand-off between two ReversiPlayer objects.  The players are
// slot g of two engines in one-move mode (raz_engine_set_position's semantics); after a slot's search finalize_move
// (raz_engine_core.h) has left in it the position after the move IN THE MOVER'S FRAME (root_black = the mover's discs,
// player 1 = the mover moves again: the opponent passed), the status in that frame and the ply's record.  k_match_turn reads
// that, keeps the game's real board in absolute colours, and arms the next mover's slot where the state lies.
//
// Part of raz_engine.hip's translation unit (it needs struct raz_engine and arm_slot); board logic is raz_bitboard.h's.
// One thread per game; plain vector stores, no floating point, integer atomics for the five counters only.
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

inline size_t match_up(size_t x) { return (x + 255) / 256 * 256; }
// Carve the workspace; with base == nullptr only the total size is computed.
inline size_t match_carve(uint32_t n, unsigned char* base, raz_match_dev* M) {
    size_t off = 0;
    auto take = [&](size_t bytes) -> unsigned char* {
        unsigned char* p = base ? base + off : nullptr;
        off = match_up(off + bytes);
        return p;
    };
    raz_match_dev d;
    d.n = n;
    d.counters = (uint32_t*)take(sizeof(raz_match_stats));
    d.game = (raz_match_game*)take((size_t)n * sizeof(raz_match_game));
    d.log = (raz_match_ply*)take((size_t)n * RAZ_MATCH_MAX_PLIES * sizeof(raz_match_ply));
    d.log_n = (uint32_t*)take((size_t)n * RAZ_MATCH_MAX_PLIES * 64 * 4);
    if (M) *M = d;
    return off;
}

// The side (0 the best model, 1 the challenger) that moves for colour `player` in a game.
__device__ __forceinline__ uint32_t match_side(uint32_t player, uint32_t best_is_black) {
    return ((player == RAZ_PLAYER_BLACK) == (best_is_black != 0)) ? 0u : 1u;
}

// Ask `side`'s slot g for the move of colour `player` on the real board: the mover's own discs are "black" inside its tree,
// whatever its colour in the game (agent/player.py:95), so the slot is armed with player 1.
__device__ __forceinline__ void match_arm(const raz_engine_dev& Eb, const raz_engine_dev& Ec, uint32_t side, uint32_t g,
                                          unsigned long long black, unsigned long long white, uint32_t player, uint32_t sims_b,
                                          uint32_t sims_c, uint32_t enable_resign) {
    const unsigned long long own = player == RAZ_PLAYER_BLACK ? black : white, enemy = player == RAZ_PLAYER_BLACK ? white : black;
    if (side == 0)
        arm_slot(Eb, g, own, enemy, RAZ_PLAYER_BLACK, sims_b, enable_resign, 1u);
    else
        arm_slot(Ec, g, own, enemy, RAZ_PLAYER_BLACK, sims_c, enable_resign, 1u);
}

// Every game on its start position, the log empty, the side to move armed.  (The counters and the log headers were cleared by
// the memset ahead of this launch.)
__global__ __launch_bounds__(256) void k_match_start(raz_match_dev M, raz_engine_dev Eb, raz_engine_dev Ec, const uint8_t* best_is_black,
                                                     const unsigned long long* black, const unsigned long long* white,
                                                     const uint8_t* player, uint32_t sims_b, uint32_t sims_c, uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M.n) return;
    raz_match_game mg;
    mg.black = black ? black[g] : RAZ_INIT_BLACK;
    mg.white = black ? white[g] : RAZ_INIT_WHITE;
    mg.player = black ? player[g] : (uint8_t)RAZ_PLAYER_BLACK;
    mg.best_is_black = best_is_black[g] ? 1 : 0;
    const uint32_t side = match_side(mg.player, mg.best_is_black);
    mg.searching = (uint8_t)(1u + side);
    mg.winner = mg.blacks = mg.whites = mg.n_plies = mg.flags = 0;
    mg.pad[0] = mg.pad[1] = 0;
    M.game[g] = mg;
    match_arm(Eb, Ec, side, g, mg.black, mg.white, mg.player, sims_b, sims_c, enable_resign);
    atomicAdd(&M.counters[kMatchLive], 1u);
    atomicAdd(&M.counters[kMatchSearching + side], 1u);
}

struct alignas(16) raz_match_q4 {
    uint32_t x, y, z, w;
};

// The hand-off.  Thread g looks at game g's searching slot and, where that slot has decided, does for the game what
// `env.step(action)` and the next `player.action(own, enemy)` call do in the reference's loop.
__global__ __launch_bounds__(256) void k_match_turn(raz_match_dev M, raz_engine_dev Eb, raz_engine_dev Ec, uint32_t sims_b, uint32_t sims_c,
                                                    uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M.n) return;
    raz_match_game mg = M.game[g];
    if (mg.searching == 0) return;   // the game has ended
    const uint32_t side = mg.searching - 1u;
    const raz_game& G = side ? Ec.game[g] : Eb.game[g];
    const uint32_t phase = G.phase, slot_error = G.error, slot_plies = G.n_plies;
    uint32_t err = slot_error;
    if (!err) {
        if (phase != RAZ_PHASE_IDLE && phase != RAZ_PHASE_DONE) return;   // still searching: no game waits for another
        if (phase == RAZ_PHASE_DONE || slot_plies != 1u) err = RAZ_MATCH_ERR_SLOT;
        else if (mg.n_plies >= RAZ_MATCH_MAX_PLIES) err = RAZ_MATCH_ERR_LOG_FULL;
    }
    if (err) {   // the game ends here, undecided, and the match says why
        atomicOr(&M.counters[kMatchError], err);
        atomicSub(&M.counters[kMatchLive], 1u);
        atomicSub(&M.counters[kMatchSearching + side], 1u);
        mg.searching = 0;
        M.game[g] = mg;
        return;
    }
    // the ply: slot g's record 0 (one-move mode records every move there)
    const uint32_t mp = side ? Ec.max_plies : Eb.max_plies;
    const raz_ply_header* rec = side ? Ec.rec : Eb.rec;
    const uint32_t* rec_n = side ? Ec.rec_n : Eb.rec_n;
    const size_t ri = (size_t)g * mp, li = (size_t)g * RAZ_MATCH_MAX_PLIES + mg.n_plies;
    raz_match_ply ply;
    ply.who = (uint8_t)side;
    ply.action = rec[ri].action;
    ply.turn = rec[ri].turn;
    ply.pad = 0;
    M.log[li] = ply;
    const raz_match_q4* src = (const raz_match_q4*)(rec_n + ri * 64);
    raz_match_q4* dst = (raz_match_q4*)(M.log_n + li * 64);
    for (int i = 0; i < 16; ++i) dst[i] = src[i];
    mg.n_plies += 1;
    atomicAdd(&M.counters[kMatchPlies], 1u);
    // the slot's board and status, from the mover's frame ("black" = the mover) to absolute colours
    const uint32_t mover = mg.player, other = 3u - mover;
    const unsigned long long sb = G.root_black, sw = G.root_white;
    const uint32_t status = G.status;
    mg.black = mover == RAZ_PLAYER_BLACK ? sb : sw;
    mg.white = mover == RAZ_PLAYER_BLACK ? sw : sb;
    mg.player = (uint8_t)(G.player == RAZ_PLAYER_BLACK ? mover : other);
    if (status) {
        const uint32_t w = status & RAZ_STATUS_WINNER_MASK;
        mg.winner = (uint8_t)(w == RAZ_WIN_BLACK ? mover : (w == RAZ_WIN_WHITE ? other : w));
        mg.flags = (uint8_t)(status & ~(uint32_t)RAZ_STATUS_WINNER_MASK);
        mg.blacks = (uint8_t)bb_popcount(mg.black);
        mg.whites = (uint8_t)bb_popcount(mg.white);
        mg.searching = 0;
        atomicSub(&M.counters[kMatchLive], 1u);
        atomicSub(&M.counters[kMatchSearching + side], 1u);
    } else {
        const uint32_t next = match_side(mg.player, mg.best_is_black);
        match_arm(Eb, Ec, next, g, mg.black, mg.white, mg.player, sims_b, sims_c, enable_resign);
        if (next != side) {
            mg.searching = (uint8_t)(1u + next);
            atomicSub(&M.counters[kMatchSearching + side], 1u);
            atomicAdd(&M.counters[kMatchSearching + next], 1u);
        }
    }
    M.game[g] = mg;
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
    if ((uintptr_t)d_workspace % 256) return raz_fail(RAZ_EINVAL, "raz_match_create: workspace must be 256-byte aligned");
    if (workspace_bytes < match_carve(best_engine->dev.B, nullptr, nullptr))
        return raz_fail(RAZ_EINVAL, "raz_match_create: workspace smaller than raz_match_workspace_bytes()");
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
    if ((d_black != nullptr) != (d_white != nullptr) || (d_black != nullptr) != (d_player != nullptr))
        return raz_fail(RAZ_EINVAL, "raz_match_start: d_black, d_white and d_player go together, all or none");
    if ((uintptr_t)d_black % 8 || (uintptr_t)d_white % 8) return raz_fail(RAZ_EINVAL, "raz_match_start: d_black / d_white must be 8-byte aligned");
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
    if (log) RAZ_HIP_TRY(hipMemcpyAsync(log, d.log, n * RAZ_MATCH_MAX_PLIES * sizeof(raz_match_ply), hipMemcpyDeviceToHost, s), "raz_match_read: log");
    if (log_root_n)
        RAZ_HIP_TRY(hipMemcpyAsync(log_root_n, d.log_n, n * RAZ_MATCH_MAX_PLIES * 64 * 4, hipMemcpyDeviceToHost, s), "raz_match_read: visit counts");
    RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_match_read: sync");
    return RAZ_OK;
}
