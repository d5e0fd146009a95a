// raz_analysis.h — retrograde analysis of whole games on the device (include/raz.h raz_analysis_*).
//
// Reference objects this replaces, per game: NBoardEngine.set_game's walk (play_game/nboard.py:96-103 - env.update, then env.step for
// every entry that is not a pass entry) over one ReversiEnv (env/reversi_env.py:42-104), and - for the command the reference leaves
// as `pass` (nboard.py:321-330) - one ReversiPlayer.action + ask_thought_about per position of that walk.  Position (g, j), the
// position after j list entries, is searched by engine slot first_slot + g * P + j in one-move mode (raz_engine_set_position's
// semantics); finalize_move (raz_engine_core.h) leaves the root's visit counts and value sums by square in the slot's record 0, and
// k_analysis_collect reduces them to the few numbers a caller reports.
//
// Entries after the game is over are IGNORED: the reference would go on calling env.step on a finished env (moving discs of a game
// that has a winner); that is not reproduced.
//
// Part of raz_engine.hip's translation unit, behind raz_handoff.h (the decided-slot rule, the carve, the host checks); board logic is
// raz_bitboard.h's, the wave reductions are raz_engine_core.h's.  Plain vector stores, no scratch, atomics for the stats block only.
#pragma once

namespace {

enum { kAnaGames = 0, kAnaPositions = 1, kAnaArmed = 2, kAnaPending = 3, kAnaSearched = 4, kAnaSolved = 5, kAnaFailed = 6, kAnaError = 7 };
enum { kAnaWavesPerBlock = 4 };

struct raz_analysis_dev {
    uint32_t n, max_moves, P, first_slot;
    uint32_t* counters;        // raz_analysis_stats
    raz_analysis_game* game;   // [n]
    raz_analysis_pos* pos;     // [n][P]
    raz_analysis_eval* eval;   // [n][P]
};
static_assert(sizeof(raz_analysis_stats) == 32 && sizeof(raz_analysis_game) == 16 && sizeof(raz_analysis_pos) == 24 &&
                  sizeof(raz_analysis_eval) == 128, "raz_analysis layouts");

inline size_t analysis_carve(uint32_t n, uint32_t max_moves, uint32_t first_slot, unsigned char* base, raz_analysis_dev* A) {
    carver ws{base, 0};
    raz_analysis_dev d;
    d.n = n;
    d.max_moves = max_moves;
    d.P = max_moves + 1;
    d.first_slot = first_slot;
    const size_t np = (size_t)n * d.P;
    d.counters = (uint32_t*)ws.take(sizeof(raz_analysis_stats));
    d.game = (raz_analysis_game*)ws.take((size_t)n * sizeof(raz_analysis_game));
    d.pos = (raz_analysis_pos*)ws.take(np * sizeof(raz_analysis_pos));
    d.eval = (raz_analysis_eval*)ws.take(np * sizeof(raz_analysis_eval));
    if (A) *A = d;
    return ws.off;
}

// The replay.  Thread g walks game g's list as NBoardEngine.set_game does, writes the position before every entry and arms the slot of
// every position that is to be searched: the mover's own discs as "black", player 1, one move, no resignation (the NBoard engine's
// player is made with enable_resign=False, nboard.py:50).  (The workspace was cleared by the memset ahead of this launch: positions
// beyond a game's walk stay NONE, every eval starts as zeros.)
__global__ __launch_bounds__(256) void k_analysis_start(raz_analysis_dev A, raz_engine_dev E, const unsigned long long* black,
                                                        const unsigned long long* white, const uint8_t* player, const int8_t* moves,
                                                        uint32_t sims) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.n) return;
    unsigned long long b = black ? black[g] : RAZ_INIT_BLACK, w = black ? white[g] : RAZ_INIT_WHITE;
    uint32_t pl = black ? player[g] : (uint32_t)RAZ_PLAYER_BLACK;
    raz_analysis_game ag;
    ag.positions = 0;
    ag.ended = RAZ_ANALYSIS_END_LIST;
    ag.winner = 0;
    ag.errors = 0;
    ag.searched = 0;
    bool over = false;
    const int8_t* list = moves + (size_t)g * A.max_moves;
    for (uint32_t j = 0; j < A.P; ++j) {
        const size_t pi = (size_t)g * A.P + j;
        int code = j < A.max_moves ? (int)list[j] : RAZ_ANALYSIS_ENTRY_END;
        if (!over && (code < RAZ_ANALYSIS_ENTRY_END || code > 63)) {   // not an entry: the list ends here, and the game says so
            ag.errors |= RAZ_ANALYSIS_ERR_BAD_CODE;
            code = RAZ_ANALYSIS_ENTRY_END;
        }
        raz_analysis_pos ap;
        ap.black = b;
        ap.white = w;
        ap.player = (uint8_t)pl;
        ap.moves_made = (uint8_t)j;
        ap.pad = 0;
        ap.played = (int8_t)((over || code == RAZ_ANALYSIS_ENTRY_END) ? RAZ_ANALYSIS_ENTRY_END : code);
        ap.state = (uint8_t)(over ? RAZ_ANALYSIS_POS_OVER : (code == RAZ_ANALYSIS_ENTRY_PASS ? RAZ_ANALYSIS_POS_PASS_ENTRY : RAZ_ANALYSIS_POS_SEARCH));
        A.pos[pi] = ap;
        ag.positions = j + 1;
        if (ap.state == RAZ_ANALYSIS_POS_SEARCH) {
            const bool blk = pl == RAZ_PLAYER_BLACK;
            arm_slot(E, A.first_slot + (uint32_t)pi, blk ? b : w, blk ? w : b, RAZ_PLAYER_BLACK, sims, 0u, 1u);
            A.eval[pi].state = RAZ_ANALYSIS_EVAL_PENDING;
            ag.searched += 1;
        }
        if (over || code == RAZ_ANALYSIS_ENTRY_END) break;
        if (code == RAZ_ANALYSIS_ENTRY_PASS) continue;   // (nboard.py:102: no env.step - ReversiEnv.step made the pass already)
        const raz_step_result r = bb_env_step(b, w, (int)pl, code);
        b = r.black;
        w = r.white;
        pl = r.player;
        if (r.status) {
            over = true;
            ag.winner = (uint8_t)(r.status & RAZ_STATUS_WINNER_MASK);
            ag.ended = (uint8_t)((r.status & RAZ_STATUS_ILLEGAL) ? RAZ_ANALYSIS_END_ILLEGAL : RAZ_ANALYSIS_END_RULES);
        }
    }
    ag.blacks = (uint8_t)bb_popcount(b);
    ag.whites = (uint8_t)bb_popcount(w);
    A.game[g] = ag;
    atomicAdd(&A.counters[kAnaGames], 1u);
    atomicAdd(&A.counters[kAnaPositions], ag.positions);
    atomicAdd(&A.counters[kAnaArmed], ag.searched);
    atomicAdd(&A.counters[kAnaPending], ag.searched);
    if (ag.errors) atomicOr(&A.counters[kAnaError], ag.errors);
}

// The reduction.  One wave per position, lane = square.  Where the position is pending and its slot has decided (phase idle, one ply
// recorded: raz_handoff.h slot_answer), the root's statistics become the position's eval; a position already collected, not searched, or
// still searching is left alone, byte for byte.
__global__ __launch_bounds__(64 * kAnaWavesPerBlock) void k_analysis_collect(raz_analysis_dev A, raz_engine_dev E) {
    const int lane = (int)(threadIdx.x & 63u);
    const size_t pi = (size_t)blockIdx.x * kAnaWavesPerBlock + (threadIdx.x >> 6);
    if (pi >= (size_t)A.n * A.P) return;
    raz_analysis_eval* ev = A.eval + pi;
    if (ev->state != RAZ_ANALYSIS_EVAL_PENDING) return;
    const uint32_t slot = A.first_slot + (uint32_t)pi;
    const uint32_t err = slot_answer(E.game[slot]);
    if (err == kSlotSearching) return;   // no position waits for another
    const int played = A.pos[pi].played;
    if (err) {
        if (lane == 0) {
            ev->flags = err;
            ev->played = (int8_t)played;
            ev->action = -1;
            ev->state = RAZ_ANALYSIS_EVAL_ERROR;
            atomicOr(&A.counters[kAnaError], err);
            atomicAdd(&A.counters[kAnaFailed], 1u);
            atomicSub(&A.counters[kAnaPending], 1u);
        }
        return;
    }
    const size_t ri = (size_t)slot * E.max_plies;   // record 0: one-move mode records every move there
    const raz_ply_header* h = E.rec + ri;
    const int action = h->action;
    if (h->flags & 1u) {   // the root solver's answer: no search behind it, the header's exact n and q
        if (lane == 0) {
            const uint32_t n = (uint32_t)h->n;
            const double q = h->q;
            ev->top_q[0] = q;
            ev->top_n[0] = n;
            ev->top_square[0] = (int8_t)action;
            ev->played_q = played == action ? q : 0.0;
            ev->played_n = played == action ? n : 0u;
            ev->sum_n = n;
            ev->n_top = 1;
            ev->played = (int8_t)played;
            ev->action = (int8_t)action;
            ev->state = RAZ_ANALYSIS_EVAL_SOLVED;
            atomicAdd(&A.counters[kAnaSolved], 1u);
            atomicSub(&A.counters[kAnaPending], 1u);
        }
        return;
    }
    const uint32_t n = E.rec_n[ri * 64 + lane];
    const double q = E.rec_w[ri * 64 + lane] / ((double)n + 1e-5);   // ReversiPlayer.var_q (agent/player.py): one addition, one division
    const uint32_t sum = wave_sum_u32(n);
    // the most visited squares, by visit count descending, the lowest square first among equals
    bool taken = false;
    uint32_t n_top = 0;
    for (; n_top < RAZ_ANALYSIS_TOP; ++n_top) {
        const uint32_t top = wave_max_u32(taken ? 0u : n);
        if (top == 0u) break;
        const int sq = __ffsll((long long)__ballot(!taken && n == top)) - 1;
        if (lane == sq) {
            ev->top_q[n_top] = q;
            ev->top_n[n_top] = n;
            ev->top_square[n_top] = (int8_t)sq;
            taken = true;
        }
    }
    if (lane == played) {
        ev->played_q = q;
        ev->played_n = n;
    }
    if (lane == 0) {
        ev->sum_n = sum;
        ev->n_top = (uint8_t)n_top;
        ev->played = (int8_t)played;
        ev->action = (int8_t)action;
        ev->state = RAZ_ANALYSIS_EVAL_SEARCHED;
        atomicAdd(&A.counters[kAnaSearched], 1u);
        atomicSub(&A.counters[kAnaPending], 1u);
    }
}

}  // namespace

struct raz_analysis {
    raz_engine* engine;
    raz_analysis_dev dev;
    size_t bytes;
    bool started;
};

extern "C" size_t raz_analysis_workspace_bytes(uint32_t n_games, uint32_t max_moves) {
    if (n_games == 0) {
        raz_fail(RAZ_EINVAL, "raz_analysis_workspace_bytes: n_games must be > 0");
        return 0;
    }
    if (max_moves < 1 || max_moves > RAZ_ANALYSIS_MAX_MOVES) {
        raz_fail(RAZ_EINVAL, "raz_analysis_workspace_bytes: max_moves must be 1..127");
        return 0;
    }
    return analysis_carve(n_games, max_moves, 0, nullptr, nullptr);
}

extern "C" int raz_analysis_create(raz_engine* engine, uint32_t first_slot, void* d_workspace, size_t workspace_bytes, uint32_t n_games,
                                   uint32_t max_moves, raz_analysis** out) {
    if (!engine || !d_workspace || !out) return raz_fail(RAZ_EINVAL, "raz_analysis_create: NULL argument");
    if (n_games == 0) return raz_fail(RAZ_EINVAL, "raz_analysis_create: n_games must be > 0");
    if (max_moves < 1 || max_moves > RAZ_ANALYSIS_MAX_MOVES) return raz_fail(RAZ_EINVAL, "raz_analysis_create: max_moves must be 1..127");
    if (!engine->started) return raz_fail(RAZ_ESTATE, "raz_analysis_create: call raz_engine_start on the engine first");
    if (!engine->dev.rec_w) return raz_fail(RAZ_ESTATE, "raz_analysis_create: engine created with record_root_w=0");
    if ((unsigned long long)first_slot + (unsigned long long)n_games * (max_moves + 1) > engine->dev.B)
        return raz_fail(RAZ_EINVAL, "raz_analysis_create: first_slot + n_games x (max_moves + 1) is beyond the engine's slots");
    const size_t need = analysis_carve(n_games, max_moves, first_slot, nullptr, nullptr);
    if (int rc = handoff_check_workspace("raz_analysis_create", "raz_analysis_workspace_bytes()", d_workspace, workspace_bytes, need)) return rc;
    raz_analysis* a = new (std::nothrow) raz_analysis();
    if (!a) return raz_fail(RAZ_ENOMEM, "raz_analysis_create: out of host memory");
    a->engine = engine;
    a->bytes = need;
    analysis_carve(n_games, max_moves, first_slot, (unsigned char*)d_workspace, &a->dev);
    a->started = false;
    *out = a;
    return RAZ_OK;
}

extern "C" void raz_analysis_destroy(raz_analysis* a) { delete a; }

extern "C" int raz_analysis_start(raz_analysis* a, const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player,
                                  const int8_t* d_moves, uint32_t sims, raz_stream_t stream) {
    if (!a || !d_moves) return raz_fail(RAZ_EINVAL, "raz_analysis_start: NULL argument");
    if (int rc = handoff_check_positions("raz_analysis_start", d_black, d_white, d_player)) return rc;
    if (sims == 0) return raz_fail(RAZ_EINVAL, "raz_analysis_start: sims must be > 0");
    if (!a->engine->started) return raz_fail(RAZ_ESTATE, "raz_analysis_start: the engine is not started");
    hipStream_t s = (hipStream_t)stream;
    const raz_analysis_dev& d = a->dev;
    RAZ_HIP_TRY(hipMemsetAsync(d.counters, 0, a->bytes, s), "raz_analysis_start: clear");
    hipLaunchKernelGGL(k_analysis_start, dim3((d.n + 255) / 256), dim3(256), 0, s, d, a->engine->dev, (const unsigned long long*)d_black,
                       (const unsigned long long*)d_white, d_player, d_moves, sims);
    int rc = raz_check_launch("raz_analysis_start");
    a->started = rc == RAZ_OK;
    return rc;
}

extern "C" int raz_analysis_collect(raz_analysis* a, raz_stream_t stream) {
    if (!a) return raz_fail(RAZ_EINVAL, "raz_analysis_collect: NULL analysis");
    if (!a->started) return raz_fail(RAZ_ESTATE, "raz_analysis_collect: call raz_analysis_start first");
    const raz_analysis_dev& d = a->dev;
    const size_t np = (size_t)d.n * d.P;
    hipLaunchKernelGGL(k_analysis_collect, dim3((unsigned)((np + kAnaWavesPerBlock - 1) / kAnaWavesPerBlock)), dim3(64 * kAnaWavesPerBlock), 0,
                       (hipStream_t)stream, d, a->engine->dev);
    return raz_check_launch("raz_analysis_collect");
}

extern "C" int raz_analysis_stats_sync(raz_analysis* a, raz_analysis_stats* out, raz_stream_t stream) {
    if (!a || !out) return raz_fail(RAZ_EINVAL, "raz_analysis_stats_sync: NULL argument");
    if (!a->started) return raz_fail(RAZ_ESTATE, "raz_analysis_stats_sync: call raz_analysis_start first");
    RAZ_HIP_TRY(hipMemcpyAsync(out, a->dev.counters, sizeof *out, hipMemcpyDeviceToHost, (hipStream_t)stream), "raz_analysis_stats_sync: copy");
    RAZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "raz_analysis_stats_sync: sync");
    return RAZ_OK;
}

extern "C" int raz_analysis_read(raz_analysis* a, raz_analysis_game* games, raz_analysis_pos* positions, raz_analysis_eval* evals,
                                 raz_stream_t stream) {
    if (!a) return raz_fail(RAZ_EINVAL, "raz_analysis_read: NULL analysis");
    if (!a->started) return raz_fail(RAZ_ESTATE, "raz_analysis_read: call raz_analysis_start first");
    hipStream_t s = (hipStream_t)stream;
    const raz_analysis_dev& d = a->dev;
    const size_t np = (size_t)d.n * d.P;
    if (games) RAZ_HIP_TRY(hipMemcpyAsync(games, d.game, (size_t)d.n * sizeof(raz_analysis_game), hipMemcpyDeviceToHost, s), "raz_analysis_read: games");
    if (positions) RAZ_HIP_TRY(hipMemcpyAsync(positions, d.pos, np * sizeof(raz_analysis_pos), hipMemcpyDeviceToHost, s), "raz_analysis_read: positions");
    if (evals) RAZ_HIP_TRY(hipMemcpyAsync(evals, d.eval, np * sizeof(raz_analysis_eval), hipMemcpyDeviceToHost, s), "raz_analysis_read: evals");
    RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_analysis_read: sync");
    return RAZ_OK;
}
