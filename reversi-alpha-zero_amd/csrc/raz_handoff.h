// raz_handoff.h — the engine hand-off, stated once for raz_match.h, raz_league.h and raz_analysis.h.
//
// The protocol: a slot of a started engine is armed in one-move mode (raz_engine_set_position's semantics).  After its search
// finalize_move (raz_engine_core.h) has left in it the position after the move IN THE MOVER'S FRAME (root_black = the mover's discs,
// player 1 = the mover moves again: the opponent passed), the status in that frame and the ply's record 0.  A slot that is idle
// with exactly one ply recorded has decided; anything else that is not "still searching" is an error that ends the game.
//
// Part of raz_engine.hip's translation unit (it needs struct raz_engine and arm_slot), included ahead of its three users.
#pragma once

static_assert(RAZ_MATCH_ERR_SLOT == RAZ_LEAGUE_ERR_SLOT && RAZ_MATCH_ERR_SLOT == RAZ_ANALYSIS_ERR_SLOT, "one word for a slot off the protocol");
static_assert(RAZ_MATCH_ERR_LOG_FULL == RAZ_LEAGUE_ERR_LOG_FULL, "one word for a full log");
static_assert(RAZ_MATCH_MAX_PLIES == RAZ_LEAGUE_MAX_PLIES, "a league game's log is a match game's");

namespace {

// ---- host: the workspace, the checks and the copies the three handles share ----------------------------------------------------------
inline size_t round_up_256(size_t x) { return (x + 255) / 256 * 256; }

// A workspace carved into sections of whole 256 bytes; with base == nullptr only the total size is computed.
struct carver {
    unsigned char* base;
    size_t off;
    unsigned char* take(size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off = round_up_256(off + bytes);
        return p;
    }
};

inline int handoff_fail(const char* fn, const char* text, const char* arg = "") {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s%s", fn, text, arg);
    return raz_fail(RAZ_EINVAL, msg);
}

// The workspace of `fn` (a raz_*_create): 256-byte aligned and at least the carve, which `sizer` (a raz_*_workspace_bytes) reports.
inline int handoff_check_workspace(const char* fn, const char* sizer, const void* d_workspace, size_t workspace_bytes, size_t need) {
    if ((uintptr_t)d_workspace % 256) return handoff_fail(fn, "workspace must be 256-byte aligned");
    return workspace_bytes < need ? handoff_fail(fn, "workspace smaller than ", sizer) : RAZ_OK;
}

// The start positions of `fn` (a raz_*_start): the three arrays go together, and the boards are 8-byte aligned.
inline int handoff_check_positions(const char* fn, const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player) {
    if ((d_black != nullptr) != (d_white != nullptr) || (d_black != nullptr) != (d_player != nullptr))
        return handoff_fail(fn, "d_black, d_white and d_player go together, all or none");
    return (uintptr_t)d_black % 8 || (uintptr_t)d_white % 8 ? handoff_fail(fn, "d_black / d_white must be 8-byte aligned") : RAZ_OK;
}

// The log copies of `fn` (a raz_*_read) for n games: the ply headers and the root visit counts, either may be NULL.
inline int handoff_read_log(const char* fn, size_t n, void* log, const void* d_log, uint32_t* log_root_n, const uint32_t* d_log_n, hipStream_t s) {
    char where[64];
    snprintf(where, sizeof where, "%s: log", fn);
    if (log) RAZ_HIP_TRY(hipMemcpyAsync(log, d_log, n * RAZ_MATCH_MAX_PLIES * sizeof(raz_match_ply), hipMemcpyDeviceToHost, s), where);
    snprintf(where, sizeof where, "%s: visit counts", fn);
    if (log_root_n) RAZ_HIP_TRY(hipMemcpyAsync(log_root_n, d_log_n, n * RAZ_MATCH_MAX_PLIES * 64 * 4, hipMemcpyDeviceToHost, s), where);
    return RAZ_OK;
}

// ---- device: the decided-slot rule ----------------------------------------------------------------------------------------------
enum : uint32_t { kSlotSearching = 0xffffffffu };   // (no error word: the engine's flags are 1..8, the users' 0x100..0x800)
// What an armed slot says: kSlotSearching - leave it alone, nobody waits for another; 0 - decided, record 0 and the root hold the
// answer; else the error word that ends the game: the engine's own flags, or ERR_SLOT for a slot that left the one-move protocol.
__device__ __forceinline__ uint32_t slot_answer(const raz_game& G) {
    const uint32_t phase = G.phase, slot_error = G.error, slot_plies = G.n_plies;
    if (slot_error) return slot_error;
    if (phase != RAZ_PHASE_IDLE && phase != RAZ_PHASE_DONE) return kSlotSearching;
    return (phase == RAZ_PHASE_DONE || slot_plies != 1u) ? RAZ_MATCH_ERR_SLOT : 0u;
}

// ---- device: games of two seats ---------------------------------------------------------------------------------------------------
// A seat: the engine slot that plays one colour of a game, the index `who` of its side (in the searching counters and in the log)
// and its simulations a move.  A context C names the seats and counters of one user:
//   C.D (counters, game, log, log_n: the workspace), C.enable_resign
//   C.seat(g, game, colour)   the seat that moves for `colour` in game g
//   C.code(game, colour)      the game's `searching` byte while that seat searches (never 0)
//   C.live / plies / error / searching   counter indices; a seat's counter is searching + who
// INVARIANT: the searching slot of a live game (searching != 0) is the mover's, seat(g, game, game.player).  start_game arms that
// seat; turn_game ends the game or arms the seat of the new side to move, on every path.
struct handoff_seat { const raz_engine_dev& E; uint32_t slot, who, sims; };
struct alignas(16) handoff_q4 { uint32_t x, y, z, w; };

// Ask the seat for the move of colour game.player on the real board: the mover's own discs are "black" inside its tree, whatever its
// colour in the game (agent/player.py:95), so the slot is armed with player 1.
template <class Game>
__device__ __forceinline__ void arm_seat(const handoff_seat& S, const Game& mg, uint32_t enable_resign) {
    const bool b = mg.player == RAZ_PLAYER_BLACK;
    arm_slot(S.E, S.slot, b ? mg.black : mg.white, b ? mg.white : mg.black, RAZ_PLAYER_BLACK, S.sims, enable_resign, 1u);
}

// Game g's record on its start position (NULL arrays: the initial position, black to move); the user's own fields are the caller's.
template <class Game>
__device__ __forceinline__ void init_game(Game& mg, uint32_t g, const unsigned long long* black, const unsigned long long* white, const uint8_t* player) {
    mg.black = black ? black[g] : RAZ_INIT_BLACK;
    mg.white = black ? white[g] : RAZ_INIT_WHITE;
    mg.player = black ? player[g] : (uint8_t)RAZ_PLAYER_BLACK;
    mg.winner = mg.blacks = mg.whites = mg.n_plies = mg.flags = 0;
}

// The game starts: its record stored, the side to move armed and counted.
template <class Ctx, class Game>
__device__ __forceinline__ void start_game(const Ctx& C, uint32_t g, Game& mg) {
    const handoff_seat S = C.seat(g, mg, mg.player);
    mg.searching = (uint8_t)C.code(mg, mg.player);
    C.D.game[g] = mg;
    arm_seat(S, mg, C.enable_resign);
    atomicAdd(&C.D.counters[Ctx::live], 1u);
    atomicAdd(&C.D.counters[Ctx::searching + S.who], 1u);
}

// The hand-off for live game g (mg = its record).  Where the searching slot has decided, this does for the game what
// `env.step(action)` and the next `player.action(own, enemy)` call do in the reference's loop (worker/evaluate.py:66-96).
template <class Ctx, class Game>
__device__ __forceinline__ void turn_game(const Ctx& C, uint32_t g, Game& mg) {
    const handoff_seat S = C.seat(g, mg, mg.player);
    const raz_game& G = S.E.game[S.slot];
    uint32_t err = slot_answer(G);
    if (err == kSlotSearching) return;
    // (LOG_FULL cannot be reached from a playable position - a ply fills a square, a playable position has two discs at least, so a
    //  game has at most 62 plies and the log holds 64; the check keeps the log's bounds all the same)
    if (!err && mg.n_plies >= RAZ_MATCH_MAX_PLIES) err = RAZ_MATCH_ERR_LOG_FULL;
    if (err) {   // the game ends here, undecided, and the error word says why
        atomicOr(&C.D.counters[Ctx::error], err);
        atomicSub(&C.D.counters[Ctx::live], 1u);
        atomicSub(&C.D.counters[Ctx::searching + S.who], 1u);
        mg.searching = 0;
        C.D.game[g] = mg;
        return;
    }
    // the ply: the slot's record 0 (one-move mode records every move there)
    const size_t ri = (size_t)S.slot * S.E.max_plies, li = (size_t)g * RAZ_MATCH_MAX_PLIES + mg.n_plies;
    std::remove_pointer_t<decltype(C.D.log)> ply;
    ply.who = (uint8_t)S.who;
    ply.action = S.E.rec[ri].action;
    ply.turn = S.E.rec[ri].turn;
    ply.pad = 0;
    C.D.log[li] = ply;
    const handoff_q4* src = (const handoff_q4*)(S.E.rec_n + ri * 64);
    handoff_q4* dst = (handoff_q4*)(C.D.log_n + li * 64);
    for (int i = 0; i < 16; ++i) dst[i] = src[i];
    mg.n_plies += 1;
    atomicAdd(&C.D.counters[Ctx::plies], 1u);
    // the slot's board and status, from the mover's frame ("black" = the mover) to absolute colours
    const uint32_t mover = mg.player, other = 3u - mover, status = G.status;
    const unsigned long long sb = G.root_black, sw = G.root_white;
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
        atomicSub(&C.D.counters[Ctx::live], 1u);
        atomicSub(&C.D.counters[Ctx::searching + S.who], 1u);
    } else {
        const handoff_seat N = C.seat(g, mg, mg.player);   // after a pass the same seat again
        arm_seat(N, mg, C.enable_resign);
        if (N.who != S.who) {
            mg.searching = (uint8_t)C.code(mg, mg.player);
            atomicSub(&C.D.counters[Ctx::searching + S.who], 1u);
            atomicAdd(&C.D.counters[Ctx::searching + N.who], 1u);
        }
    }
    C.D.game[g] = mg;
}

}  // namespace
