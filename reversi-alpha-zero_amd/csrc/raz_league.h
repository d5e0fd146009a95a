// raz_league.h — a league of up to 16 models on the device: the hand-off of raz_handoff.h with (model, slot) read from a pairing per
// game instead of "two engines, slot g <-> game g" (include/raz.h raz_league_*).
//
// Game g names its two models and the slot of each model's engine that plays it (raz_league_pairing); league_ctx makes seats of
// them, and start_game / turn_game (raz_handoff.h) do the rest as they do it for the match.  The engines' descriptors
// (raz_engine_dev) are a TABLE IN THE WORKSPACE, not kernel arguments: sixteen of them do not fit a kernel-argument segment
// (static_assert below).
//
// Part of raz_engine.hip's translation unit, behind raz_handoff.h.  One thread per game; plain vector stores, no floating point,
// integer atomics for the counters and the claim words only.
#pragma once

namespace {

// raz_league_stats as u32 words
enum { kLeagueLive = 0, kLeaguePlies = 1, kLeagueError = 2, kLeagueModels = 3, kLeagueSearching = 4 /* + model */ };

struct raz_league_dev {
    uint32_t n_games, n_models;
    uint32_t* counters;            // raz_league_stats
    raz_engine_dev* table;         // [n_models] the engines' descriptors as last uploaded
    raz_league_pairing* pairing;   // [n_games] copied by raz_league_start
    raz_league_game* game;         // [n_games]
    raz_league_ply* log;           // [n_games][RAZ_LEAGUE_MAX_PLIES]
    uint32_t* claim;               // [sum of the engines' slots] lowest game index that names the slot; model m's words start at claim_off[m]
    uint32_t* log_n;               // [n_games][RAZ_LEAGUE_MAX_PLIES][64]
    uint32_t claim_off[RAZ_LEAGUE_MAX_MODELS];
    uint32_t slots[RAZ_LEAGUE_MAX_MODELS];   // the engines' n_games
    const uint32_t* sims;          // [RAZ_LEAGUE_MAX_MODELS] simulations a move per model, behind the stats in their section (raz_league_start)
};
static_assert(sizeof(raz_league_pairing) == 16 && sizeof(raz_league_game) == 32 && sizeof(raz_league_ply) == 4 &&
              sizeof(raz_league_stats) == 128, "raz_league layouts");
static_assert(RAZ_LEAGUE_MAX_MODELS * sizeof(raz_engine_dev) > 4096, "the descriptor table would fit kernel arguments: it need not live in HBM");
static_assert(sizeof(raz_engine_dev) % 8 == 0, "raz_engine_dev [n_models] in a 256-byte aligned section");

// The sections raz_league_start clears (counters, games, log headers; claim words) lie together.
inline size_t league_carve(uint32_t n_models, const uint32_t* slots, uint32_t n_games, unsigned char* base, raz_league_dev* L) {
    carver ws{base, 0};
    raz_league_dev d;
    memset(&d, 0, sizeof d);
    d.n_games = n_games;
    d.n_models = n_models;
    size_t total = 0;
    for (uint32_t m = 0; m < n_models; ++m) {
        d.claim_off[m] = (uint32_t)total;
        d.slots[m] = slots[m];
        total += slots[m];
    }
    d.counters = (uint32_t*)ws.take(sizeof(raz_league_stats) + RAZ_LEAGUE_MAX_MODELS * 4);
    d.sims = base ? d.counters + sizeof(raz_league_stats) / 4 : nullptr;
    d.table = (raz_engine_dev*)ws.take((size_t)n_models * sizeof(raz_engine_dev));
    d.pairing = (raz_league_pairing*)ws.take((size_t)n_games * sizeof(raz_league_pairing));
    d.game = (raz_league_game*)ws.take((size_t)n_games * sizeof(raz_league_game));
    d.log = (raz_league_ply*)ws.take((size_t)n_games * RAZ_LEAGUE_MAX_PLIES * sizeof(raz_league_ply));
    d.claim = (uint32_t*)ws.take(total * 4);
    d.log_n = (uint32_t*)ws.take((size_t)n_games * RAZ_LEAGUE_MAX_PLIES * 64 * 4);
    if (L) *L = d;
    return ws.off;
}

// Both model indices below n_models and different, both slots below their engine's n_games.
__device__ __forceinline__ bool league_sound(const raz_league_dev& L, const raz_league_pairing& P) {
    if (P.black_model >= L.n_models || P.white_model >= L.n_models || P.black_model == P.white_model) return false;
    return P.black_slot < L.slots[P.black_model] && P.white_slot < L.slots[P.white_model];
}

__device__ __forceinline__ void league_claim(uint32_t* word, uint32_t g) {
#ifdef RAZ_WAVE_EMU
    if (g < *word) *word = g;   // (the emulator runs one lane at a time and has no atomicMin)
#else
    atomicMin(word, g);
#endif
}

// The league's seats: (model, slot) of a colour from the game's pairing, the engine from the table in the workspace.
struct league_ctx {
    const raz_league_dev& D;
    const raz_league_pairing P;
    uint32_t enable_resign;
    enum { live = kLeagueLive, plies = kLeaguePlies, error = kLeagueError, searching = kLeagueSearching };
    __device__ __forceinline__ handoff_seat seat(uint32_t, const raz_league_game&, uint32_t colour) const {
        const bool b = colour == RAZ_PLAYER_BLACK;
        const uint32_t model = b ? P.black_model : P.white_model;
        return handoff_seat{D.table[model], b ? P.black_slot : P.white_slot, model, D.sims[model]};
    }
    __device__ __forceinline__ uint32_t code(const raz_league_game&, uint32_t colour) const { return colour; }   // 1: black's model's slot, 2: white's
};

// Start, first launch: keep game g's pairing and, where it is sound, claim its two slots for the lowest game index that names them.
// (The claim words were set to 0xffffffff by the memset ahead of this launch.)
__global__ __launch_bounds__(256) void k_league_claim(raz_league_dev L, const raz_league_pairing* pairings) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= L.n_games) return;
    raz_league_pairing P = pairings[g];
    P.pad0 = 0;
    P.pad1 = 0;
    L.pairing[g] = P;
    if (!league_sound(L, P)) return;
    league_claim(&L.claim[L.claim_off[P.black_model] + P.black_slot], g);
    league_claim(&L.claim[L.claim_off[P.white_model] + P.white_slot], g);
}

// Start, second launch: game g starts where its pairing is sound and both its slots are its own; then as k_match_start starts one
// (start_game).  Slots no started game names are not touched.
__global__ __launch_bounds__(256) void k_league_start(raz_league_dev L, const unsigned long long* black, const unsigned long long* white,
                                                      const uint8_t* player, uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= L.n_games) return;
    if (g == 0) L.counters[kLeagueModels] = L.n_models;
    const raz_league_pairing P = L.pairing[g];
    raz_league_game mg;
    init_game(mg, g, black, white, player);
    mg.black_model = P.black_model;
    mg.white_model = P.white_model;
    mg.pad8[0] = mg.pad8[1] = mg.pad8[2] = 0;
    mg.pad = 0;
    const bool mine = league_sound(L, P) && L.claim[L.claim_off[P.black_model] + P.black_slot] == g &&
                      L.claim[L.claim_off[P.white_model] + P.white_slot] == g;
    if (!mine) {
        mg.searching = 0;
        mg.flags = (uint8_t)RAZ_LEAGUE_GAME_NOT_STARTED;
        L.game[g] = mg;
        atomicOr(&L.counters[kLeagueError], RAZ_LEAGUE_ERR_PAIRING);
        return;
    }
    start_game(league_ctx{L, P, enable_resign}, g, mg);
}

// The hand-off (raz_handoff.h turn_game) for every game that is live, with (model, slot) from the game's pairing.
__global__ __launch_bounds__(256) void k_league_turn(raz_league_dev L, uint32_t enable_resign) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= L.n_games) return;
    raz_league_game mg = L.game[g];
    if (mg.searching == 0) return;   // the game has ended, or never started
    mg.pad8[0] = mg.pad8[1] = mg.pad8[2] = 0;   // (stated, not carried: seven odd bytes carried from load to store cost a private array)
    mg.pad = 0;
    turn_game(league_ctx{L, L.pairing[g], enable_resign}, g, mg);
}

}  // namespace

struct raz_league {
    raz_engine* engine[RAZ_LEAGUE_MAX_MODELS];
    raz_engine_dev uploaded[RAZ_LEAGUE_MAX_MODELS];   // the descriptors as the table in the workspace holds them
    raz_league_dev dev;
    uint32_t sims[RAZ_LEAGUE_MAX_MODELS];             // ... and the simulations a move
    uint32_t enable_resign;
    bool started;
};

extern "C" size_t raz_league_workspace_bytes(uint32_t n_models, const uint32_t* slots_per_model, uint32_t n_games) {
    if (n_models < 2 || n_models > RAZ_LEAGUE_MAX_MODELS) {
        raz_fail(RAZ_EINVAL, "raz_league_workspace_bytes: n_models must be 2..16");
        return 0;
    }
    if (n_games == 0 || !slots_per_model) {
        raz_fail(RAZ_EINVAL, "raz_league_workspace_bytes: n_games must be > 0 and slots_per_model given");
        return 0;
    }
    return league_carve(n_models, slots_per_model, n_games, nullptr, nullptr);
}

extern "C" int raz_league_create(raz_engine* const* engines, uint32_t n_models, void* d_workspace, size_t workspace_bytes, uint32_t n_games,
                                 raz_league** out) {
    if (!engines || !d_workspace || !out) return raz_fail(RAZ_EINVAL, "raz_league_create: NULL argument");
    if (n_models < 2 || n_models > RAZ_LEAGUE_MAX_MODELS) return raz_fail(RAZ_EINVAL, "raz_league_create: n_models must be 2..16");
    if (n_games == 0) return raz_fail(RAZ_EINVAL, "raz_league_create: n_games must be > 0");
    uint32_t slots[RAZ_LEAGUE_MAX_MODELS];
    for (uint32_t m = 0; m < n_models; ++m) {
        if (!engines[m]) return raz_fail(RAZ_EINVAL, "raz_league_create: NULL argument (an engine)");
        for (uint32_t k = 0; k < m; ++k)
            if (engines[k] == engines[m]) return raz_fail(RAZ_EINVAL, "raz_league_create: every model needs an engine of its own (the same engine twice)");
        slots[m] = engines[m]->dev.B;
    }
    for (uint32_t m = 0; m < n_models; ++m)
        if (!engines[m]->started) return raz_fail(RAZ_ESTATE, "raz_league_create: call raz_engine_start on every engine first");
    const size_t need = league_carve(n_models, slots, n_games, nullptr, nullptr);
    if (int rc = handoff_check_workspace("raz_league_create", "raz_league_workspace_bytes()", d_workspace, workspace_bytes, need)) return rc;
    raz_league* l = new (std::nothrow) raz_league();
    if (!l) return raz_fail(RAZ_ENOMEM, "raz_league_create: out of host memory");
    for (uint32_t m = 0; m < n_models; ++m) l->engine[m] = engines[m];
    league_carve(n_models, slots, n_games, (unsigned char*)d_workspace, &l->dev);
    l->started = false;
    *out = l;
    return RAZ_OK;
}

extern "C" void raz_league_destroy(raz_league* l) { delete l; }

namespace {
// Bring the table in the workspace up to the engines' present descriptors, ordered on `s`; all: every entry, else the changed ones.
int league_upload(raz_league* l, bool all, hipStream_t s, const char* what) {
    for (uint32_t m = 0; m < l->dev.n_models; ++m) {
        if (!all && memcmp(&l->engine[m]->dev, &l->uploaded[m], sizeof(raz_engine_dev)) == 0) continue;
        memcpy(&l->uploaded[m], &l->engine[m]->dev, sizeof(raz_engine_dev));
        RAZ_HIP_TRY(hipMemcpyAsync(l->dev.table + m, &l->uploaded[m], sizeof(raz_engine_dev), hipMemcpyHostToDevice, s), what);
    }
    return RAZ_OK;
}
}  // namespace

extern "C" int raz_league_start(raz_league* l, const raz_league_pairing* d_pairings, const uint64_t* d_black, const uint64_t* d_white,
                                const uint8_t* d_player, const uint32_t* sims_per_model, int enable_resign, raz_stream_t stream) {
    if (!l || !d_pairings || !sims_per_model) return raz_fail(RAZ_EINVAL, "raz_league_start: NULL argument");
    if (int rc = handoff_check_positions("raz_league_start", d_black, d_white, d_player)) return rc;
    if ((uintptr_t)d_pairings % 4) return raz_fail(RAZ_EINVAL, "raz_league_start: d_pairings must be 4-byte aligned");
    raz_league_dev& d = l->dev;
    for (uint32_t m = 0; m < d.n_models; ++m) {
        if (sims_per_model[m] == 0) return raz_fail(RAZ_EINVAL, "raz_league_start: sims must be > 0");
        if (!l->engine[m]->started) return raz_fail(RAZ_ESTATE, "raz_league_start: an engine is not started");
    }
    hipStream_t s = (hipStream_t)stream;
    // the counters; the games, the log's headers (the visit counts of a ply are written with its header); the claim words
    RAZ_HIP_TRY(hipMemsetAsync(d.counters, 0, sizeof(raz_league_stats), s), "raz_league_start: clear counters");
    RAZ_HIP_TRY(hipMemsetAsync(d.game, 0, (size_t)((unsigned char*)d.claim - (unsigned char*)d.game), s), "raz_league_start: clear");
    RAZ_HIP_TRY(hipMemsetAsync(d.claim, 0xff, (size_t)((unsigned char*)d.log_n - (unsigned char*)d.claim), s), "raz_league_start: clear claims");
    if (int rc = league_upload(l, true, s, "raz_league_start: descriptor table")) return rc;
    for (uint32_t m = 0; m < RAZ_LEAGUE_MAX_MODELS; ++m) l->sims[m] = m < d.n_models ? sims_per_model[m] : 0u;
    RAZ_HIP_TRY(hipMemcpyAsync((void*)d.sims, l->sims, sizeof l->sims, hipMemcpyHostToDevice, s), "raz_league_start: sims");
    l->enable_resign = enable_resign != 0;
    const dim3 grid((d.n_games + 255) / 256), block(256);
    hipLaunchKernelGGL(k_league_claim, grid, block, 0, s, d, d_pairings);
    int rc = raz_check_launch("raz_league_start: claim");
    if (rc != RAZ_OK) return rc;
    hipLaunchKernelGGL(k_league_start, grid, block, 0, s, d, (const unsigned long long*)d_black, (const unsigned long long*)d_white, d_player,
                       l->enable_resign);
    rc = raz_check_launch("raz_league_start");
    l->started = rc == RAZ_OK;
    return rc;
}

extern "C" int raz_league_turn(raz_league* l, raz_stream_t stream) {
    if (!l) return raz_fail(RAZ_EINVAL, "raz_league_turn: NULL league");
    if (!l->started) return raz_fail(RAZ_ESTATE, "raz_league_turn: call raz_league_start first");
    // (raz_engine_set_solver_pool_every and the like between two turns: no stale descriptor is left behind)
    if (int rc = league_upload(l, false, (hipStream_t)stream, "raz_league_turn: descriptor table")) return rc;
    const raz_league_dev& d = l->dev;
    hipLaunchKernelGGL(k_league_turn, dim3((d.n_games + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, l->enable_resign);
    return raz_check_launch("raz_league_turn");
}

extern "C" int raz_league_stats_sync(raz_league* l, raz_league_stats* out, raz_stream_t stream) {
    if (!l || !out) return raz_fail(RAZ_EINVAL, "raz_league_stats_sync: NULL argument");
    if (!l->started) return raz_fail(RAZ_ESTATE, "raz_league_stats_sync: call raz_league_start first");
    RAZ_HIP_TRY(hipMemcpyAsync(out, l->dev.counters, sizeof *out, hipMemcpyDeviceToHost, (hipStream_t)stream), "raz_league_stats_sync: copy");
    RAZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "raz_league_stats_sync: sync");
    return RAZ_OK;
}

extern "C" int raz_league_read(raz_league* l, raz_league_game* games, raz_league_pairing* pairings, raz_league_ply* log, uint32_t* log_root_n,
                               raz_stream_t stream) {
    if (!l) return raz_fail(RAZ_EINVAL, "raz_league_read: NULL league");
    if (!l->started) return raz_fail(RAZ_ESTATE, "raz_league_read: call raz_league_start first");
    hipStream_t s = (hipStream_t)stream;
    const raz_league_dev& d = l->dev;
    const size_t n = d.n_games;
    if (games) RAZ_HIP_TRY(hipMemcpyAsync(games, d.game, n * sizeof(raz_league_game), hipMemcpyDeviceToHost, s), "raz_league_read: games");
    if (pairings) RAZ_HIP_TRY(hipMemcpyAsync(pairings, d.pairing, n * sizeof(raz_league_pairing), hipMemcpyDeviceToHost, s), "raz_league_read: pairings");
    if (int rc = handoff_read_log("raz_league_read", n, log, d.log, log_root_n, d.log_n, s)) return rc;
    RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_league_read: sync");
    return RAZ_OK;
}
