// raz_replay.hip — the trainer's packed rows, made on the device from the self-play outbox (include/raz.h raz_train_rows_count /
// raz_train_rows_fill).
//
// Reference: the same rows raz_emit.hip writes as text and the `opt` worker reads back (worker/self_play.py:180-194,219-231: black.moves
// + white.moves, z by the winner; agent/player.py:166-179: 8 symmetric rows per searched ply, :132,366-385: the saved policy;
// worker/optimize.py:214-231: the consumer), in the layout of lib/data_helper.pack_game_data - own u64[R], enemy u64[R], policy
// f32[R][64], z i8[R] - bit for bit what json.load + np.asarray(float32) make of the text: the proportional policy is the f64
// quotient n / sum(n) rounded ONCE to f32 (float.__repr__ round-trips the double, numpy rounds it to f32).
//
// Three kernels, no atomics, no scratch, plain vector stores:
//   k_rows_count  one wave per game, lane = ply (in chunks of 64): 8 x the plies that carry a row, into d_row_offset[g]
//   k_rows_scan   ONE workgroup turns those counts into their exclusive prefix sum in place, in game order, chunk after chunk with a
//                 running carry: one fixed order of additions, the total at [n_games]
//   k_rows_fill   one wave per (game, ply), lane = square: the ply's rank among the game's rows from ballots over the game's
//                 player / has_row bytes, the 256 B of root_n in one coalesced load, sum and first maximum by the wave reductions of
//                 raz_engine_core.h, then eight coalesced 256 B stores of the policy (the source lane of each symmetry by __shfl) and
//                 the eight board pairs and z bytes from lanes 0-7.
#include <stdio.h>
#include "raz_engine_core.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kScanBlock = 256;

// has_row plies of black / of white among plies [0, np) of game g, and among those before ply j: uniform over the wave
struct RowRanks {
    uint32_t black, white, black_before, white_before;
};
__device__ __forceinline__ RowRanks row_ranks(const raz_ply_header* __restrict__ H, uint32_t np, uint32_t j, int lane) {
    RowRanks r = {0u, 0u, 0u, 0u};
    for (uint32_t base = 0; base < np; base += 64) {   // (np is wave-uniform: every lane meets every ballot)
        const uint32_t p = base + (uint32_t)lane;
        uint32_t player = 0, has_row = 0;
        if (p < np) {
            player = H[p].player;
            has_row = H[p].has_row;
        }
        const unsigned long long mb = __ballot(has_row != 0 && player == RAZ_PLAYER_BLACK);
        const unsigned long long mw = __ballot(has_row != 0 && player == RAZ_PLAYER_WHITE);
        // the plies of this chunk that come before ply j
        const unsigned long long before = j >= base + 64 ? ~0ull : (j <= base ? 0ull : ((1ull << (j - base)) - 1ull));
        r.black += (uint32_t)__popcll(mb);
        r.white += (uint32_t)__popcll(mw);
        r.black_before += (uint32_t)__popcll(mb & before);
        r.white_before += (uint32_t)__popcll(mw & before);
    }
    return r;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_rows_count(const raz_ply_header* __restrict__ headers,
                                                                    const raz_game_summary* __restrict__ summary,
                                                                    const uint8_t* __restrict__ done, uint32_t n_games, uint32_t plies,
                                                                    uint32_t* __restrict__ row_offset) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t g = uni((uint32_t)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    if (g >= n_games) return;
    uint32_t rows = 0;
    if (!done || done[g]) {
        const uint32_t np = uni(min(summary[g].n_plies, plies));
        const RowRanks r = row_ranks(headers + (size_t)g * plies, np, 0u, lane);
        rows = 8u * (r.black + r.white);
    }
    if (lane == 0) row_offset[g] = rows;
}

// in place: row_offset[0 .. n_games) holds the games' row counts on entry, their exclusive prefix sum on exit, [n_games] the total
__global__ __launch_bounds__(kScanBlock) void k_rows_scan(uint32_t* __restrict__ row_offset, uint32_t n_games) {
    __shared__ uint32_t s[kScanBlock];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_games; base += kScanBlock) {
        const uint32_t i = base + t;
        const uint32_t v = i < n_games ? row_offset[i] : 0u;
        s[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
            const uint32_t x = t >= d ? s[t - d] : 0u;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        const uint32_t inclusive = s[t], total = s[kScanBlock - 1];
        if (i < n_games) row_offset[i] = carry + inclusive - v;
        carry += total;
        __syncthreads();   // (the next chunk overwrites s)
    }
    if (t == 0) row_offset[n_games] = carry;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_rows_fill(const raz_ply_header* __restrict__ headers,
                                                                   const uint32_t* __restrict__ root_n,
                                                                   const raz_game_summary* __restrict__ summary,
                                                                   const uint8_t* __restrict__ done, uint32_t n_games, uint32_t plies,
                                                                   int change_tau_turn, int save_policy_of_tau_1,
                                                                   const uint32_t* __restrict__ row_offset, unsigned long long capacity_rows,
                                                                   unsigned long long* __restrict__ out_own,
                                                                   unsigned long long* __restrict__ out_enemy, float* __restrict__ out_policy,
                                                                   int8_t* __restrict__ out_z) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t w = uni((uint32_t)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));   // < n_games * plies + 3 < 2^29 + 3
    const uint32_t g = w / plies, j = w - g * plies;
    if (g >= n_games) return;
    if (done && !done[g]) return;
    const uint32_t np = uni(min(summary[g].n_plies, plies));
    if (j >= np) return;
    const raz_ply_header* H = headers + (size_t)g * plies;
    const uint32_t player = uni((uint32_t)H[j].player);
    if (!uni((uint32_t)H[j].has_row) || (player != RAZ_PLAYER_BLACK && player != RAZ_PLAYER_WHITE)) return;
    // everything above is wave-uniform: the whole wave is here or nowhere

    // black.moves + white.moves: black's plies in ply order, then white's
    const RowRanks r = row_ranks(H, np, j, lane);
    const uint32_t rank = player == RAZ_PLAYER_BLACK ? r.black_before : r.black + r.white_before;
    const unsigned long long row0 = (unsigned long long)row_offset[g] + 8ull * rank;

    // the saved policy of the ply (agent/player.py:132, 366-385)
    const uint32_t n = root_n[((size_t)g * plies + j) * 64 + lane];
    float p;
    if (save_policy_of_tau_1 || (int)uni((uint32_t)H[j].turn) < change_tau_turn) {
        // the exact integer sum, which may pass 2^32, from two 16-bit halves (each at most 64 x 65535)
        const unsigned long long sum = ((unsigned long long)wave_sum_u32(n >> 16) << 16) + wave_sum_u32(n & 0xffffu);
        p = (float)((double)n / (double)sum);   // one f64 division, rounded once to f32 (sum == 0: the plain division, nan)
    } else {
        const uint32_t top = wave_max_u32(n);   // np.argmax: the first maximum
        p = lane == __ffsll((long long)__ballot(n == top)) - 1 ? 1.0f : 0.0f;
    }

    // policy: output square `lane` of symmetry (flip, rot) takes the square np.flipud (if flip) then np.rot90(k=-rot) bring there -
    // raz_emit.hip policy_permutation: a quarter turn reads (r, c) from (7 - c, r), the flip reads it from (7 - r, c), and the LAST
    // operation's map is applied to the output index first
    int idx = lane;
    for (int rot = 0; rot < 4; ++rot) {
        const float plain = __shfl(p, idx);
        const float flipped = __shfl(p, ((7 - (idx >> 3)) << 3) | (idx & 7));
        if (row0 + rot < capacity_rows) out_policy[(row0 + rot) * 64 + lane] = plain;
        if (row0 + 4 + rot < capacity_rows) out_policy[(row0 + 4 + rot) * 64 + lane] = flipped;
        idx = ((7 - (idx & 7)) << 3) | (idx >> 3);
    }

    // boards and z: lane s < 8 writes symmetry s = flip * 4 + rot
    if (lane < 8 && row0 + lane < capacity_rows) {
        raz_bb o = H[j].own, e = H[j].enemy;
        if (lane & 4) {
            o = bb_flip_vertical(o);
            e = bb_flip_vertical(e);
        }
        for (int k = 0; k < (lane & 3); ++k) {
            o = bb_rotate90(o);
            e = bb_rotate90(e);
        }
        const int winner = summary[g].status & 0x0f;
        const int black_win = winner == RAZ_WIN_BLACK ? 1 : (winner == RAZ_WIN_WHITE ? -1 : 0);
        out_own[row0 + lane] = o;
        out_enemy[row0 + lane] = e;
        out_z[row0 + lane] = (int8_t)(player == RAZ_PLAYER_BLACK ? black_win : -black_win);
    }
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// RAZ_OK, or the refusal both entries share
int check_extent(const char* who, uint32_t n_games, uint32_t plies) {
    static thread_local char msg[128];
    if (plies == 0) {
        snprintf(msg, sizeof msg, "%s: plies == 0", who);
        return raz_fail(RAZ_EINVAL, msg);
    }
    if ((unsigned long long)n_games * plies * 8ull >= (1ull << 32)) {
        snprintf(msg, sizeof msg, "%s: n_games * plies * 8 must stay below 2^32 (row numbers are 32-bit)", who);
        return raz_fail(RAZ_EINVAL, msg);
    }
    return RAZ_OK;
}

unsigned blocks_for(unsigned long long waves) { return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace

extern "C" int raz_train_rows_count(const void* d_headers, const raz_game_summary* d_summary, const uint8_t* d_done, uint32_t n_games,
                                    uint32_t plies, uint32_t* d_row_offset, uint64_t* total_rows, raz_stream_t stream) {
    if (!d_row_offset || misaligned(d_row_offset, 4)) return raz_fail(RAZ_EINVAL, "raz_train_rows_count: d_row_offset is NULL or not 4-byte aligned");
    if (int rc = check_extent("raz_train_rows_count", n_games, plies)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_games == 0) {
        RAZ_HIP_TRY(hipMemsetAsync(d_row_offset, 0, sizeof(uint32_t), s), "raz_train_rows_count: hipMemsetAsync");
    } else {
        if (!d_headers || !d_summary) return raz_fail(RAZ_EINVAL, "raz_train_rows_count: NULL array");
        if (misaligned(d_headers, 8) || misaligned(d_summary, 8)) return raz_fail(RAZ_EINVAL, "raz_train_rows_count: d_headers / d_summary must be 8-byte aligned");
        hipLaunchKernelGGL(k_rows_count, dim3(blocks_for(n_games)), dim3(64 * kWavesPerBlock), 0, s, (const raz_ply_header*)d_headers,
                           d_summary, d_done, n_games, plies, d_row_offset);
        if (int rc = raz_check_launch("raz_train_rows_count (k_rows_count)")) return rc;
        hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(kScanBlock), 0, s, d_row_offset, n_games);
        if (int rc = raz_check_launch("raz_train_rows_count (k_rows_scan)")) return rc;
    }
    if (total_rows) {
        uint32_t total = 0;
        RAZ_HIP_TRY(hipMemcpyAsync(&total, d_row_offset + n_games, sizeof total, hipMemcpyDeviceToHost, s), "raz_train_rows_count: hipMemcpyAsync");
        RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_train_rows_count: hipStreamSynchronize");
        *total_rows = total;
    }
    return RAZ_OK;
}

extern "C" int raz_train_rows_fill(const void* d_headers, const uint32_t* d_root_n, const raz_game_summary* d_summary, const uint8_t* d_done,
                                   uint32_t n_games, uint32_t plies, int change_tau_turn, int save_policy_of_tau_1,
                                   const uint32_t* d_row_offset, uint64_t capacity_rows, uint64_t* d_own, uint64_t* d_enemy,
                                   float* d_policy, int8_t* d_z, raz_stream_t stream) {
    if (int rc = check_extent("raz_train_rows_fill", n_games, plies)) return rc;
    if (n_games == 0) return RAZ_OK;
    if (!d_headers || !d_root_n || !d_summary || !d_row_offset || !d_own || !d_enemy || !d_policy || !d_z)
        return raz_fail(RAZ_EINVAL, "raz_train_rows_fill: NULL array");
    if (misaligned(d_headers, 8) || misaligned(d_summary, 8) || misaligned(d_own, 8) || misaligned(d_enemy, 8))
        return raz_fail(RAZ_EINVAL, "raz_train_rows_fill: d_headers / d_summary / d_own / d_enemy must be 8-byte aligned");
    if (misaligned(d_root_n, 4) || misaligned(d_row_offset, 4) || misaligned(d_policy, 4))
        return raz_fail(RAZ_EINVAL, "raz_train_rows_fill: d_root_n / d_row_offset / d_policy must be 4-byte aligned");
    if (capacity_rows == 0) return RAZ_OK;
    hipLaunchKernelGGL(k_rows_fill, dim3(blocks_for((unsigned long long)n_games * plies)), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream,
                       (const raz_ply_header*)d_headers, d_root_n, d_summary, d_done, n_games, plies, change_tau_turn, save_policy_of_tau_1,
                       d_row_offset, (unsigned long long)capacity_rows, (unsigned long long*)d_own, (unsigned long long*)d_enemy, d_policy,
                       d_z);
    return raz_check_launch("raz_train_rows_fill");
}
