// raz_solver_batch.hip — raz_solve_batch (include/raz.h): ReversiSolver.solve (lib/alt/reversi_solver_cython.pyx:40-127) for a BATCH
// of independent positions, outside any engine.
//
// The pool of raz_solver_pool.h answers one request per game and therefore spreads every solve over many lanes, hands it across
// kernels and shares a memo.  A batch is the opposite case and needs none of that.  The host cuts it into CHUNKS whose worst-case
// split fits the workspace, and a chunk runs
//   the split   raz_solver_split.h's kernels, shared with raz_solver_exact.hip: classify, roots, expand ply by ply (every record
//               of more than 8 empties and, for the first `plies` plies, every one of more than `leaf`);
//   k_sb_leaves one task per LANE: every record that was not expanded is a subtree of <= 8 empties, searched depth first with the
//               node in registers and the ancestors' frames in LDS ([level][word][lane]), one move per iteration, the last empty
//               square finished inside the move function.  A wave draws tasks for ALL its idle lanes with one atomicAdd (every
//               8th iteration, or at once when the whole wave is idle) and stops drawing when the counter has passed the end;
//   the fold and the output rows, raz_solver_split.h's again.
// Every launch ends by construction, under every `tuning`: a task is a subtree of at most 8 empties (<= 109 601 node visits) - the
// tuning can ask for MORE splitting than that (a smaller leaf), and it can stop the extra splitting after some plies, but a record
// of more than 8 empties is always expanded, so no tuning puts more than that on a lane.  The answer is f(position, mode) - the
// recursion in oracle/orc_solver.c - whatever the chunks, the leaf size, the number of plies split or the order in which the
// atomics hand out records.  In win/loss mode subtrees the sequential scan would have skipped are searched too; their values are
// never read (the fold's scan stops where the reference's stops).  No memo.  The search itself (the move function, the scan, a
// lane's node and its frame word) is raz_solver_search.h's, the same statement the pool's lanes run.  Measurements: DESIGN.md 4.7.
#include "raz_solver_split.h"

namespace {

#define SB_MAX_EMPTIES 14
#define SB_MAX_LEAF 8        // a lane's subtree: <= 8 empties
#define SB_MIN_LEAF 2
#define SB_MAX_PLIES 6       // 14 - 8: plies the split may go down
#define SB_REC_BYTES 24
#define SB_TUNING_MASK 0x00ffffffu
static_assert(SB_MAX_PLIES + 2 <= SPLIT_LEVELS, "levels");

struct SbWs : SplitWs {
    static constexpr int kMaxEmpties = SB_MAX_EMPTIES, kAlways = SB_MAX_LEAF;
    static constexpr bool kLinks = false;
    static constexpr const char* kWho = "raz_solve_batch";
    static constexpr auto kBytes = raz_solve_batch_workspace_bytes;
    uint32_t cap;
};

// FRAMES: the deepest stack a task needs - a node has at least two empty squares (the last one is finished by solver_play), so a
// task of e <= SB_MAX_LEAF empties pushes at most e - 2 frames
constexpr int FRAMES = SB_MAX_LEAF - 2;
static_assert(RAZ_SOLVER_INLINE_LAST >= 1, "FRAMES rests on solver_play finishing the last empty square itself");
struct SbFrames {   // a lane's column of the wave's frames: level d = three 8-byte words (own, enemy, moves left) and SolverNode's frame word
    unsigned long long* f64;   // word j of level d: f64[(d * 3 + j) * 64]
    uint32_t* f32;             // f32[d * 64]
    __device__ __forceinline__ void put(int d, raz_bb own, raz_bb enemy, raz_bb left, uint32_t word) const {
        f64[(d * 3 + 0) * 64] = own;
        f64[(d * 3 + 1) * 64] = enemy;
        f64[(d * 3 + 2) * 64] = left;
        f32[d * 64] = word;
    }
    __device__ __forceinline__ void get(int d, raz_bb& own, raz_bb& enemy, raz_bb& left, uint32_t& word) const {
        own = f64[(d * 3 + 0) * 64];
        enemy = f64[(d * 3 + 1) * 64];
        left = f64[(d * 3 + 2) * 64];
        word = f32[d * 64];
    }
};
__global__ __launch_bounds__(64) void k_sb_leaves(SbWs W, uint32_t exact) {
    __shared__ unsigned long long fr64[FRAMES * 3 * 64];
    __shared__ uint32_t fr32[FRAMES * 64];
    const int lane = threadIdx.x;
    const SbFrames frames{fr64 + lane, fr32 + lane};
    const uint32_t total = W.hdr->count < W.cap ? W.hdr->count : W.cap;
    bool have = false, dry = false;
    SolverNode nd;   // the node the lane's search stands on
    nd.begin(0ULL, 0ULL, 0ULL);
    int d = 0;
    uint32_t task = 0u, task_meta = 0u;
    unsigned long long visits = 0ULL;
    for (uint32_t it = 0u;; ++it) {
        const unsigned long long idle = __ballot(!have);
        if (idle == ~0ULL && dry) break;
        if (!dry && idle && (idle == ~0ULL || (it & 7u) == 0u)) {
            // a record number for each idle lane; a record that is no task (a value, an expanded node) leaves its lane idle until
            // the next draw
            uint32_t base;
            const uint32_t t = solver_draw(&W.hdr->next, idle, lane, base);
            if (base >= total) dry = true;
            if (!have && t < total) {
                const uint32_t m = W.meta[t];
                if (rec_kind(m) != 0 && !rec_expanded(m)) {
                    task = t;
                    task_meta = m;
                    const raz_bb own = W.own[t], enemy = W.enemy[t];
                    nd.begin(own, enemy, bbv_legal_moves(own, enemy));
                    d = 0;
                    have = true;
                }
            }
        }
        if (have) {
            // finished nodes hand their value to their parents (at most two per iteration: the wave runs as many rounds of this
            // loop as its deepest unwinding lane needs), then the node the search stands on plays its next move
            bool may_move = false;
            for (int returns = 0; returns <= 2; ++returns) {
                if (!nd.finished(exact != 0u)) {
                    may_move = true;
                    break;
                }
                if (returns == 2) break;
                if (d == 0) {
                    W.meta[task] = rec_meta(rec_kind(task_meta) == 1 ? -nd.bsc : nd.bsc, nd.bmv, rec_kind(task_meta), 0, 0);
                    have = false;
                    break;
                }
                nd.give_to_parent(frames, d, nd.bsc);
            }
            if (have && may_move) {
                // (d < FRAMES always holds: see above; the test keeps the stores inside the arrays)
                nd.play_next(frames, d, exact != 0u, d < FRAMES);
                ++visits;
            }
        }
    }
    for (int s = 1; s < 64; s <<= 1) visits += __shfl_xor(visits, s);
    if (lane == 0 && visits) atomicAdd(&W.hdr->visits, visits);
}

}  // namespace

extern "C" size_t raz_solve_batch_workspace_bytes(size_t n, int max_empties) {
    if (max_empties > SB_MAX_EMPTIES || n > ((size_t)1 << 31)) return 0;
    if (max_empties < 0) max_empties = 0;
    // the worst split any `tuning` can ask for: the smallest leaf size, all the plies
    size_t rec = split_need(max_empties, SB_MIN_LEAF, SB_MAX_PLIES, SB_MAX_LEAF);
    if (rec < 256) rec = 256;
    return split_fixed_bytes(n) + rec * SB_REC_BYTES;
}

extern "C" int raz_solve_batch(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int exactly,
                               int8_t* d_move, int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes,
                               uint32_t tuning, raz_stream_t stream) {
    if (tuning & ~SB_TUNING_MASK) return raz_fail(RAZ_EINVAL, "raz_solve_batch: unknown tuning bits");
    const int leaf = (tuning & 15u) ? (int)(tuning & 15u) : SB_MAX_LEAF;
    const int plies = ((tuning >> 4) & 15u) ? (int)((tuning >> 4) & 15u) - 1 : SB_MAX_PLIES;
    const size_t chunk_rows = (tuning >> 8) & 0xffffu;
    if (leaf < SB_MIN_LEAF || leaf > SB_MAX_LEAF) return raz_fail(RAZ_EINVAL, "raz_solve_batch: tuning: leaf size must be 2..8");
    if (plies > SB_MAX_PLIES) return raz_fail(RAZ_EINVAL, "raz_solve_batch: tuning: at most 6 plies are split");
    if (n == 0) return RAZ_OK;
    if (int rc = split_check_args<SbWs>(d_black, d_white, d_player, n, d_move, d_score, d_status, d_workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t fixed = split_fixed_bytes(n);
    size_t cap = (workspace_bytes - fixed) / SB_REC_BYTES;
    if (cap > 0xfffffff0u) cap = 0xfffffff0u;   // record numbers are 32-bit
    SbWs W;
    split_layout(W, (unsigned char*)d_workspace, (unsigned char*)d_workspace + fixed, cap);
    const unsigned long long *bl = (const unsigned long long*)d_black, *wh = (const unsigned long long*)d_white;
    const uint32_t exact = (uint32_t)(exactly != 0);
    std::vector<uint8_t> emp;
    if (int rc = split_classify(W, bl, wh, d_player, n, workspace_bytes, s, emp)) return rc;

    for (size_t r0 = 0; r0 < n;) {
        const SplitChunk c = split_chunk<SbWs>(emp, r0, leaf, plies, cap, chunk_rows);
        const uint32_t rows = (uint32_t)(c.r1 - r0);
        hipLaunchKernelGGL(k_split_roots<SbWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, r0, rows);
        for (int p = 0; p < c.plies; ++p) {
            hipLaunchKernelGGL(k_split_expand<SbWs>, dim3(split_grid(c.used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, leaf, plies, exact);
            hipLaunchKernelGGL(k_split_mark<SbWs>, dim3(1), dim3(64), 0, s, W, p);
        }
        hipLaunchKernelGGL(k_sb_leaves, dim3(split_grid(c.used, 64, 3072)), dim3(64), 0, s, W, exact);
        for (int p = c.plies - 1; p >= 0; --p)
            hipLaunchKernelGGL(k_split_fold<SbWs>, dim3(split_grid(c.used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, exact);
        hipLaunchKernelGGL(k_split_out<SbWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, r0, rows, d_move, d_score, d_status);
        if (int rc = raz_check_launch("raz_solve_batch")) return rc;
        r0 = c.r1;
    }
    return RAZ_OK;
}
