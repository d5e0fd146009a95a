// raz_solver_batch.hip — raz_solve_batch (include/raz.h): ReversiSolver.solve (lib/alt/reversi_solver_cython.pyx:40-127) for a BATCH
// of independent positions, outside any engine.
//
// The pool of raz_solver_pool.h answers one request per game and therefore spreads every solve over many lanes, hands it across
// kernels and shares a memo.  A batch is the opposite case and needs none of that:
//   k_sb_classify  one thread per row: its status and its number of empty squares, into the workspace (no output byte yet);
//   (the host reads the rows' empties and cuts the batch into CHUNKS whose worst-case split fits the workspace)
//   k_sb_roots     one RECORD per row of the chunk - a node: the position from its mover's view;
//   k_sb_expand    ply by ply: every record of the last level with more than 8 empties - and, for the first `plies` plies, every one
//                  with more than `leaf` - gets its children, in ascending move
//                  order, as one contiguous run of records taken with an atomicAdd on the record counter.  A child the game ends
//                  at is a VALUE, a child the opponent passes at is a KIND of record (the value keeps its sign on the way up);
//   k_sb_leaves    one task per LANE: every record that was not expanded is a subtree of <= 8 empties, searched depth first
//                  with the node in registers and the ancestors' frames in LDS ([level][word][lane]), one move per iteration,
//                  the last empty square finished inside the move function.  A wave draws tasks for ALL its idle lanes with one
//                  atomicAdd (every 8th iteration, or at once when the whole wave is idle) and stops drawing when the counter
//                  has passed the end;
//   k_sb_fold      level by level, bottom up: a parent runs the reference's scan over its children's values;
//   k_sb_out       the chunk's rows of d_move / d_score / d_status.
// Every launch ends by construction, under every `tuning`: a task is a subtree of at most 8 empties (<= 109 601 node visits) - the
// tuning can ask for MORE splitting than that (a smaller leaf), and it can stop the extra splitting after some plies, but a record
// of more than 8 empties is always expanded, so no tuning puts more than that on a lane.  Grids
// are fixed-size and grid-stride, no wave waits for another wave or kernel - the record counter and the task counter are the only
// words waves share inside a launch.  The answer is f(position, mode) - the recursion in oracle/orc_solver.c - whatever the chunks,
// the leaf size, the number of plies split or the order in which the atomics hand out records: a record's children are found
// through the parent (first child, count), never through their own numbers' order across parents.  In win/loss mode subtrees the
// sequential scan would have skipped are searched too; their values are never read (the fold's scan stops where the reference's
// stops).  No memo.  The search itself (the move function, the scan, a lane's node and its frame word) is raz_solver_search.h's,
// the same statement the pool's lanes run: one statement, two drivers.  Measurements: DESIGN.md 4.7.
#include <exception>
#include <vector>
#include "raz_internal.h"
#include "raz_solver_search.h"   // the per-lane search itself: solver_play, solver_scan, SolverNode (shared with raz_solver_pool.h)

namespace {

#define SB_MAX_EMPTIES 14
#define SB_MAX_LEAF 8        // a lane's subtree: <= 8 empties
#define SB_MIN_LEAF 2
#define SB_MAX_PLIES 6       // 14 - 8: plies the split may go down
#define SB_UNKNOWN RAZ_SOLVER_UNKNOWN
#define SB_HDR_BYTES 256
#define SB_REC_BYTES 24
#define SB_TUNING_MASK 0x00ffffffu

// emp[] codes of a row that is not searched (a searched row: its empties, 0..14)
#define SB_ROW_NO_MOVE 0xF1
#define SB_ROW_TOO_DEEP 0xF2
#define SB_ROW_INVALID 0xF3

struct SbHdr {                       // the first 256 bytes of the workspace
    unsigned long long visits;       // [0]  node visits (moves played by expand + leaves) of the last call: include/raz.h
    uint32_t count;                  // [8]  records in use
    uint32_t next;                   // [12] next task = record number to look at
    uint32_t level[SB_MAX_PLIES + 2];   // level p = records [level[p], level[p + 1])
};
static_assert(sizeof(SbHdr) <= SB_HDR_BYTES, "header");

// meta word of a record: bits 0-7 value + 128 (0 = not known yet), 8-15 best move + 1, 16-17 kind (0 the game ended on the way here:
// the value was known at once; 1 the parent's opponent moves here: parent's value = -f; 2 the parent's mover moves here - a pass,
// or a root: + f), 18 expanded, 19-23 children
struct SbWs {
    SbHdr* hdr;
    uint8_t* emp;                    // per ROW of the batch
    unsigned long long *own, *enemy; // per record: the position from its mover's view
    uint32_t *first, *meta;          // first child; the word above
    uint32_t cap;                    // records the arrays hold
};
__device__ __forceinline__ uint32_t sb_meta(int value, int move, int kind, int expanded, int nch) {
    return (uint32_t)(value + 128) | ((uint32_t)(move + 1) << 8) | ((uint32_t)kind << 16) | ((uint32_t)expanded << 18) | ((uint32_t)nch << 19);
}
__device__ __forceinline__ int sb_value(uint32_t m) { return (int)(m & 0xffu) - 128; }
__device__ __forceinline__ int sb_kind(uint32_t m) { return (int)((m >> 16) & 3u); }

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_sb_classify(SbWs W, const unsigned long long* __restrict__ black, const unsigned long long* __restrict__ white,
                                                        const uint8_t* __restrict__ player, size_t n) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const raz_bb b = black[i], w = white[i];
        const int p = player[i];
        int code;
        if ((b & w) || (p != 1 && p != 2)) code = SB_ROW_INVALID;
        else if (bb_popcount(~(b | w)) > SB_MAX_EMPTIES) code = SB_ROW_TOO_DEEP;
        else if (!bbv_legal_moves(p == 1 ? b : w, p == 1 ? w : b)) code = SB_ROW_NO_MOVE;
        else code = bb_popcount(~(b | w));
        W.emp[i] = (uint8_t)code;
    }
}

__global__ __launch_bounds__(kBlock) void k_sb_roots(SbWs W, const unsigned long long* __restrict__ black, const unsigned long long* __restrict__ white,
                                                     const uint8_t* __restrict__ player, size_t r0, uint32_t rows) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const bool search = W.emp[r0 + i] <= SB_MAX_EMPTIES;
        const bool is_black = player[r0 + i] == 1;
        W.own[i] = search ? (is_black ? black[r0 + i] : white[r0 + i]) : 0ULL;
        W.enemy[i] = search ? (is_black ? white[r0 + i] : black[r0 + i]) : 0ULL;
        W.first[i] = 0u;
        W.meta[i] = search ? sb_meta(SB_UNKNOWN, -1, 2, 0, 0) : sb_meta(-100, -1, 0, 0, 0);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // (nothing else reads or writes these words during this launch)
        W.hdr->count = rows;
        W.hdr->next = 0u;
        W.hdr->level[0] = 0u;
        W.hdr->level[1] = rows;
    }
}

// after the expansion of level p: level p + 1 ends where the record counter stands
__global__ __launch_bounds__(64) void k_sb_mark(SbWs W, int p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) W.hdr->level[p + 2] = W.hdr->count;
}

// a record of level p is expanded when it has more than SB_MAX_LEAF empties (the bound on a lane's work: whatever the tuning), or
// more than `leaf` and p < plies (a finer split: the default leaf is SB_MAX_LEAF, where both say the same)
__global__ __launch_bounds__(kBlock) void k_sb_expand(SbWs W, int p, int leaf, int plies, uint32_t exact) {
    const uint32_t lo = W.hdr->level[p], hi = W.hdr->level[p + 1], stride = gridDim.x * kBlock;
    uint32_t visits = 0u;
    for (uint32_t i = lo + blockIdx.x * kBlock + threadIdx.x; i < hi; i += stride) {
        const uint32_t m = W.meta[i];
        if (sb_kind(m) == 0) continue;
        const raz_bb own = W.own[i], enemy = W.enemy[i];
        const int e = bb_popcount(~(own | enemy));
        if (e <= leaf || (p >= plies && e <= SB_MAX_LEAF)) continue;
        const raz_bb moves = bbv_legal_moves(own, enemy);
        const int nch = bb_popcount(moves);
        const uint32_t first = atomicAdd(&W.hdr->count, (uint32_t)nch);
        // (the host cuts the chunks by sb_need, the most records their rows can take, so a run always fits; the test only keeps
        // the stores below inside the arrays whatever the counter holds)
        if (first + (uint32_t)nch > W.cap || first + (uint32_t)nch < first) continue;
        uint32_t c = first;
        for (raz_bb l = moves; l; l &= l - 1, ++c) {
            raz_bb no, ne, nm;
            int v;
            const int kind = solver_play(__ffsll((long long)l) - 1, own, enemy, no, ne, nm, v, exact != 0u);
            W.own[c] = no;
            W.enemy[c] = ne;
            W.first[c] = 0u;
            W.meta[c] = sb_meta(kind ? SB_UNKNOWN : v, -1, kind, 0, 0);
        }
        visits += (uint32_t)nch;
        W.first[i] = first;
        W.meta[i] = sb_meta(SB_UNKNOWN, -1, sb_kind(m), 1, nch);
    }
    if (visits) atomicAdd(&W.hdr->visits, (unsigned long long)visits);
}

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
            // ONE atomic per wave hands a record number to each idle lane; a record that is no task (a value, an expanded node)
            // leaves its lane idle until the next draw
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(&W.hdr->next, (uint32_t)__popcll(idle));
            base = (uint32_t)__builtin_amdgcn_readfirstlane(base);
            if (base >= total) dry = true;
            const uint32_t t = base + (uint32_t)__popcll(idle & ((1ULL << lane) - 1ULL));
            if (!have && t < total) {
                const uint32_t m = W.meta[t];
                if (sb_kind(m) != 0 && !((m >> 18) & 1u)) {
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
                    W.meta[task] = sb_meta(sb_kind(task_meta) == 1 ? -nd.bsc : nd.bsc, nd.bmv, sb_kind(task_meta), 0, 0);
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

// level p: the reference's loop over a node's moves (solver_scan) on the children's values (all of them are there; the ones
// behind a decided scan are not read)
__global__ __launch_bounds__(kBlock) void k_sb_fold(SbWs W, int p, uint32_t exact) {
    const uint32_t lo = W.hdr->level[p], hi = W.hdr->level[p + 1], stride = gridDim.x * kBlock;
    for (uint32_t i = lo + blockIdx.x * kBlock + threadIdx.x; i < hi; i += stride) {
        const uint32_t m = W.meta[i];
        if (!((m >> 18) & 1u)) continue;
        const int nch = (int)((m >> 19) & 31u);
        const uint32_t first = W.first[i];
        int bm, bs;
        solver_scan([&](int j) { return sb_value(W.meta[first + j]); }, nch, bbv_legal_moves(W.own[i], W.enemy[i]), exact != 0u, bm, bs);
        W.meta[i] = sb_meta(sb_kind(m) == 1 ? -bs : bs, bm, sb_kind(m), 1, nch);
    }
}

__global__ __launch_bounds__(kBlock) void k_sb_out(SbWs W, size_t r0, uint32_t rows, int8_t* __restrict__ move, int8_t* __restrict__ score,
                                                   uint8_t* __restrict__ status) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const int code = W.emp[r0 + i];
        const uint32_t m = W.meta[i];
        const bool search = code <= SB_MAX_EMPTIES;
        move[r0 + i] = (int8_t)(search ? (int)((m >> 8) & 0xffu) - 1 : -1);
        score[r0 + i] = (int8_t)(search ? sb_value(m) : -100);
        status[r0 + i] = (uint8_t)(search ? 0 : code - 0xF0);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the plies a row of e empties is expanded for (k_sb_expand's rule): down to `leaf` empties but for at most `plies` plies, and
// in any case down to SB_MAX_LEAF
int sb_plies(int e, int leaf, int plies) {
    const int asked = e > leaf ? (e - leaf < plies ? e - leaf : plies) : 0, bound = e > SB_MAX_LEAF ? e - SB_MAX_LEAF : 0;
    return asked > bound ? asked : bound;
}
// the most records such a row can need: level k holds at most e (e - 1) ... (e - k + 1) nodes (a move fills a square, whoever
// plays it)
size_t sb_need(int e, int leaf, int plies) {
    const int k_max = sb_plies(e, leaf, plies);
    size_t total = 1, level = 1;
    for (int k = 0; k < k_max; ++k) {
        level *= (size_t)(e - k);
        total += level;
    }
    return total;
}
size_t sb_fixed_bytes(size_t n) { return SB_HDR_BYTES + (n + 255) / 256 * 256; }
unsigned sb_grid(size_t items, unsigned per, unsigned most) {
    const size_t g = (items + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > most ? most : g));
}

}  // namespace

extern "C" size_t raz_solve_batch_workspace_bytes(size_t n, int max_empties) {
    if (max_empties > SB_MAX_EMPTIES || n > ((size_t)1 << 31)) return 0;
    if (max_empties < 0) max_empties = 0;
    // the worst split any `tuning` can ask for: the smallest leaf size, all the plies
    size_t rec = sb_need(max_empties, SB_MIN_LEAF, SB_MAX_PLIES);
    if (rec < 256) rec = 256;
    return sb_fixed_bytes(n) + rec * SB_REC_BYTES;
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
    if (!d_black || !d_white || !d_player || !d_move || !d_score || !d_status || !d_workspace)
        return raz_fail(RAZ_EINVAL, "raz_solve_batch: NULL array");
    if (((uintptr_t)d_black | (uintptr_t)d_white) & 7u) return raz_fail(RAZ_EINVAL, "raz_solve_batch: bitboard arrays must be 8-byte aligned");
    if ((uintptr_t)d_workspace & 255u) return raz_fail(RAZ_EINVAL, "raz_solve_batch: the workspace must be 256-byte aligned");
    const size_t least = raz_solve_batch_workspace_bytes(n, 0);
    if (least == 0) return raz_fail(RAZ_EINVAL, "raz_solve_batch: n too large");
    if (workspace_bytes < least) return raz_fail(RAZ_EINVAL, "raz_solve_batch: workspace smaller than raz_solve_batch_workspace_bytes(n, 0)");
    hipStream_t s = (hipStream_t)stream;
    const size_t fixed = sb_fixed_bytes(n);
    size_t cap = (workspace_bytes - fixed) / SB_REC_BYTES;
    if (cap > 0xfffffff0u) cap = 0xfffffff0u;   // record numbers are 32-bit
    SbWs W;
    unsigned char* base = (unsigned char*)d_workspace;
    W.hdr = (SbHdr*)base;
    W.emp = base + SB_HDR_BYTES;
    W.own = (unsigned long long*)(base + fixed);
    W.enemy = W.own + cap;
    W.first = (uint32_t*)(W.enemy + cap);
    W.meta = W.first + cap;
    W.cap = (uint32_t)cap;
    const unsigned long long *bl = (const unsigned long long*)d_black, *wh = (const unsigned long long*)d_white;

    RAZ_HIP_TRY(hipMemsetAsync(base, 0, SB_HDR_BYTES, s), "raz_solve_batch (clear)");
    hipLaunchKernelGGL(k_sb_classify, dim3(sb_grid(n, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, n);
    if (int rc = raz_check_launch("raz_solve_batch (classify)")) return rc;
    std::vector<uint8_t> emp;
    try {
        emp.resize(n);
    } catch (const std::exception&) {   // (nothing may be thrown through the C boundary)
        return raz_fail(RAZ_ENOMEM, "raz_solve_batch: no host memory for the rows' empties");
    }
    RAZ_HIP_TRY(hipMemcpyAsync(emp.data(), W.emp, n, hipMemcpyDeviceToHost, s), "raz_solve_batch (read the rows' empties)");
    RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_solve_batch (synchronise)");
    int deepest = 0;
    for (size_t i = 0; i < n; ++i)
        if (emp[i] <= SB_MAX_EMPTIES && emp[i] > deepest) deepest = emp[i];
    if (workspace_bytes < raz_solve_batch_workspace_bytes(n, deepest))   // (no output byte has been written)
        return raz_fail(RAZ_EINVAL, "raz_solve_batch: workspace smaller than raz_solve_batch_workspace_bytes(n, the most empties of a row)");

    for (size_t r0 = 0; r0 < n;) {
        // the chunk: as many rows as the records hold in the worst case (a row that is not searched still has its record)
        size_t used = 0, r1 = r0;
        int chunk_plies = 0;
        while (r1 < n && (chunk_rows == 0 || r1 - r0 < chunk_rows)) {
            const int e = emp[r1] <= SB_MAX_EMPTIES ? emp[r1] : 0;
            const size_t need = sb_need(e, leaf, plies);
            if (used + need > cap && r1 > r0) break;
            used += need;
            const int k = sb_plies(e, leaf, plies);
            if (k > chunk_plies) chunk_plies = k;
            ++r1;
        }
        const uint32_t rows = (uint32_t)(r1 - r0);
        hipLaunchKernelGGL(k_sb_roots, dim3(sb_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, r0, rows);
        for (int p = 0; p < chunk_plies; ++p) {
            hipLaunchKernelGGL(k_sb_expand, dim3(sb_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, leaf, plies, (uint32_t)(exactly != 0));
            hipLaunchKernelGGL(k_sb_mark, dim3(1), dim3(64), 0, s, W, p);
        }
        hipLaunchKernelGGL(k_sb_leaves, dim3(sb_grid(used, 64, 3072)), dim3(64), 0, s, W, (uint32_t)(exactly != 0));
        for (int p = chunk_plies - 1; p >= 0; --p)
            hipLaunchKernelGGL(k_sb_fold, dim3(sb_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, (uint32_t)(exactly != 0));
        hipLaunchKernelGGL(k_sb_out, dim3(sb_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, r0, rows, d_move, d_score, d_status);
        if (int rc = raz_check_launch("raz_solve_batch")) return rc;
        r0 = r1;
    }
    return RAZ_OK;
}
