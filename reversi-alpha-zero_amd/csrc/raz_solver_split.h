// raz_solver_split.h — the RECORD TREE that raz_solve_batch (raz_solver_batch.hip) and raz_solve_exact (raz_solver_exact.hip) split
// a batch into before their lanes search, stated once for the two: the workspace's header and record arrays, the record's meta
// word, the kernels around the search (classify, roots, expand + mark, fold, out), the host's sizing, argument checks,
// classification pass and chunk cut, and the per-wave task draw of the two search kernels.  What a solver adds is its own: its
// limits, its search kernel, its tuning word and its launch sequence.  Each solver names itself with a workspace type derived from
// SplitWs that carries, as compile-time constants,
//   kMaxEmpties  the most empties a row may have;
//   kAlways      the empties above which a record is always split, whatever the tuning: the bound on one lane's task;
//   kLinks       whether a record has the words `parent` and `bound` (the exact solver's sibling bounds);
//   kWho, kBytes the entry point's name (raz_last_error() names the call that failed) and its workspace-size function.
// Every launch here ends by construction: the grids are fixed-size and grid-stride, no wave waits for another wave or kernel - the
// record counter is the only word waves share inside a launch.  A record's children are found through the parent (first child,
// count), never through their own numbers' order across parents, so the answer does not depend on the order in which the atomics
// hand out records.
#pragma once
#include <cstdio>
#include <exception>
#include <vector>
#include "raz_internal.h"
#include "raz_solver_search.h"   // solver_play, solver_scan

namespace {

#define SPLIT_HDR_BYTES 256
#define SPLIT_LEVELS 8           // the roots, at most 6 plies of children, and the end of the last level
#define SPLIT_NONE 0xffffffffu   // no parent: a root
#define SPLIT_LOWEST (-66)       // below every value: a record's bound before a child has finished

// emp[] codes of a row that is not searched (a searched row: its empties)
#define SPLIT_ROW_NO_MOVE 0xF1
#define SPLIT_ROW_TOO_DEEP 0xF2
#define SPLIT_ROW_INVALID 0xF3

struct SplitHdr {                    // the first 256 bytes of the workspace
    unsigned long long visits;       // [0]  node visits (moves played by expand + the search) of the last call: include/raz.h
    uint32_t count;                  // [8]  records in use
    uint32_t next;                   // [12] next task = record number to look at
    uint32_t open;                   // [16] lanes that parked a task in the last launches (the exact solver's; unused by the batch)
    uint32_t overflow;               // [20] a run of children did not fit: the host's sizing was wrong
    uint32_t level[SPLIT_LEVELS];    // level p = records [level[p], level[p + 1])
};
static_assert(sizeof(SplitHdr) <= SPLIT_HDR_BYTES, "header");

struct SplitWs {                     // (a solver's own record words follow these, then `cap`: the records the arrays hold)
    SplitHdr* hdr;
    uint8_t* emp;                    // per ROW of the batch
    unsigned long long *own, *enemy; // per record: the position from its mover's view
    uint32_t *first, *meta;          // first child; the word below
};
// meta word of a record: bits 0-7 value + 128 (0 = not known yet), 8-15 best move + 1, 16-17 kind (0 the game ended on the way here:
// the value was known at once; 1 the parent's opponent moves here: parent's value = -f; 2 the parent's mover moves here - a pass,
// or a root: + f), 18 expanded, 19-23 children
__device__ __forceinline__ uint32_t rec_meta(int value, int move, int kind, int expanded, int nch) {
    return (uint32_t)(value + 128) | ((uint32_t)(move + 1) << 8) | ((uint32_t)kind << 16) | ((uint32_t)expanded << 18) | ((uint32_t)nch << 19);
}
__device__ __forceinline__ int rec_value(uint32_t m) { return (int)(m & 0xffu) - 128; }
__device__ __forceinline__ int rec_move(uint32_t m) { return (int)((m >> 8) & 0xffu) - 1; }
__device__ __forceinline__ int rec_kind(uint32_t m) { return (int)((m >> 16) & 3u); }
__device__ __forceinline__ bool rec_expanded(uint32_t m) { return (m >> 18) & 1u; }
__device__ __forceinline__ int rec_children(uint32_t m) { return (int)((m >> 19) & 31u); }

// The task draw of a search kernel: ONE atomic per wave hands a record number to each lane of `wanting` (wave-uniform, not empty).
// Returns the calling lane's number (meaningful for the lanes of `wanting`); `base` is the wave's first, the same in every lane.
__device__ __forceinline__ uint32_t solver_draw(uint32_t* next, unsigned long long wanting, int lane, uint32_t& base) {
    base = 0u;
    if (lane == 0) base = atomicAdd(next, (uint32_t)__popcll(wanting));
    base = (uint32_t)__builtin_amdgcn_readfirstlane(base);
    return base + (uint32_t)__popcll(wanting & ((1ULL << lane) - 1ULL));
}

constexpr int kBlock = 256;

// one thread per row: its status or its number of empty squares, into the workspace (no output byte yet)
template <class Ws>
__global__ __launch_bounds__(kBlock) void k_split_classify(Ws W, const unsigned long long* __restrict__ black, const unsigned long long* __restrict__ white,
                                                           const uint8_t* __restrict__ player, size_t n) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const raz_bb b = black[i], w = white[i];
        const int p = player[i];
        int code;
        if ((b & w) || (p != 1 && p != 2)) code = SPLIT_ROW_INVALID;
        else if (bb_popcount(~(b | w)) > Ws::kMaxEmpties) code = SPLIT_ROW_TOO_DEEP;
        else if (!bbv_legal_moves(p == 1 ? b : w, p == 1 ? w : b)) code = SPLIT_ROW_NO_MOVE;
        else code = bb_popcount(~(b | w));
        W.emp[i] = (uint8_t)code;
    }
}

// one RECORD per row of the chunk - a node: the position from its mover's view
template <class Ws>
__global__ __launch_bounds__(kBlock) void k_split_roots(Ws W, const unsigned long long* __restrict__ black, const unsigned long long* __restrict__ white,
                                                        const uint8_t* __restrict__ player, size_t r0, uint32_t rows) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const bool search = W.emp[r0 + i] <= Ws::kMaxEmpties;
        const bool is_black = player[r0 + i] == 1;
        W.own[i] = search ? (is_black ? black[r0 + i] : white[r0 + i]) : 0ULL;
        W.enemy[i] = search ? (is_black ? white[r0 + i] : black[r0 + i]) : 0ULL;
        W.first[i] = 0u;
        if constexpr (Ws::kLinks) {
            W.parent[i] = SPLIT_NONE;
            W.bound[i] = (uint32_t)(SPLIT_LOWEST + 128);
        }
        W.meta[i] = search ? rec_meta(RAZ_SOLVER_UNKNOWN, -1, 2, 0, 0) : rec_meta(-100, -1, 0, 0, 0);
    }
    // (nothing else reads or writes these words during this launch; `open` and `overflow` stand at 0: the call cleared the header,
    // the host clears `open` before every group of rounds, and a call that finds `overflow` raised ends there)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        W.hdr->count = rows;
        W.hdr->next = 0u;
        W.hdr->level[0] = 0u;
        W.hdr->level[1] = rows;
    }
}

// after the expansion of level p: level p + 1 ends where the record counter stands
template <class Ws>
__global__ __launch_bounds__(64) void k_split_mark(Ws W, int p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) W.hdr->level[p + 2] = W.hdr->count;
}

// ply by ply: a record of level p is SPLIT when it has more than kAlways empties (the bound on a lane's work: not a knob), or more
// than `leaf` and p < plies (the tuning's finer split).  It gets its children, in ASCENDING move order, as one contiguous run of
// records taken with an atomicAdd on the record counter.  A child the game ends at is a VALUE, a child the opponent passes at is a
// KIND of record (the value keeps its sign on the way up)
template <class Ws>
__global__ __launch_bounds__(kBlock) void k_split_expand(Ws W, int p, int leaf, int plies, uint32_t exact) {
    const uint32_t lo = W.hdr->level[p], hi = W.hdr->level[p + 1], stride = gridDim.x * kBlock;
    uint32_t visits = 0u;
    for (uint32_t i = lo + blockIdx.x * kBlock + threadIdx.x; i < hi; i += stride) {
        const uint32_t m = W.meta[i];
        if (rec_kind(m) == 0) continue;
        const raz_bb own = W.own[i], enemy = W.enemy[i];
        const int e = bb_popcount(~(own | enemy));
        if (!(e > Ws::kAlways || (e > leaf && p < plies))) continue;
        const raz_bb moves = bbv_legal_moves(own, enemy);
        const int nch = bb_popcount(moves);
        const uint32_t first = atomicAdd(&W.hdr->count, (uint32_t)nch);
        // (the host cuts the chunks by split_need, the most records their rows can take, so a run always fits; if one ever did not,
        // nothing is stored - the stores below stay inside the arrays whatever the counter holds - and the header says so)
        if (first + (uint32_t)nch > W.cap || first + (uint32_t)nch < first) {
            W.hdr->overflow = 1u;
            continue;
        }
        uint32_t c = first;
        for (raz_bb l = moves; l; l &= l - 1, ++c) {
            raz_bb no, ne, nm;
            int v;
            const int kind = solver_play(__ffsll((long long)l) - 1, own, enemy, no, ne, nm, v, exact != 0u);
            W.own[c] = no;
            W.enemy[c] = ne;
            W.first[c] = 0u;
            if constexpr (Ws::kLinks) {
                W.parent[c] = i;
                W.bound[c] = (uint32_t)(SPLIT_LOWEST + 128);
            }
            W.meta[c] = rec_meta(kind ? RAZ_SOLVER_UNKNOWN : v, -1, kind, 0, 0);
        }
        visits += (uint32_t)nch;
        W.first[i] = first;
        W.meta[i] = rec_meta(RAZ_SOLVER_UNKNOWN, -1, rec_kind(m), 1, nch);
    }
    if (visits) atomicAdd(&W.hdr->visits, (unsigned long long)visits);
}

// level by level, bottom up: the reference's loop over a node's moves (solver_scan: ascending, strict improvement) on the
// children's values (all of them are there; the ones behind a decided scan are not read)
template <class Ws>
__global__ __launch_bounds__(kBlock) void k_split_fold(Ws W, int p, uint32_t exact) {
    const uint32_t lo = W.hdr->level[p], hi = W.hdr->level[p + 1], stride = gridDim.x * kBlock;
    for (uint32_t i = lo + blockIdx.x * kBlock + threadIdx.x; i < hi; i += stride) {
        const uint32_t m = W.meta[i];
        if (!rec_expanded(m)) continue;
        const int nch = rec_children(m);
        const uint32_t first = W.first[i];
        int bm, bs;
        solver_scan([&](int j) { return rec_value(W.meta[first + j]); }, nch, bbv_legal_moves(W.own[i], W.enemy[i]), exact != 0u, bm, bs);
        W.meta[i] = rec_meta(rec_kind(m) == 1 ? -bs : bs, bm, rec_kind(m), 1, nch);
    }
}

// the chunk's rows of d_move / d_score / d_status
template <class Ws>
__global__ __launch_bounds__(kBlock) void k_split_out(Ws W, size_t r0, uint32_t rows, int8_t* __restrict__ move, int8_t* __restrict__ score,
                                                      uint8_t* __restrict__ status) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const int code = W.emp[r0 + i];
        const uint32_t m = W.meta[i];
        const bool search = code <= Ws::kMaxEmpties;
        move[r0 + i] = (int8_t)(search ? rec_move(m) : -1);
        score[r0 + i] = (int8_t)(search ? rec_value(m) : -100);
        status[r0 + i] = (uint8_t)(search ? 0 : code - 0xF0);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the plies a row of e empties is expanded for (k_split_expand's rule): down to `leaf` empties but for at most `plies` plies, and
// in any case down to `always`
int split_plies(int e, int leaf, int plies, int always) {
    const int asked = e > leaf ? (e - leaf < plies ? e - leaf : plies) : 0, forced = e > always ? e - always : 0;
    return asked > forced ? asked : forced;
}
// the most records such a row can need: level k holds at most e (e - 1) ... (e - k + 1) nodes (a move fills a square, whoever
// plays it)
size_t split_need(int e, int leaf, int plies, int always) {
    const int k_max = split_plies(e, leaf, plies, always);
    size_t total = 1, level = 1;
    for (int k = 0; k < k_max; ++k) {
        level *= (size_t)(e - k);
        total += level;
    }
    return total;
}
size_t split_fixed_bytes(size_t n) { return SPLIT_HDR_BYTES + (n + 255) / 256 * 256; }
unsigned split_grid(size_t items, unsigned per, unsigned most) {
    const size_t g = (items + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > most ? most : g));
}
// the header and the rows' codes at the front of the workspace, `cap` records from `records` on
template <class Ws>
void split_layout(Ws& W, unsigned char* base, unsigned char* records, size_t cap) {
    W.hdr = (SplitHdr*)base;
    W.emp = base + SPLIT_HDR_BYTES;
    W.own = (unsigned long long*)records;
    W.enemy = W.own + cap;
    W.first = (uint32_t*)(W.enemy + cap);
    W.meta = W.first + cap;
    W.cap = (uint32_t)cap;
}

// an error text that names the entry point: `fmt` with every %s = who
struct SplitText {
    char text[160];
    SplitText(const char* fmt, const char* who) { snprintf(text, sizeof text, fmt, who, who); }
    operator const char*() const { return text; }
};

// the checks both entry points make on their arrays (after their own tuning checks and n == 0)
template <class Ws>
int split_check_args(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, const int8_t* d_move,
                     const int8_t* d_score, const uint8_t* d_status, const void* d_workspace, size_t workspace_bytes) {
    if (!d_black || !d_white || !d_player || !d_move || !d_score || !d_status || !d_workspace)
        return raz_fail(RAZ_EINVAL, SplitText("%s: NULL array", Ws::kWho));
    if (((uintptr_t)d_black | (uintptr_t)d_white) & 7u) return raz_fail(RAZ_EINVAL, SplitText("%s: bitboard arrays must be 8-byte aligned", Ws::kWho));
    if ((uintptr_t)d_workspace & 255u) return raz_fail(RAZ_EINVAL, SplitText("%s: the workspace must be 256-byte aligned", Ws::kWho));
    const size_t least = Ws::kBytes(n, 0);
    if (least == 0) return raz_fail(RAZ_EINVAL, SplitText("%s: n too large", Ws::kWho));
    if (workspace_bytes < least) return raz_fail(RAZ_EINVAL, SplitText("%s: workspace smaller than %s_workspace_bytes(n, 0)", Ws::kWho));
    return RAZ_OK;
}

// the classification pass, with the call's one synchronisation that every batch needs: `emp` = the rows' codes, read back.  Fails
// - before any output byte is written - when the workspace is smaller than the deepest searched row asks for
template <class Ws>
int split_classify(const Ws& W, const unsigned long long* bl, const unsigned long long* wh, const uint8_t* d_player, size_t n,
                   size_t workspace_bytes, hipStream_t s, std::vector<uint8_t>& emp) {
    RAZ_HIP_TRY(hipMemsetAsync(W.hdr, 0, SPLIT_HDR_BYTES, s), SplitText("%s (clear)", Ws::kWho));
    hipLaunchKernelGGL(k_split_classify<Ws>, dim3(split_grid(n, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, n);
    if (int rc = raz_check_launch(SplitText("%s (classify)", Ws::kWho))) return rc;
    try {
        emp.resize(n);
    } catch (const std::exception&) {   // (nothing may be thrown through the C boundary)
        return raz_fail(RAZ_ENOMEM, SplitText("%s: no host memory for the rows' empties", Ws::kWho));
    }
    RAZ_HIP_TRY(hipMemcpyAsync(emp.data(), W.emp, n, hipMemcpyDeviceToHost, s), SplitText("%s (read the rows' empties)", Ws::kWho));
    RAZ_HIP_TRY(hipStreamSynchronize(s), SplitText("%s (synchronise)", Ws::kWho));
    int deepest = 0;
    for (size_t i = 0; i < n; ++i)
        if (emp[i] <= Ws::kMaxEmpties && emp[i] > deepest) deepest = emp[i];
    if (workspace_bytes < Ws::kBytes(n, deepest))
        return raz_fail(RAZ_EINVAL, SplitText("%s: workspace smaller than %s_workspace_bytes(n, the most empties of a row)", Ws::kWho));
    return RAZ_OK;
}

// The chunk that starts at row r0: as many rows [r0, r1) as `cap` records hold in the worst case (a row that is not searched still
// has its record; the first row is taken whatever it needs) and at most chunk_rows of them (0: no such limit); `used` = that worst
// case, `plies` = the deepest split among the rows
struct SplitChunk {
    size_t r1, used;
    int plies;
};
template <class Ws>
SplitChunk split_chunk(const std::vector<uint8_t>& emp, size_t r0, int leaf, int plies, size_t cap, size_t chunk_rows) {
    SplitChunk c{r0, 0, 0};
    while (c.r1 < emp.size() && (chunk_rows == 0 || c.r1 - r0 < chunk_rows)) {
        const int e = emp[c.r1] <= Ws::kMaxEmpties ? emp[c.r1] : 0;
        const size_t need = split_need(e, leaf, plies, Ws::kAlways);
        if (c.used + need > cap && c.r1 > r0) break;
        c.used += need;
        const int k = split_plies(e, leaf, plies, Ws::kAlways);
        if (k > c.plies) c.plies = k;
        ++c.r1;
    }
    return c;
}

}  // namespace
