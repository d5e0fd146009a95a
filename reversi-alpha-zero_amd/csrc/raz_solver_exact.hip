// raz_solver_exact.hip — raz_solve_exact (include/raz.h): the full scan of ReversiSolver.solve (exactly = True) for a batch of
// positions of up to RAZ_SOLVE_EXACT_MAX_EMPTIES empties, searched with BOUNDS passed down (alpha-beta) instead of the
// exhaustive scan of raz_solver_batch.hip.  The answer - the game-theoretic disc difference and the lowest-numbered move that
// attains it - is the same pure function of the position; only the number of nodes visited differs.
//
//   the split      raz_solver_split.h's kernels, shared with raz_solver_batch.hip: classify, roots, expand ply by ply (a record of
//                  more than 12 empties and, for at most `plies` plies, one of more than `leaf`).  Here every record knows its
//                  parent and carries a BOUND word: the best value a finished child has proven for it so far;
//   k_se_search    one task per LANE: a record that was not expanded is searched depth first, fail-soft, children ordered by the
//                  opponent's mobility (three tiers; not below SE_ORDER_MIN empties), the last empty square finished in
//                  solver_play.  The ancestors' frames live in the workspace ([level][word][slot]: coalesced), and so does the
//                  node itself between launches: a lane that has visited `budget` nodes in this launch PARKS - its registers go
//                  to its slot - and the same slot resumes in the next launch.  A wave draws tasks for its idle lanes with one
//                  atomicAdd, as k_sb_leaves does (solver_draw);
//   the fold and the output rows, raz_solver_split.h's again.
//
// Sibling bounds.  A task T whose parent P has the bound a (P's view: v(P) >= a, proven by a finished sibling) is searched under a
// window ONE WIDER than alpha-beta's: T's result is exact whenever T's value in P's view is >= a, and otherwise a bound that says
// "< a".  a never exceeds v(P), so every child that attains v(P) - the lowest-numbered one among them too, whenever it was
// searched - holds its exact value and every other child holds something smaller: the fold needs no flag to tell a bound from a
// value, solver_scan finds the first maximum.  P's own result is exact (the maximum is attained by an exact child), so the levels
// above see values only.  A result raises P's bound only where it is a valid lower bound of v(P).  Inside a task the root of a
// ROW keeps the same extra point of window for its later children (moves are not searched in ascending order there), and takes
// an equal value from a lower-numbered move.
// Every launch ends: a lane stops at `budget` visits, and a round advances every parked task by at least one node (its lane
// resumes it before it may draw another).  The host loop runs until the device reports no parked lane and no undrawn record, under
// a cap on rounds derived from the bound on the chunk's node visits.  No floating point, no memo.
#include "raz_solver_split.h"

namespace {

#define SE_MAX_EMPTIES RAZ_SOLVE_EXACT_MAX_EMPTIES
#define SE_MAX_PLIES 6
#define SE_DEFAULT_LEAF 10
#define SE_MAX_TASK 12         // a record of more empties is always split, whatever the tuning: the bound on one lane's task
#define SE_ORDER_MIN 5        // nodes with fewer empties play their moves in ascending order
#define SE_DEFAULT_BUDGET 32768u
#define SE_FRAMES 16          // a node has at least two empties: a task of e <= 17 empties pushes at most e - 2 frames
#define SE_REC_BYTES 32
#define SE_SLOT_W64 (SE_FRAMES * 5 + 5)
#define SE_SLOT_W32 (SE_FRAMES + 3)
#define SE_SLOT_BYTES (SE_SLOT_W64 * 8 + SE_SLOT_W32 * 4)
#define SE_MAX_SLOTS 131072u
#define SE_NONE SPLIT_NONE
#define SE_LO SPLIT_LOWEST    // below every value
#define SE_HI 66              // above every value
#define SE_TUNING_MASK 0x03ffffffu
static_assert(SE_MAX_EMPTIES - 2 <= SE_FRAMES, "frames");
static_assert(SE_MAX_PLIES + 2 <= SPLIT_LEVELS, "levels");
static_assert(RAZ_SOLVER_INLINE_LAST >= 1, "SE_FRAMES rests on solver_play finishing the last empty square itself");

struct SeWs : SplitWs {
    static constexpr int kMaxEmpties = SE_MAX_EMPTIES, kAlways = SE_MAX_TASK;
    static constexpr bool kLinks = true;
    static constexpr const char* kWho = "raz_solve_exact";
    static constexpr auto kBytes = raz_solve_exact_workspace_bytes;
    uint32_t *parent, *bound;   // per record: its parent (SE_NONE: a root); value + 128 of the best finished child (this record's view)
    uint32_t cap;
    unsigned long long* s64;    // slots: word j of slot s = s64[j * nslots + s]
    uint32_t* s32;
    uint32_t nslots;
};

// before a chunk's first round: no slot holds a task
__global__ __launch_bounds__(kBlock) void k_se_clear_slots(SeWs W, uint32_t slots) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < slots; i += stride) W.s32[(size_t)(SE_FRAMES + 1) * W.nslots + i] = SE_NONE;
}

// the node a lane's search stands on
struct SeNode {
    raz_bb own, enemy, left, t0, t1;   // the position from its mover's view; the moves not played yet; the first two tiers of the order
    int best, alpha, beta;             // fail-soft: the best result so far; the window this node was entered with
    int pmove, flip;                   // the move that led here; 1: the parent's value of that move is -f(this node)

    __device__ __forceinline__ uint32_t word() const {
        return (uint32_t)(best + 128) | ((uint32_t)(alpha + 128) << 8) | ((uint32_t)(beta + 128) << 16) | ((uint32_t)pmove << 24) | ((uint32_t)flip << 30);
    }
    __device__ __forceinline__ void set_word(uint32_t w) {
        best = (int)(w & 0xffu) - 128;
        alpha = (int)((w >> 8) & 0xffu) - 128;
        beta = (int)((w >> 16) & 0xffu) - 128;
        pmove = (int)((w >> 24) & 63u);
        flip = (int)((w >> 30) & 1u);
    }
    // the order of the moves: t0 = the moves that leave the opponent the fewest moves, t1 = those within two of that, the rest
    // after them; ascending inside a tier.  (Beyond the 16th move of a node everything is in the last tier.)
    __device__ __forceinline__ void order(bool on) {
        t0 = t1 = 0ULL;
        if (!on || bb_popcount(~(own | enemy)) < SE_ORDER_MIN || !(left & (left - 1))) return;
        unsigned long long keys = 0ULL;
        int least = 15, j = 0;
        for (raz_bb m = left; m && j < 16; m &= m - 1, ++j) {
            const int a = __ffsll((long long)m) - 1;
            const raz_bb fl = bbv_calc_flip(a, own, enemy);
            int k = bb_popcount(bbv_legal_moves(enemy ^ fl, (own ^ fl) | (1ULL << a)));
            k = k > 15 ? 15 : k;
            least = k < least ? k : least;
            keys |= (unsigned long long)k << (4 * j);
        }
        j = 0;
        for (raz_bb m = left; m && j < 16; m &= m - 1, ++j) {
            const int k = (int)((keys >> (4 * j)) & 15ULL);
            const raz_bb bit = m & (~m + 1ULL);
            if (k == least) t0 |= bit;
            if (k <= least + 2) t1 |= bit;
        }
    }
    __device__ __forceinline__ void begin(raz_bb o, raz_bb e, raz_bb moves, int a, int b, int move_here, int sign_flips, bool ordered) {
        own = o; enemy = e; left = moves;
        best = SE_LO; alpha = a; beta = b;
        pmove = move_here; flip = sign_flips;
        order(ordered);
    }
    __device__ __forceinline__ bool finished() const { return left == 0ULL || best >= beta; }
};

struct SeSlot {   // a lane's column of the slot arrays
    unsigned long long* f64;
    uint32_t* f32;
    size_t n;
    __device__ __forceinline__ void put(int d, const SeNode& nd) const {
        f64[(size_t)(d * 5 + 0) * n] = nd.own;
        f64[(size_t)(d * 5 + 1) * n] = nd.enemy;
        f64[(size_t)(d * 5 + 2) * n] = nd.left;
        f64[(size_t)(d * 5 + 3) * n] = nd.t0;
        f64[(size_t)(d * 5 + 4) * n] = nd.t1;
        f32[(size_t)d * n] = nd.word();
    }
    __device__ __forceinline__ void get(int d, SeNode& nd) const {
        nd.own = f64[(size_t)(d * 5 + 0) * n];
        nd.enemy = f64[(size_t)(d * 5 + 1) * n];
        nd.left = f64[(size_t)(d * 5 + 2) * n];
        nd.t0 = f64[(size_t)(d * 5 + 3) * n];
        nd.t1 = f64[(size_t)(d * 5 + 4) * n];
        nd.set_word(f32[(size_t)d * n]);
    }
};

// a maximum on a shared word, with the compare-and-swap the emulator's header has
__device__ __forceinline__ void se_raise(uint32_t* p, uint32_t v) {
    uint32_t old = *(volatile uint32_t*)p;
    while (old < v) {
        const uint32_t seen = atomicCAS(p, old, v);
        if (seen == old) break;
        old = seen;
    }
}

// flags: 1 ordering off, 2 sibling bounds off
__global__ __launch_bounds__(64) void k_se_search(SeWs W, uint32_t budget, uint32_t flags) {
    if (W.hdr->overflow) return;   // (the same for every wave: set, if at all, by the split before this launch)
    const int lane = threadIdx.x;
    const uint32_t slot = blockIdx.x * 64u + (uint32_t)lane;   // (the host launches at most nslots / 64 blocks)
    const SeSlot S{W.s64 + slot, W.s32 + slot, (size_t)W.nslots};
    const bool ordered = !(flags & 1u), siblings = !(flags & 2u);
    const uint32_t total = W.hdr->count < W.cap ? W.hdr->count : W.cap;
    SeNode nd;
    nd.begin(0ULL, 0ULL, 0ULL, SE_LO, SE_HI, 0, 0, false);
    int d = 0, bmv = 64;
    uint32_t task = S.f32[(size_t)(SE_FRAMES + 1) * S.n], task_meta = 0u;
    // (dry from the start once the counter has passed the end: idle waves of later launches add nothing to it, so it cannot wrap)
    bool have = task != SE_NONE, dry = *(volatile uint32_t*)&W.hdr->next >= total;
    if (have) {   // a parked task: the node in the slot's last level, its depth and best root move beside the task's number
        S.get(SE_FRAMES, nd);
        const uint32_t w = S.f32[(size_t)(SE_FRAMES + 2) * S.n];
        d = (int)(w & 0xffu);
        bmv = (int)((w >> 8) & 0xffu);
        task_meta = W.meta[task];
    }
    uint32_t visits = 0u;
    for (uint32_t it = 0u;; ++it) {
        const unsigned long long working = __ballot(have && visits < budget);
        const unsigned long long wanting = __ballot(!have && visits < budget);
        if (!working && (dry || !wanting)) break;
        if (!dry && wanting && (!working || (it & 7u) == 0u)) {
            uint32_t base;
            const uint32_t t = solver_draw(&W.hdr->next, wanting, lane, base);
            if (base >= total) dry = true;
            if (!have && visits < budget && t < total) {
                const uint32_t m = W.meta[t];
                if (rec_kind(m) != 0 && !rec_expanded(m)) {
                    task = t;
                    task_meta = m;
                    const raz_bb own = W.own[t], enemy = W.enemy[t];
                    const uint32_t par = W.parent[t];
                    int a = SE_LO, b = SE_HI;
                    if (siblings && par != SE_NONE) {
                        // the parent's bound pb: exact where this task's value in the parent's view is >= pb
                        const int pb = (int)*(volatile uint32_t*)&W.bound[par] - 128;
                        if (rec_kind(m) == 1) b = 1 - pb;
                        else a = pb - 1;
                    }
                    nd.begin(own, enemy, bbv_legal_moves(own, enemy), a, b, 0, 0, ordered);
                    d = 0;
                    bmv = 64;
                    have = true;
                }
            }
        }
        if (have && visits < budget) {
            bool may_move = false;
            for (int returns = 0; returns <= 2; ++returns) {
                if (!nd.finished()) {
                    may_move = true;
                    break;
                }
                if (returns == 2) break;
                if (d == 0) {
                    const int r = nd.best, kind = rec_kind(task_meta);
                    W.meta[task] = rec_meta(kind == 1 ? -r : r, bmv < 64 ? bmv : -1, kind, 0, 0);
                    const uint32_t par = W.parent[task];
                    if (siblings && par != SE_NONE) {   // (only a valid lower bound of the parent's value raises its bound)
                        if (kind == 1 && r < nd.beta) se_raise(&W.bound[par], (uint32_t)(-r + 128));
                        if (kind != 1 && r > nd.alpha) se_raise(&W.bound[par], (uint32_t)(r + 128));
                    }
                    have = false;
                    task = SE_NONE;
                    break;
                }
                const int v = nd.flip ? -nd.best : nd.best, a = nd.pmove;
                --d;
                S.get(d, nd);
                if (v > nd.best) {
                    nd.best = v;
                    if (d == 0) bmv = a;
                } else if (d == 0 && v == nd.best && a < bmv) bmv = a;
            }
            if (have && may_move) {
                const raz_bb pick = (nd.left & nd.t0) ? (nd.left & nd.t0) : ((nd.left & nd.t1) ? (nd.left & nd.t1) : nd.left);
                const int a = __ffsll((long long)pick) - 1;
                nd.left &= ~(1ULL << a);
                raz_bb no, ne, nm;
                int score;
                const int kind = solver_play(a, nd.own, nd.enemy, no, ne, nm, score, true);
                ++visits;
                if (kind && d < SE_FRAMES) {
                    // the child's window: fail-soft alpha-beta; the task's root keeps one more point below its best value, so
                    // that a lower-numbered move of the same value, searched later, still shows that value
                    const int floor_here = d == 0 ? nd.best - 1 : nd.best, lo = nd.alpha > floor_here ? nd.alpha : floor_here, hi = nd.beta;
                    S.put(d, nd);
                    ++d;
                    nd.begin(no, ne, nm, kind == 1 ? -hi : lo, kind == 1 ? -lo : hi, a, kind == 1 ? 1 : 0, ordered);
                } else {
                    if (score > nd.best) {
                        nd.best = score;
                        if (d == 0) bmv = a;
                    } else if (d == 0 && score == nd.best && a < bmv) bmv = a;
                }
            }
        }
    }
    // park: the slot keeps the node as level SE_FRAMES and, in the two words behind the levels' words, the task's number (SE_NONE:
    // none) and the depth with the best root move
    S.f32[(size_t)(SE_FRAMES + 1) * S.n] = have ? task : SE_NONE;
    if (have) {
        S.put(SE_FRAMES, nd);
        S.f32[(size_t)(SE_FRAMES + 2) * S.n] = (uint32_t)d | ((uint32_t)bmv << 8);
    }
    const unsigned long long parked = __ballot(have);
    unsigned long long v64 = visits;
    for (int s = 1; s < 64; s <<= 1) v64 += __shfl_xor(v64, s);
    if (lane == 0) {
        if (v64) atomicAdd(&W.hdr->visits, v64);
        if (parked) atomicAdd(&W.hdr->open, (uint32_t)__popcll(parked));
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// a bound on the node visits under a position of e empties, whatever the bounds cut: T(e) = e (1 + T(e - 1)), saturating
unsigned long long se_tree(int e) {
    unsigned long long t = 0;
    for (int k = 1; k <= e; ++k) {
        if (t > (1ULL << 56)) return 1ULL << 62;
        t = (unsigned long long)k * (1ULL + t);
    }
    return t;
}
size_t se_good_slots(int e) { return e <= 8 ? 4096 : SE_MAX_SLOTS; }
const uint32_t kBudgets[] = {SE_DEFAULT_BUDGET, 3u, 16u, 128u, 1024u, 8192u};

}  // namespace

extern "C" size_t raz_solve_exact_workspace_bytes(size_t n, int max_empties) {
    if (max_empties > SE_MAX_EMPTIES || n > ((size_t)1 << 31)) return 0;
    if (max_empties < 0) max_empties = 0;
    size_t rec = split_need(max_empties, SE_DEFAULT_LEAF, SE_MAX_PLIES, SE_MAX_TASK);
    if (rec < 256) rec = 256;
    return split_fixed_bytes(n) + (se_good_slots(max_empties) * SE_SLOT_BYTES + 255) / 256 * 256 + rec * SE_REC_BYTES;
}

extern "C" int raz_solve_exact(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int8_t* d_move,
                               int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes, uint32_t tuning,
                               raz_stream_t stream) {
    if (tuning & ~SE_TUNING_MASK) return raz_fail(RAZ_EINVAL, "raz_solve_exact: unknown tuning bits");
    const int leaf = (tuning & 31u) ? (int)(tuning & 31u) : SE_DEFAULT_LEAF;
    const int plies = ((tuning >> 5) & 7u) ? (int)((tuning >> 5) & 7u) - 1 : SE_MAX_PLIES;
    const size_t chunk_rows = (tuning >> 8) & 0xfffu;
    const uint32_t budget_code = (tuning >> 20) & 15u, flags = (tuning >> 24) & 3u;
    if (leaf < 2 || leaf > SE_MAX_EMPTIES) return raz_fail(RAZ_EINVAL, "raz_solve_exact: tuning: leaf size must be 2..17");
    if (plies > SE_MAX_PLIES) return raz_fail(RAZ_EINVAL, "raz_solve_exact: tuning: at most 6 plies are split");
    if (budget_code >= sizeof(kBudgets) / sizeof(kBudgets[0])) return raz_fail(RAZ_EINVAL, "raz_solve_exact: tuning: unknown node budget");
    const uint32_t budget = kBudgets[budget_code];
    if (n == 0) return RAZ_OK;
    if (int rc = split_check_args<SeWs>(d_black, d_white, d_player, n, d_move, d_score, d_status, d_workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t fixed = split_fixed_bytes(n), avail = workspace_bytes - fixed;
    // the slots take at most a fifth of what is left (and never more than SE_MAX_SLOTS), the records the rest
    size_t nslots = avail / 5 / SE_SLOT_BYTES / 64 * 64;
    if (nslots > SE_MAX_SLOTS) nslots = SE_MAX_SLOTS;
    if (nslots < 64) nslots = 64;
    const size_t slot_bytes = (nslots * SE_SLOT_BYTES + 255) / 256 * 256;
    size_t cap = (avail - slot_bytes) / SE_REC_BYTES;
    if (cap > 0xfffffff0u) cap = 0xfffffff0u;
    SeWs W;
    unsigned char* base = (unsigned char*)d_workspace;
    split_layout(W, base, base + fixed + slot_bytes, cap);
    W.parent = W.meta + cap;
    W.bound = W.parent + cap;
    W.s64 = (unsigned long long*)(base + fixed);
    W.s32 = (uint32_t*)(W.s64 + (size_t)SE_SLOT_W64 * nslots);
    W.nslots = (uint32_t)nslots;
    const unsigned long long *bl = (const unsigned long long*)d_black, *wh = (const unsigned long long*)d_white;
    std::vector<uint8_t> emp;
    if (int rc = split_classify(W, bl, wh, d_player, n, workspace_bytes, s, emp)) return rc;

    for (size_t r0 = 0; r0 < n;) {
        // where the first row's split does not fit the records, the chunk splits fewer plies (no split at all is one record: it
        // always fits)
        int p_here = plies;
        const int e0 = emp[r0] <= SE_MAX_EMPTIES ? emp[r0] : 0;
        while (p_here > 0 && split_need(e0, leaf, p_here, SE_MAX_TASK) > cap) --p_here;
        const SplitChunk c = split_chunk<SeWs>(emp, r0, leaf, p_here, cap, chunk_rows);
        unsigned long long nodes = 0;
        for (size_t r = r0; r < c.r1; ++r) {
            const unsigned long long t = se_tree(emp[r] <= SE_MAX_EMPTIES ? emp[r] : 0);
            nodes = nodes + t < (1ULL << 62) ? nodes + t : (1ULL << 62);
        }
        const uint32_t rows = (uint32_t)(c.r1 - r0);
        const size_t used = c.used;
        const unsigned blocks = split_grid(used, 64, (unsigned)(nslots / 64));
        hipLaunchKernelGGL(k_split_roots<SeWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, r0, rows);
        hipLaunchKernelGGL(k_se_clear_slots, dim3(split_grid(blocks * 64u, kBlock, 2048)), dim3(kBlock), 0, s, W, blocks * 64u);
        for (int p = 0; p < c.plies; ++p) {
            hipLaunchKernelGGL(k_split_expand<SeWs>, dim3(split_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, leaf, p_here, 1u);
            hipLaunchKernelGGL(k_split_mark<SeWs>, dim3(1), dim3(64), 0, s, W, p);
        }
        if (int rc = raz_check_launch("raz_solve_exact (split)")) return rc;
        // the rounds: every round visits at least min(budget, what is left) nodes on every lane that holds a task, and lanes
        // without one draw while records are left - so nodes / budget rounds, one more per record, bound the loop
        const unsigned long long max_rounds = nodes / budget + (unsigned long long)used + 2ULL;
        bool done = false;
        unsigned long long seen_visits = ~0ULL;
        uint32_t seen_next = ~0u;
        // the rounds come in GROUPS of 1, 2, 4 ... 16 launches with one read of the header behind each group: `open` counts the
        // lanes that parked in any launch of the group, so a group without one (and no record undrawn) was the last; the launches
        // of a group behind the one that finished the work find nothing to do
        unsigned group = 1;
        for (unsigned long long round = 0; round < max_rounds && !done; round += group, group = group < 16 ? group * 2 : 16) {
            RAZ_HIP_TRY(hipMemsetAsync(&W.hdr->open, 0, sizeof(uint32_t), s), "raz_solve_exact (round)");
            for (unsigned k = 0; k < group; ++k) hipLaunchKernelGGL(k_se_search, dim3(blocks), dim3(64), 0, s, W, budget, flags);
            if (int rc = raz_check_launch("raz_solve_exact (search)")) return rc;
            SplitHdr h;
            RAZ_HIP_TRY(hipMemcpyAsync(&h, W.hdr, sizeof(SplitHdr), hipMemcpyDeviceToHost, s), "raz_solve_exact (read the round's state)");
            RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_solve_exact (synchronise)");
            if (h.overflow) return raz_fail(RAZ_EDEVICE, "raz_solve_exact: the split did not fit the records the host had sized for it");
            done = h.open == 0u && h.next >= (h.count < W.cap ? h.count : W.cap);
            // a launch with work left visits a node on every lane that holds a task, or draws records: a group that did neither is stuck
            if (!done && h.visits == seen_visits && h.next == seen_next)
                return raz_fail(RAZ_EDEVICE, "raz_solve_exact: a group of rounds of the search made no progress");
            seen_visits = h.visits;
            seen_next = h.next;
        }
        if (!done) return raz_fail(RAZ_EDEVICE, "raz_solve_exact: the search did not end within the rounds its node bound allows");
        for (int p = c.plies - 1; p >= 0; --p) hipLaunchKernelGGL(k_split_fold<SeWs>, dim3(split_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, 1u);
        hipLaunchKernelGGL(k_split_out<SeWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, r0, rows, d_move, d_score, d_status);
        if (int rc = raz_check_launch("raz_solve_exact")) return rc;
        r0 = c.r1;
    }
    return RAZ_OK;
}
