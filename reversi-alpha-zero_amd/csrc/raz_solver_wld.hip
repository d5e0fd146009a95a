// raz_solver_wld.hip — raz_solve_wld (include/raz.h): WHO WINS, for a batch of positions of up to RAZ_SOLVE_WLD_MAX_EMPTIES empties.
// A solved row answers the OUTCOME o in {+1, 0, -1} - the sign of the game-theoretic disc difference from the side to move's view -
// and the lowest-numbered legal move whose own outcome is o: a pure function of the position.
//
//   the split      raz_solver_split.h's kernels, shared with raz_solver_batch.hip and raz_solver_exact.hip: classify, roots, expand
//                  ply by ply (a record of more than WL_MAX_TASK empties always and, for at most `plies` plies, one of more than
//                  `leaf`).  A record knows its parent and carries, beside the split's words,
//                    bound    PROVEN SO FAR: outcome + 128 of the best valid lower bound a finished child has reported (the record's
//                             own view; below 127: nothing yet),
//                    upper    the largest upper bound + 2 a finished child has reported (0: none) - the record's own upper bound once
//                             every child has reported,
//                    pending  its children that have not reported yet,
//                    claimed  1 once the record itself has reported to its parent;
//                  a ROW'S ROOT reports to nobody and keeps in the last two words the lowest child index proven a win and the lowest
//                  proven at least a draw (k_wl_link sets all of them, bottom up, from the children the game ends at);
//   k_wl_search    one task per LANE, as k_se_search: a record that was not expanded is searched depth first, fail-soft, under a window
//                  clamped to -1 <= alpha < beta <= +1, every value clamped to its sign where it is stored; children ordered by the
//                  opponent's mobility; frames and the parked node in the lane's workspace slot;
//   the fold and the output rows, raz_solver_split.h's again (every stored value is one of -1, 0, +1, in the parent's view).
//
// Record cuts.  A lane that draws a record, or resumes a parked one, walks its ancestors (at most WL_MAX_PLIES + 1 of them): an
// ancestor A of proven word b says that only a value above b (A's view) matters below it, which, carried to the task's view with the
// signs of the kinds on the way, raises the task's alpha or lowers its beta.  Where alpha >= beta an ancestor is DECIDED: the task is
// dropped - it stores the least value of its parent's view, which cannot become that parent's maximum unless the maximum is that
// value anyway, and reports the bounds (-1, +1), which say nothing.  A finished task reports (l, u), bounds on its true outcome
// that follow from its fail-soft result and its window; wl_report carries them to the parent's view, raises the parent's two words
// (compare-and-swap loops that end) and takes one from `pending`.  The record whose last child reported, or whose proven word
// reached +1, reports in its turn: ONE reporter per record, claimed by a compare-and-swap of `claimed` from 0 to 1.  No lane waits
// for another.  Every bound ever reported holds for the true outcome AND for the value the fold will compute, so a window is never
// narrower than alpha-beta allows and the fold's values are right wherever they matter (DESIGN.md has the argument).
// The ROOT of a row is special: the answer names the lowest-numbered move of the best outcome, so a root move is dropped only when
// a LOWER-numbered root move is proven a win, and it is searched under (0, +1) only when a win is proven anywhere or a draw at a
// lower number; otherwise under (-1, +1).  Below the root the move does not matter and ties need no extra point of window.
// Every launch ends: a lane stops at `budget` visits, and a round advances every parked task that is not dropped by at least one
// node.  The host loop is raz_solve_exact's: groups of rounds under a cap, an error when a group made no progress.  No floating
// point, no memo.
#include "raz_solver_split.h"

namespace {

#define WL_MAX_EMPTIES RAZ_SOLVE_WLD_MAX_EMPTIES
#define WL_MAX_PLIES 6
#define WL_DEFAULT_LEAF 10
#ifndef WL_MAX_TASK
#define WL_MAX_TASK 15         // a record of more empties is always split, whatever the tuning: the bound on one lane's task
#endif                         // (15 against 16, measured: DESIGN.md)
#define WL_ORDER_MIN 5         // nodes with fewer empties play their moves in ascending order
#define WL_DEFAULT_BUDGET 1024u   // (measured against 8 192 and 32 768: a parked task looks at its ancestors again when it resumes)
#define WL_FRAMES (WL_MAX_TASK - 1)   // a node has at least two empties: a task of e empties pushes at most e - 2 frames
#define WL_REC_BYTES 44
#define WL_SLOT_W64 (WL_FRAMES * 5 + 5)
#define WL_SLOT_W32 (WL_FRAMES + 3)
#define WL_SLOT_BYTES (WL_SLOT_W64 * 8 + WL_SLOT_W32 * 4)
#define WL_MAX_SLOTS 131072u
#define WL_NONE SPLIT_NONE
#define WL_LO (-2)             // below every outcome
#define WL_TUNING_MASK 0x07ffffffu
static_assert(WL_MAX_TASK - 2 <= WL_FRAMES, "frames");
static_assert(WL_MAX_EMPTIES - WL_MAX_TASK <= WL_MAX_PLIES, "the forced split must fit the levels");
static_assert(WL_MAX_PLIES + 2 <= SPLIT_LEVELS, "levels");
static_assert(RAZ_SOLVER_INLINE_LAST >= 1, "WL_FRAMES rests on solver_play finishing the last empty square itself");

struct WlWs : SplitWs {
    static constexpr int kMaxEmpties = WL_MAX_EMPTIES, kAlways = WL_MAX_TASK;
    static constexpr bool kLinks = true;
    static constexpr const char* kWho = "raz_solve_wld";
    static constexpr auto kBytes = raz_solve_wld_workspace_bytes;
    uint32_t *parent, *bound;            // per record: its parent (WL_NONE: a root); proven so far (see above)
    uint32_t cap;
    unsigned long long* s64;             // slots: word j of slot s = s64[j * nslots + s]; the 32-bit words behind the 64-bit ones
    uint32_t nslots;
    // the three words behind `bound` (found from it: fewer kernel arguments for the search kernel to hold in registers); a root:
    // claimed = lowest child index proven a win, upper = lowest proven at least a draw
    __device__ __forceinline__ uint32_t* pending() const { return bound + cap; }
    __device__ __forceinline__ uint32_t* claimed() const { return bound + 2 * (size_t)cap; }
    __device__ __forceinline__ uint32_t* upper() const { return bound + 3 * (size_t)cap; }
    __device__ __forceinline__ uint32_t* s32() const { return (uint32_t*)(s64 + (size_t)WL_SLOT_W64 * nslots); }
};

__device__ __forceinline__ int wl_sign(int v) { return (v > 0) - (v < 0); }
__device__ __forceinline__ uint32_t wl_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a maximum / a minimum on a shared word, with the compare-and-swap the emulator's header has
__device__ __forceinline__ void wl_max(uint32_t* p, uint32_t v) {
    uint32_t old = wl_load(p);
    while (old < v) {
        const uint32_t seen = atomicCAS(p, old, v);
        if (seen == old) break;
        old = seen;
    }
}
__device__ __forceinline__ void wl_min(uint32_t* p, uint32_t v) {
    uint32_t old = wl_load(p);
    while (old > v) {
        const uint32_t seen = atomicCAS(p, old, v);
        if (seen == old) break;
        old = seen;
    }
}
__device__ __forceinline__ int wl_proven(const WlWs& W, uint32_t rec) {   // a record's proven word as an outcome (-1: nothing)
    const int b = (int)wl_load(&W.bound[rec]) - 128;
    return b < -1 ? -1 : b;
}

// before a chunk's first round: no slot holds a task
__global__ __launch_bounds__(kBlock) void k_wl_clear_slots(WlWs W, uint32_t slots) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < slots; i += stride) W.s32()[(size_t)(WL_FRAMES + 1) * W.nslots + i] = WL_NONE;
}

// After the split, level by level from the deepest expanded one up: a child the game ends at holds a disc difference - it becomes its
// sign - and counts as reported, and so does an expanded child that k_wl_link itself found finished a level below; the rest are
// `pending`.  (No atomics: a level's launch reads what the launch before it wrote.)
__global__ __launch_bounds__(kBlock) void k_wl_link(WlWs W, int p) {
    const uint32_t lo = W.hdr->level[p], hi = W.hdr->level[p + 1], stride = gridDim.x * kBlock;
    for (uint32_t i = lo + blockIdx.x * kBlock + threadIdx.x; i < hi; i += stride) {
        const uint32_t m = W.meta[i];
        if (!rec_expanded(m)) continue;
        const int nch = rec_children(m);
        const uint32_t first = W.first[i];
        const bool root = W.parent[i] == WL_NONE;
        uint32_t pend = 0u, win = WL_NONE, draw = WL_NONE;
        int lb = -1, ub = -2;
        for (int j = 0; j < nch; ++j) {
            const uint32_t c = first + (uint32_t)j, cm = W.meta[c];
            int l, u;   // the child's bounds in this record's view
            if (rec_kind(cm) == 0) {
                l = u = wl_sign(rec_value(cm));
                W.meta[c] = rec_meta(l, -1, 0, 0, 0);
            } else if (rec_expanded(cm) && W.claimed()[c] == 1u) {
                const int cb = (int)W.bound[c] - 128, cl = cb >= 1 ? 1 : (cb < -1 ? -1 : cb), cu = cb >= 1 ? 1 : (int)W.upper()[c] - 2;
                l = rec_kind(cm) == 1 ? -cu : cl;
                u = rec_kind(cm) == 1 ? -cl : cu;
            } else {
                ++pend;
                continue;
            }
            lb = l > lb ? l : lb;
            ub = u > ub ? u : ub;
            if (l >= 1 && win == WL_NONE) win = (uint32_t)j;
            if (l >= 0 && draw == WL_NONE) draw = (uint32_t)j;
        }
        W.pending()[i] = pend;
        if (lb > -1) W.bound[i] = (uint32_t)(lb + 128);
        W.claimed()[i] = root ? win : ((pend == 0u || lb >= 1) ? 1u : 0u);
        W.upper()[i] = root ? draw : (uint32_t)(ub + 2);
    }
}

// The window of task t in its own view from its ancestors' proven words; false: an ancestor is decided, the task is dropped
__device__ __forceinline__ bool wl_window(const WlWs& W, uint32_t t, int& alpha, int& beta) {
    alpha = -1;
    beta = 1;
    int sign = 1;   // (an ancestor's view -> the task's view)
    uint32_t cur = t;
#pragma unroll 1
    for (int hop = 0; hop <= WL_MAX_PLIES; ++hop) {
        const uint32_t par = W.parent[cur];
        if (par == WL_NONE) break;
        if (rec_kind(W.meta[cur]) == 1) sign = -sign;
        int b;
        if (W.parent[par] == WL_NONE) {   // a row's root: the lowest-numbered best move must survive
            const uint32_t idx = cur - W.first[par], win = wl_load(&W.claimed()[par]), draw = wl_load(&W.upper()[par]);
            if (win < idx) return false;
            b = (win != WL_NONE || draw < idx) ? 0 : -1;
        } else b = wl_proven(W, par);
        if (sign > 0) alpha = b > alpha ? b : alpha;
        else beta = -b < beta ? -b : beta;
        cur = par;
    }
    return alpha < beta;
}

// Record `rec` is finished with the bounds l <= its outcome <= u (its own view): up the tree while records finish
__device__ __forceinline__ void wl_report(const WlWs& W, uint32_t rec, int l, int u) {
    uint32_t cur = rec;
#pragma unroll 1
    for (int hop = 0; hop <= WL_MAX_PLIES; ++hop) {
        const uint32_t par = W.parent[cur];
        if (par == WL_NONE) return;
        const bool flips = rec_kind(W.meta[cur]) == 1;
        const int pl = flips ? -u : l, pu = flips ? -l : u;   // the parent's view
        if (W.parent[par] == WL_NONE) {
            const uint32_t idx = cur - W.first[par];
            if (pl >= 1) wl_min(&W.claimed()[par], idx);
            if (pl >= 0) wl_min(&W.upper()[par], idx);
            return;
        }
        if (pl > -1) wl_max(&W.bound[par], (uint32_t)(pl + 128));
        wl_max(&W.upper()[par], (uint32_t)(pu + 2));
        __threadfence();
        const uint32_t left = atomicSub(&W.pending()[par], 1u) - 1u;
        __threadfence();
        const int proven = wl_proven(W, par);
        if (left != 0u && proven < 1) return;
        if (atomicCAS(&W.claimed()[par], 0u, 1u) != 0u) return;   // (another lane reports this record)
        l = proven;
        u = proven >= 1 ? 1 : (int)wl_load(&W.upper()[par]) - 2;
        cur = par;
    }
}

// the node a lane's search stands on
struct WlNode {
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
        if (!on || bb_popcount(~(own | enemy)) < WL_ORDER_MIN || !(left & (left - 1))) return;
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
        best = WL_LO; alpha = a; beta = b;
        pmove = move_here; flip = sign_flips;
        order(ordered);
    }
    __device__ __forceinline__ bool finished() const { return left == 0ULL || best >= beta; }
};

struct WlSlot {   // a lane's column of the slot arrays
    unsigned long long* f64;
    uint32_t* f32;
    size_t n;
    __device__ __forceinline__ void put(int d, const WlNode& nd) const {
        f64[(size_t)(d * 5 + 0) * n] = nd.own;
        f64[(size_t)(d * 5 + 1) * n] = nd.enemy;
        f64[(size_t)(d * 5 + 2) * n] = nd.left;
        f64[(size_t)(d * 5 + 3) * n] = nd.t0;
        f64[(size_t)(d * 5 + 4) * n] = nd.t1;
        f32[(size_t)d * n] = nd.word();
    }
    __device__ __forceinline__ void get(int d, WlNode& nd) const {
        nd.own = f64[(size_t)(d * 5 + 0) * n];
        nd.enemy = f64[(size_t)(d * 5 + 1) * n];
        nd.left = f64[(size_t)(d * 5 + 2) * n];
        nd.t0 = f64[(size_t)(d * 5 + 3) * n];
        nd.t1 = f64[(size_t)(d * 5 + 4) * n];
        nd.set_word(f32[(size_t)d * n]);
    }
};

// the value v of move a reaches the node at depth d.  At a ROW'S ROOT the lowest-numbered move of the best outcome is kept, and
// once a win is known only lower-numbered moves are still of interest
__device__ __forceinline__ void wl_take(WlNode& nd, int d, bool row_root, int& bmv, int v, int a) {
    if (v > nd.best) {
        nd.best = v;
        if (d == 0) bmv = a;
    } else if (d == 0 && v == nd.best && a < bmv) bmv = a;
    if (d == 0 && row_root && nd.best >= 1) nd.left &= (1ULL << bmv) - 1ULL;
}

// flags: 1 ordering off, 2 the ancestors' proven words do not narrow a task's window, 4 record cuts off (no walk, no report)
__global__ __launch_bounds__(64) void k_wl_search(WlWs W, uint32_t budget, uint32_t flags) {
    if (W.hdr->overflow) return;   // (the same for every wave: set, if at all, by the split before this launch)
    const int lane = threadIdx.x;
    const uint32_t slot = blockIdx.x * 64u + (uint32_t)lane;   // (the host launches at most nslots / 64 blocks)
    const WlSlot S{W.s64 + slot, W.s32() + slot, (size_t)W.nslots};
    const bool ordered = !(flags & 1u), narrow = !(flags & 2u), cuts = !(flags & 4u);
    const uint32_t total = W.hdr->count < W.cap ? W.hdr->count : W.cap;
    WlNode nd;
    nd.begin(0ULL, 0ULL, 0ULL, -1, 1, 0, 0, false);
    int d = 0, bmv = 64;
    uint32_t task = S.f32[(size_t)(WL_FRAMES + 1) * S.n], task_meta = 0u;
    // look: the task's ancestors are to be looked at before its next node - it was drawn (fresh: its root node is to be set up too)
    // or it was parked
    bool have = task != WL_NONE, row_root = false, dry = wl_load(&W.hdr->next) >= total;
    int look = 0;   // 1: a parked task, 2: a fresh one
    uint32_t visits = 0u;
    if (have) {   // a parked task: the node in the slot's last level, its depth and best root move beside the task's number
        task_meta = W.meta[task];
        row_root = W.parent[task] == WL_NONE;
        S.get(WL_FRAMES, nd);
        const uint32_t w = S.f32[(size_t)(WL_FRAMES + 2) * S.n];
        d = (int)(w & 0xffu);
        bmv = (int)((w >> 8) & 0xffu);
        look = cuts ? 1 : 0;
    }
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
                    row_root = W.parent[t] == WL_NONE;
                    have = true;
                    look = 2;
                }
            }
        }
        bool report = false;
        int rep_l = -1, rep_u = 1;   // (a dropped task's bounds say nothing)
        if (have && look != 0) {
            int a = -1, b = 1;
            if (cuts && !wl_window(W, task, a, b)) {   // an ancestor is decided: dropped, with the least value of the parent's view
                W.meta[task] = rec_meta(-1, -1, rec_kind(task_meta), 0, 0);
                report = true;
                have = false;
            } else if (look == 2) {
                if (!narrow) {
                    a = -1;
                    b = 1;
                }
                const raz_bb own = W.own[task], enemy = W.enemy[task];
                // (a row's root is never cut off: its beta stands above every outcome)
                nd.begin(own, enemy, bbv_legal_moves(own, enemy), a, row_root ? 2 : b, 0, 0, ordered);
                d = 0;
                bmv = 64;
            }
            look = 0;
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
                    // the bounds the fail-soft result gives under the task's window
                    rep_l = r >= nd.beta || r > nd.alpha ? r : -1;
                    rep_u = r <= nd.alpha || r < nd.beta ? r : 1;
                    report = cuts;
                    have = false;
                    break;
                }
                const int v = nd.flip ? -nd.best : nd.best, a = nd.pmove;
                --d;
                S.get(d, nd);
                wl_take(nd, d, row_root, bmv, v, a);
            }
            if (have && may_move) {
                const raz_bb pick = (nd.left & nd.t0) ? (nd.left & nd.t0) : ((nd.left & nd.t1) ? (nd.left & nd.t1) : nd.left);
                const int a = __ffsll((long long)pick) - 1;
                nd.left &= ~(1ULL << a);
                raz_bb no, ne, nm;
                int score;
                const int kind = solver_play(a, nd.own, nd.enemy, no, ne, nm, score, true);
                ++visits;
                if (kind && d < WL_FRAMES) {
                    // the child's window: fail-soft alpha-beta.  A row's root asks every move for its full outcome until a win is
                    // known, or a draw at a lower number: then only whether the move wins
                    int lo = nd.alpha > nd.best ? nd.alpha : nd.best;
                    if (d == 0 && row_root) lo = (nd.best >= 1 || (nd.best == 0 && a > bmv)) ? 0 : -1;
                    const int hi = nd.beta > 1 ? 1 : nd.beta;
                    S.put(d, nd);
                    ++d;
                    nd.begin(no, ne, nm, kind == 1 ? -hi : lo, kind == 1 ? -lo : hi, a, kind == 1 ? 1 : 0, ordered);
                } else wl_take(nd, d, row_root, bmv, wl_sign(score), a);
            }
        }
        if (report) wl_report(W, task, rep_l, rep_u);
    }
    // park: the slot keeps the node as level WL_FRAMES and, in the two words behind the levels' words, the task's number (WL_NONE:
    // none) and the depth with the best root move
    S.f32[(size_t)(WL_FRAMES + 1) * S.n] = have ? task : WL_NONE;
    if (have) {
        S.put(WL_FRAMES, nd);
        S.f32[(size_t)(WL_FRAMES + 2) * S.n] = (uint32_t)d | ((uint32_t)bmv << 8);
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
unsigned long long wl_tree(int e) {
    unsigned long long t = 0;
    for (int k = 1; k <= e; ++k) {
        if (t > (1ULL << 56)) return 1ULL << 62;
        t = (unsigned long long)k * (1ULL + t);
    }
    return t;
}
size_t wl_good_slots(int e) { return e <= 8 ? 4096 : WL_MAX_SLOTS; }
const uint32_t kWlBudgets[] = {WL_DEFAULT_BUDGET, 3u, 16u, 128u, 1024u, 8192u, 32768u};

}  // namespace

// The records the workspace must hold for a row of e empties: split_need(e, 10, 6, 15), the worst case of the default split - at 21
// empties six plies down to 15, 1 + 21 + 21 * 20 + ... + 21 * 20 * 19 * 18 * 17 * 16 = 41 664 022 records of 44 bytes
extern "C" size_t raz_solve_wld_workspace_bytes(size_t n, int max_empties) {
    if (max_empties > WL_MAX_EMPTIES || n > ((size_t)1 << 31)) return 0;
    if (max_empties < 0) max_empties = 0;
    size_t rec = split_need(max_empties, WL_DEFAULT_LEAF, WL_MAX_PLIES, WL_MAX_TASK);
    if (rec < 256) rec = 256;
    return split_fixed_bytes(n) + (wl_good_slots(max_empties) * WL_SLOT_BYTES + 255) / 256 * 256 + rec * WL_REC_BYTES;
}

extern "C" int raz_solve_wld(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int8_t* d_move,
                             int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes, uint32_t tuning,
                             raz_stream_t stream) {
    if (tuning & ~WL_TUNING_MASK) return raz_fail(RAZ_EINVAL, "raz_solve_wld: unknown tuning bits");
    const int leaf = (tuning & 31u) ? (int)(tuning & 31u) : WL_DEFAULT_LEAF;
    const int plies = ((tuning >> 5) & 7u) ? (int)((tuning >> 5) & 7u) - 1 : WL_MAX_PLIES;
    const size_t chunk_rows = (tuning >> 8) & 0xfffu;
    const uint32_t budget_code = (tuning >> 20) & 15u, flags = (tuning >> 24) & 7u;
    if (leaf < 2 || leaf > WL_MAX_EMPTIES) return raz_fail(RAZ_EINVAL, "raz_solve_wld: tuning: leaf size must be 2..the most empties");
    if (plies > WL_MAX_PLIES) return raz_fail(RAZ_EINVAL, "raz_solve_wld: tuning: at most 6 plies are split");
    if (budget_code >= sizeof(kWlBudgets) / sizeof(kWlBudgets[0])) return raz_fail(RAZ_EINVAL, "raz_solve_wld: tuning: unknown node budget");
    const uint32_t budget = kWlBudgets[budget_code];
    if (n == 0) return RAZ_OK;
    if (int rc = split_check_args<WlWs>(d_black, d_white, d_player, n, d_move, d_score, d_status, d_workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t fixed = split_fixed_bytes(n), avail = workspace_bytes - fixed;
    // the slots take at most a fifth of what is left (and never more than WL_MAX_SLOTS), the records the rest
    size_t nslots = avail / 5 / WL_SLOT_BYTES / 64 * 64;
    if (nslots > WL_MAX_SLOTS) nslots = WL_MAX_SLOTS;
    if (nslots < 64) nslots = 64;
    const size_t slot_bytes = (nslots * WL_SLOT_BYTES + 255) / 256 * 256;
    size_t cap = (avail - slot_bytes) / WL_REC_BYTES;
    if (cap > 0xfffffff0u) cap = 0xfffffff0u;
    WlWs W;
    unsigned char* base = (unsigned char*)d_workspace;
    split_layout(W, base, base + fixed + slot_bytes, cap);
    W.parent = W.meta + cap;
    W.bound = W.parent + cap;
    W.s64 = (unsigned long long*)(base + fixed);
    W.nslots = (uint32_t)nslots;
    const unsigned long long *bl = (const unsigned long long*)d_black, *wh = (const unsigned long long*)d_white;
    std::vector<uint8_t> emp;
    if (int rc = split_classify(W, bl, wh, d_player, n, workspace_bytes, s, emp)) return rc;

    for (size_t r0 = 0; r0 < n;) {
        // where the first row's split does not fit the records, the chunk splits fewer plies (down to what the task bound forces:
        // that much always fits a workspace of the size asked for)
        int p_here = plies;
        const int e0 = emp[r0] <= WL_MAX_EMPTIES ? emp[r0] : 0;
        while (p_here > 0 && split_need(e0, leaf, p_here, WL_MAX_TASK) > cap) --p_here;
        const SplitChunk c = split_chunk<WlWs>(emp, r0, leaf, p_here, cap, chunk_rows);
        unsigned long long nodes = 0;
        for (size_t r = r0; r < c.r1; ++r) {
            const unsigned long long t = wl_tree(emp[r] <= WL_MAX_EMPTIES ? emp[r] : 0);
            nodes = nodes + t < (1ULL << 62) ? nodes + t : (1ULL << 62);
        }
        const uint32_t rows = (uint32_t)(c.r1 - r0);
        const size_t used = c.used;
        const unsigned blocks = split_grid(used, 64, (unsigned)(nslots / 64));
        hipLaunchKernelGGL(k_split_roots<WlWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, bl, wh, d_player, r0, rows);
        hipLaunchKernelGGL(k_wl_clear_slots, dim3(split_grid(blocks * 64u, kBlock, 2048)), dim3(kBlock), 0, s, W, blocks * 64u);
        for (int p = 0; p < c.plies; ++p) {
            hipLaunchKernelGGL(k_split_expand<WlWs>, dim3(split_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, leaf, p_here, 1u);
            hipLaunchKernelGGL(k_split_mark<WlWs>, dim3(1), dim3(64), 0, s, W, p);
        }
        for (int p = c.plies - 1; p >= 0; --p) hipLaunchKernelGGL(k_wl_link, dim3(split_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p);
        if (int rc = raz_check_launch("raz_solve_wld (split)")) return rc;
        // the rounds, as raz_solve_exact runs them: nodes / budget rounds, one more per record, bound the loop; groups of 1, 2, 4 ...
        // 16 launches with one read of the header behind each
        const unsigned long long max_rounds = nodes / budget + (unsigned long long)used + 2ULL;
        bool done = false;
        unsigned long long seen_visits = ~0ULL;
        uint32_t seen_next = ~0u;
        unsigned group = 1;
        for (unsigned long long round = 0; round < max_rounds && !done; round += group, group = group < 16 ? group * 2 : 16) {
            RAZ_HIP_TRY(hipMemsetAsync(&W.hdr->open, 0, sizeof(uint32_t), s), "raz_solve_wld (round)");
            for (unsigned k = 0; k < group; ++k) hipLaunchKernelGGL(k_wl_search, dim3(blocks), dim3(64), 0, s, W, budget, flags);
            if (int rc = raz_check_launch("raz_solve_wld (search)")) return rc;
            SplitHdr h;
            RAZ_HIP_TRY(hipMemcpyAsync(&h, W.hdr, sizeof(SplitHdr), hipMemcpyDeviceToHost, s), "raz_solve_wld (read the round's state)");
            RAZ_HIP_TRY(hipStreamSynchronize(s), "raz_solve_wld (synchronise)");
            if (h.overflow) return raz_fail(RAZ_EDEVICE, "raz_solve_wld: the split did not fit the records the host had sized for it");
            done = h.open == 0u && h.next >= (h.count < W.cap ? h.count : W.cap);
            // a launch with work left visits a node on every lane that keeps its task, or draws records: a group that did neither is stuck
            if (!done && h.visits == seen_visits && h.next == seen_next)
                return raz_fail(RAZ_EDEVICE, "raz_solve_wld: a group of rounds of the search made no progress");
            seen_visits = h.visits;
            seen_next = h.next;
        }
        if (!done) return raz_fail(RAZ_EDEVICE, "raz_solve_wld: the search did not end within the rounds its node bound allows");
        for (int p = c.plies - 1; p >= 0; --p) hipLaunchKernelGGL(k_split_fold<WlWs>, dim3(split_grid(used, kBlock, 2048)), dim3(kBlock), 0, s, W, p, 1u);
        hipLaunchKernelGGL(k_split_out<WlWs>, dim3(split_grid(rows, kBlock, 2048)), dim3(kBlock), 0, s, W, r0, rows, d_move, d_score, d_status);
        if (int rc = raz_check_launch("raz_solve_wld")) return rc;
        r0 = c.r1;
    }
    return RAZ_OK;
}
