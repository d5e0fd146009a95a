// raz_solver_search.h — the reference's end-game recursion (lib/alt/reversi_solver_cython.pyx:40-127) as ONE LANE runs it, stated
// once for the two solvers whose lanes do: the engine's pool (raz_solver_pool.h) and raz_solve_batch (raz_solver_batch.hip).
// raz_solve_exact (raz_solver_exact.hip) searches with bounds on a node of its own and takes solver_play and solver_scan from here;
// the record tree the two batch calls split their rows into, whose kernels run the same two functions, is raz_solver_split.h's.
// Here are the RULES - what a move leads to, how a node scans its children's values, when a node is finished, how a finished node's
// value reaches its parent, what an ancestor's frame word holds.  The LOOPS around them, and where the frames live, are the
// kernels': the pool's lanes probe a memo, park their searches between launches and cap the returns per iteration; the batch's
// count node visits and draw tasks per wave.  (The wave-uniform search of raz_engine_core.h, solver_solve_scalar, is a third
// statement on the scalar forms of the primitives, inside the tree kernels; it is not built from this header.)
#pragma once
#include "raz_bitboard_valu.h"   // the per-LANE forms of the bitboard primitives (same results for every input)

namespace {

#define RAZ_SOLVER_UNKNOWN (-128)   // a value that is not there yet

// RAZ_SOLVER_INLINE_LAST: a position with ONE empty square left is not handed back as a node - it would cost the worker wave a whole
// iteration to play its only move - but finished in the move function: whoever can play the square plays it (one more calc_flip), the
// discs are counted, and the move reports "the game ends there" with that count.  The same value the two steps give (a node with one
// move has nothing to choose and nothing to cut off); in a full-width search every second node is such a node.
#ifndef RAZ_SOLVER_INLINE_LAST
#define RAZ_SOLVER_INLINE_LAST 1   // 2: positions with TWO empty squares are finished in the move function too (solver_last_two)
// Measured on mini.yml as shipped (M sims/s: two-kernel lock-step / continuous batching / fused lock-step; tools/sessions/r6_s22-24.sh,
// profiles/r6/solver_last_squares_finished_in_the_move_function_ab.json), level x iterations per round:
//   0 x 128: 31.2 / 31.4 / 25.4 (4.61 rounds per answer)     1 x 128: 33.7 / 32.6 / 29.5 (3.28)     1 x 96: 34.2 / 33.7 / 27.5     1 x 64: 33.6 / 32.9 / 23.7
//   2 x 128: 32.0 / 30.6 / 32.1 (2.15: fewer, longer iterations - a round of 128 takes too long)     2 x 96: 33.2 / 31.6 / 30.4     2 x 80: 33.8 / 32.5 / 29.5     2 x 64: 33.8 / 33.3 / 27.7
// Level 1 at 96 iterations per round is the default (the worker runs the two-kernel pipeline with continuous batching when the solver is on).
#endif
// one empty square e, `own` to move: the final disc difference for `own` (env/reversi_env.py:68-85: the mover plays it if that flips
// something, else the opponent does, else the game is over as it stands)
__device__ __forceinline__ int solver_last_one(int e, raz_bb own, raz_bb enemy) {
    const int f = bb_popcount(bbv_calc_flip(e, own, enemy));
    const int po = bb_popcount(own), pe = bb_popcount(enemy);
    if (f) return (po + f + 1) - (pe - f);
    const int g = bb_popcount(bbv_calc_flip(e, enemy, own));
    return g ? (po - g) - (pe + g + 1) : po - pe;
}
// two empty squares, `own` to move with the legal moves `moves` (not empty): the reference's loop over them (ascending, strict
// improvement, non-exact: done at the first value > 0) with each reply finished by solver_last_one
__device__ __forceinline__ int solver_last_two(raz_bb moves, raz_bb own, raz_bb enemy, bool exact) {
    const raz_bb empties = ~(own | enemy);
    int bs = -100;
    for (raz_bb m = moves; m; m &= m - 1) {
        const int s = __ffsll((long long)m) - 1;
        const raz_bb fl = bbv_calc_flip(s, own, enemy);
        const raz_bb o2 = (own ^ fl) | (1ULL << s), e2 = enemy ^ fl;
        const int val = -solver_last_one(__ffsll((long long)(empties & ~(1ULL << s))) - 1, e2, o2);
        if (bs < val) bs = val;
        if (!exact && bs > 0) break;
    }
    return bs;
}
// a position after `mover` (own, enemy) played square a: who moves next.  kind 0: the game ends (v = disc difference for `mover`) -
// there, or on the last RAZ_SOLVER_INLINE_LAST squares, finished here; 1: the opponent moves; 2: the opponent passes (the mover
// again); (no, ne, nm) = the next position from ITS mover's view and its moves
__device__ __forceinline__ int solver_play(int a, raz_bb own, raz_bb enemy, raz_bb& no, raz_bb& ne, raz_bb& nm, int& v, bool exact) {
    const raz_bb flipped = bbv_calc_flip(a, own, enemy);
    const raz_bb nown = (own ^ flipped) | (1ULL << a), nenemy = enemy ^ flipped;
    const raz_bb l1 = bbv_legal_moves(nenemy, nown);
    const raz_bb l2 = l1 ? 0ULL : bbv_legal_moves(nown, nenemy);
    if (!(l1 | l2)) {
        v = bb_popcount(nown) - bb_popcount(nenemy);
        no = ne = nm = 0ULL;
        return 0;
    }
    if (RAZ_SOLVER_INLINE_LAST >= 2 && bb_popcount(~(nown | nenemy)) == 2) {
        // two squares left: the node's mover is the opponent if it can move (l1), else the mover of this move again (l2)
        const bool opp = l1 != 0ULL;
        const int nv = solver_last_two(l1 | l2, opp ? nenemy : nown, opp ? nown : nenemy, exact);
        v = opp ? -nv : nv;
        no = ne = nm = 0ULL;
        return 0;
    }
    if (RAZ_SOLVER_INLINE_LAST && bb_popcount(~(nown | nenemy)) == 1) {
        // the last square: the opponent's if it can play it (l1), else the mover's again (l2)
        const bool opp = l1 != 0ULL;
        const raz_bb last_own = opp ? nenemy : nown, last_enemy = opp ? nown : nenemy;
        const int f = bb_popcount(bbv_calc_flip(__ffsll((long long)(l1 | l2)) - 1, last_own, last_enemy));
        const int last = bb_popcount(last_own) + f + 1, other = bb_popcount(last_enemy) - f;
        v = opp ? other - last : last - other;   // (for the mover of THIS move)
        no = ne = nm = 0ULL;
        return 0;
    }
    no = l1 ? nenemy : nown;
    ne = l1 ? nown : nenemy;
    nm = l1 ? l1 : l2;
    v = 0;
    return l1 ? 1 : 2;
}

// the reference's loop over a node's moves, on values that are already there: val(j) = the value of the node's j-th move (`moves` in
// ascending order, n of them), RAZ_SOLVER_UNKNOWN = not there yet.  Returns false while the scan is not decided.  Strict improvement
// keeps the first maximum; non-exact: it ends at the first value > 0 (the values behind it are not asked for)
template <class Val>
__device__ __forceinline__ bool solver_scan(Val val, int n, raz_bb moves, bool exact, int& bm, int& bs) {
    bm = -1;
    bs = -100;
    raz_bb m = moves;
    for (int j = 0; j < n; ++j, m &= m - 1) {
        const int v = val(j);
        if (v == RAZ_SOLVER_UNKNOWN) return false;
        if (bs < v) {
            bm = __ffsll((long long)m) - 1;
            bs = v;
        }
        if (!exact && bs > 0) break;
    }
    return true;
}

// The node a lane's depth-first search stands on (in registers), the same loop one move at a time.  Its ancestors wait in FRAMES,
// the kernel's own storage: frames.put(d, own, enemy, left, word) / frames.get(d, own, enemy, left, word) keep level d of this lane.
struct SolverNode {
    raz_bb own, enemy, left;   // the position from its mover's view; the moves not played yet
    int bmv, bsc;              // best move and its value so far
    int pact, flip;            // the move that led here (-1: the search's root); 1: the parent's value of that move is -f(this node)

    __device__ __forceinline__ void begin(raz_bb o, raz_bb e, raz_bb moves, int move_here = -1, int sign_flips = 0) {
        own = o; enemy = e; left = moves;
        bmv = -1; bsc = -100;
        pact = move_here; flip = sign_flips;
    }
    __device__ __forceinline__ bool finished(bool exact) const { return left == 0ULL || (!exact && bsc > 0); }
    __device__ __forceinline__ void take(int a, int v) {
        if (bsc < v) {
            bmv = a;
            bsc = v;
        }
    }
    // an ancestor's frame word: best move + 1 | best score + 128 << 8 | the move that led here + 1 << 16 | sign flips << 24
    __device__ __forceinline__ uint32_t word() const {
        return (uint32_t)(bmv + 1) | ((uint32_t)(bsc + 128) << 8) | ((uint32_t)(pact + 1) << 16) | ((uint32_t)flip << 24);
    }
    __device__ __forceinline__ void set_word(uint32_t w) {
        bmv = (int)(w & 0xffu) - 1;
        bsc = (int)((w >> 8) & 0xffu) - 128;
        pact = (int)((w >> 16) & 0xffu) - 1;
        flip = (int)((w >> 24) & 1u);
    }
    // this node (d > 0) has the value rs: back to the parent, which takes it as the value of the move that led here
    template <class Frames>
    __device__ __forceinline__ void give_to_parent(const Frames& frames, int& d, int rs) {
        const int v = flip ? -rs : rs, a = pact;
        uint32_t w;
        --d;
        frames.get(d, own, enemy, left, w);
        set_word(w);
        take(a, v);
    }
    // the next move: down a ply - this node becomes frame d, the search stands on the child (returns true) - or, where the game
    // ends with that move, its score is taken.  `room`: the frames have a level d
    template <class Frames>
    __device__ __forceinline__ bool play_next(const Frames& frames, int& d, bool exact, bool room = true) {
        const int a = __ffsll((long long)left) - 1;
        left &= left - 1;
        raz_bb no, ne, nm;
        int score;
        const int kind = solver_play(a, own, enemy, no, ne, nm, score, exact);
        if (kind && room) {
            frames.put(d, own, enemy, left, word());
            ++d;
            begin(no, ne, nm, a, kind == 1 ? 1 : 0);
            return true;
        }
        take(a, score);
        return false;
    }
};

}  // namespace
