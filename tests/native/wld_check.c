/* wld_check.c - an independent yardstick for raz_solve_wld: a plain host negamax over the three outcomes (+1 win, 0 draw, -1 loss
 * for the side to move), on loops of its own (no code shared with the library, the oracle or ab_check.c).  wld_root searches EVERY
 * root move under the window (-1, +1), so every root move's own outcome is recorded; the answer - the best outcome and the
 * lowest-numbered move that has it - follows from them.
 * Rules: ReversiEnv's - a side without a move passes, the game ends when neither side can move, the outcome is the sign of the disc
 * difference (disc count only). */
#include <stdint.h>

static uint64_t wld_nodes;

/* the eight directions as shifts with the wrap-around columns masked off */
static const int SH[4] = {1, 7, 8, 9};
static const uint64_t MASK[4] = {0x7e7e7e7e7e7e7e7eULL, 0x7e7e7e7e7e7e7e7eULL, 0xffffffffffffffffULL, 0x7e7e7e7e7e7e7e7eULL};

/* the discs that a move on square sq flips (0: not a legal move) */
static uint64_t flips(int sq, uint64_t own, uint64_t enemy) {
    const uint64_t x = 1ULL << sq;
    uint64_t all = 0;
    if ((own | enemy) & x) return 0;
    for (int k = 0; k < 4; ++k) {
        const uint64_t e = enemy & MASK[k];
        uint64_t line = 0, c = (x << SH[k]) & e;
        while (c) {
            line |= c;
            c = (c << SH[k]) & e;
        }
        if (line) {   /* the run of enemy discs from x must end on an own disc */
            uint64_t end = x;
            for (;;) {
                end <<= SH[k];
                if (!(end & line)) break;
            }
            if (end & own) all |= line;
        }
        line = 0;
        c = (x >> SH[k]) & e;
        while (c) {
            line |= c;
            c = (c >> SH[k]) & e;
        }
        if (line) {
            uint64_t end = x;
            for (;;) {
                end >>= SH[k];
                if (!(end & line)) break;
            }
            if (end & own) all |= line;
        }
    }
    return all;
}
static uint64_t legal(uint64_t own, uint64_t enemy) {
    const uint64_t empty = ~(own | enemy);
    uint64_t all = 0;
    for (int k = 0; k < 4; ++k) {
        const uint64_t e = enemy & MASK[k];
        uint64_t t = (own << SH[k]) & e;
        for (int i = 0; i < 5; ++i) t |= (t << SH[k]) & e;
        all |= (t << SH[k]) & empty;
        t = (own >> SH[k]) & e;
        for (int i = 0; i < 5; ++i) t |= (t >> SH[k]) & e;
        all |= (t >> SH[k]) & empty;
    }
    return all;
}
static int discs(uint64_t x) { return __builtin_popcountll(x); }
static int sign(int v) { return (v > 0) - (v < 0); }

/* the outcome of (own to move, enemy) within (alpha, beta), -1 <= alpha < beta <= 1, fail-soft; the moves that leave the opponent
 * the fewest replies first */
static int wld(uint64_t own, uint64_t enemy, int alpha, int beta, int passed) {
    int sq[64], key[64], n = 0, best = -2;
    const int order = discs(~(own | enemy)) > 5;
    for (uint64_t m = legal(own, enemy); m; m &= m - 1) {
        const int s = __builtin_ctzll(m);
        const uint64_t f = flips(s, own, enemy);
        sq[n] = s;
        key[n] = order ? discs(legal(enemy ^ f, own ^ f ^ (1ULL << s))) : 0;
        ++n;
    }
    if (!n) return passed ? sign(discs(own) - discs(enemy)) : -wld(enemy, own, -beta, -alpha, 1);
    for (int i = 0; i < n; ++i) {
        int at = i;
        for (int j = i + 1; j < n; ++j)
            if (key[j] < key[at]) at = j;
        const int s = sq[at];
        sq[at] = sq[i];
        key[at] = key[i];
        const uint64_t f = flips(s, own, enemy);
        ++wld_nodes;
        const int v = -wld(enemy ^ f, own ^ f ^ (1ULL << s), -beta, -(alpha > best ? alpha : best), 0);
        if (v > best) best = v;
        if (best >= beta) break;
    }
    return best;
}

/* outcomes[s] = the outcome of root move s for the side to move (own), -100 where s is no legal move; returns the number of legal
 * moves (0: the side to move has none) and the answer in *move / *outcome */
int wld_root(uint64_t own, uint64_t enemy, int8_t* outcomes, int* move, int* outcome, uint64_t* nodes) {
    int n = 0;
    *move = -1;
    *outcome = -100;
    wld_nodes = 0;
    for (int s = 0; s < 64; ++s) {
        outcomes[s] = -100;
        const uint64_t f = flips(s, own, enemy);
        if (!f) continue;
        ++n;
        ++wld_nodes;
        outcomes[s] = (int8_t)-wld(enemy ^ f, own ^ f ^ (1ULL << s), -1, 1, 0);
        if (outcomes[s] > *outcome) {
            *outcome = outcomes[s];
            *move = s;
        }
    }
    *nodes = wld_nodes;
    return n;
}
