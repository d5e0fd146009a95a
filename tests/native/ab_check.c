/* ab_check.c - an independent yardstick for raz_solve_exact beyond the oracle's reach: a plain host negamax with bounds, on loops of
 * its own (no code shared with the library or the oracle).  ab_root runs a FULL window under every root child, so every root
 * child's exact value is recorded; the answer - the first maximum in ascending square order - follows from them.
 * Rules: ReversiEnv's - a side without a move passes, the game ends when neither side can move, the value is the disc difference. */
#include <stdint.h>

static const int DR[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, DC[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
static uint64_t ab_nodes;

static uint64_t flips(int sq, uint64_t own, uint64_t enemy) {
    uint64_t all = 0;
    if ((own | enemy) >> sq & 1) return 0;
    for (int k = 0; k < 8; ++k) {
        uint64_t line = 0;
        int r = sq / 8 + DR[k], c = sq % 8 + DC[k];
        while (r >= 0 && r < 8 && c >= 0 && c < 8 && (enemy >> (r * 8 + c) & 1)) {
            line |= 1ULL << (r * 8 + c);
            r += DR[k];
            c += DC[k];
        }
        if (line && r >= 0 && r < 8 && c >= 0 && c < 8 && (own >> (r * 8 + c) & 1)) all |= line;
    }
    return all;
}
static int mobility(uint64_t own, uint64_t enemy) {
    int n = 0;
    for (uint64_t m = ~(own | enemy); m; m &= m - 1) n += flips(__builtin_ctzll(m), own, enemy) != 0;
    return n;
}
static int discs(uint64_t x) { return __builtin_popcountll(x); }

/* the value of (own to move, enemy) within (alpha, beta), fail-soft; children with the fewest replies first */
static int ab(uint64_t own, uint64_t enemy, int alpha, int beta, int passed) {
    int sq[64], key[64], n = 0, best = -100;
    for (uint64_t m = ~(own | enemy); m; m &= m - 1) {   /* (ascending squares) */
        const int s = __builtin_ctzll(m);
        const uint64_t f = flips(s, own, enemy);
        if (!f) continue;
        sq[n] = s;
        key[n] = discs(~(own | enemy)) > 5 ? mobility(enemy ^ f, (own ^ f) | 1ULL << s) : 0;
        ++n;
    }
    if (!n) return passed ? discs(own) - discs(enemy) : -ab(enemy, own, -beta, -alpha, 1);
    for (int i = 0; i < n; ++i) {
        int at = i;
        for (int j = i + 1; j < n; ++j)
            if (key[j] < key[at]) at = j;
        const int s = sq[at];
        sq[at] = sq[i];
        key[at] = key[i];
        const uint64_t f = flips(s, own, enemy);
        ++ab_nodes;
        const int v = -ab(enemy ^ f, (own ^ f) | 1ULL << s, -beta, -(alpha > best ? alpha : best), 0);
        if (v > best) best = v;
        if (best >= beta) break;
    }
    return best;
}

/* values[s] = the exact value of root move s for the side to move (own), -100 where s is no legal move; returns the number of
 * legal moves (0: the side to move has none) and the answer in *move / *score */
int ab_root(uint64_t own, uint64_t enemy, int8_t* values, int* move, int* score, uint64_t* nodes) {
    int n = 0;
    *move = -1;
    *score = -100;
    ab_nodes = 0;
    for (int s = 0; s < 64; ++s) {
        values[s] = -100;
        const uint64_t f = flips(s, own, enemy);
        if (!f) continue;
        ++n;
        ++ab_nodes;
        values[s] = (int8_t)-ab(enemy ^ f, (own ^ f) | 1ULL << s, -65, 65, 0);
        if (values[s] > *score) {
            *score = values[s];
            *move = s;
        }
    }
    *nodes = ab_nodes;
    return n;
}
