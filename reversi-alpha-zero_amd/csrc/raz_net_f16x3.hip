// raz_net_f16x3.hip — forward pass of WIDE policy/value nets (F % 128 == 0, e.g. the 256x10 net of config.py:187-193)
// with the 3x3 convolutions of the trunk on the f16 matrix cores at f32-class accuracy: "raznet-forward-v2".
//
// f32 MFMA runs at the f32 vector rate (157 TF); f16 MFMA at 16x that.  Every f32 operand x is carried as a pair of halfs
// (hi, lo) = (f16(x), f16(x - hi)) - 22 significant bits; subnormal halfs are kept by the matrix core (probed:
// tools/probe_f16.hip) - and a product x*w is evaluated as  hi_x*hi_w + hi_x*lo_w + lo_x*hi_w  (the dropped lo*lo term is
// 2^-22 relative), three v_mfma_f32_32x32x16_f16 accumulating in f32 into ONE accumulator.  Weights are pre-scaled per
// layer by a power of two S (max |w| * S in [2^14, 2^15): the lo halves of all but negligible weights stay normal numbers;
// the accumulator is multiplied by the exact 1/S before the bias).  Net effect: 3/16 of the f32-MFMA time per MAC, results
// within 1e-5 of the fp32 graph (tests: vs fp32 torch and vs the exact-f32 kernel raznet-forward-v1 on the benchmarked
// shape), NOT bit-identical to the CPU oracle's fmaf chains - the matrix core's internal 16-term summation is not a
// documented IEEE sequence - so games played on this path are checked against the oracle fed with THIS net's outputs
// through the reference's own NN seam (ReversiPlayer(api=...), agent/player.py:41).  The first layer (2 planes) and the
// heads (raz_net_heads.h) stay exact-f32 VALU chains as in v1.
//
// Activations live in HBM already split, in the order the kernel's LDS image wants them:
//     [position][16-channel chunk][plane: k-group(8 ch) x {hi, lo} = 4][square 64][8 halfs]      (F*256 bytes per position)
// so that one (position, chunk) is four lane-linear 1 KiB pieces moved by global_load_lds (no registers, no ds_write).
//
// GEMM view per layer: D[oc, sq] += W[oc, k] * X[k, sq], k = (chunk, tap, channel in chunk).
//   workgroup = 8 waves = 128 output channels x 8 positions (one workgroup per CU, 2 waves per SIMD, <= 256 VGPRs);
//               wave = 64 oc x 4 board rows of FOUR positions = 2 x 4 MFMA tiles (128 accumulator registers): wave w takes the oc
//               half w & 1, the position group (w >> 1) & 1 (positions 0-3 or 4-7) and the row half w >> 2 (board rows 0-3 or 4-7);
//               N tile j is board row 4 half + j, its column c is position c >> 3, file c & 7
//   K loop    = 16 chunks x 3 tap groups (dy = -1, 0, +1) = 48 stages; a stage's weights (24 KB: 3 taps x 16 channels x 128 oc x
//               {hi, lo}) arrive by LDS-DMA TWO stages ahead in three buffers, and once per chunk the 8 positions' activations
//               (32 KB) in two images, while the stages before them run 3 taps x 8 tiles x 3 MFMAs per wave: one barrier per stage,
//               no register staging.  A stage has therefore been in LDS since the barrier BEFORE its own, and a wave reads each
//               tap's operands while the tap before it computes - a stage's first tap during the last tap of the stage before,
//               across the barrier (TapOps, tap_pipelined): after a barrier the matrix instructions start from registers
//   hazards   = who writes each LDS area, who reads it last, and the barrier between (barrier s opens stage s = 3 c + tg; a wave drains
//               its own DMA - the vmcnt(0) of __syncthreads - before it arrives at any barrier, so what was issued before barrier s - 1
//               by anyone is in LDS when barrier s opens):
//                 weight buffer tg   written: stage (c, tg)'s weights, issued after barrier s - 2 (stages 0 and 1: before barrier 0),
//                                    so landed when barrier s - 1 opens.  Read: first tap during stage s - 1's last tap, after barrier
//                                    s - 1; the rest in stage s.  Last read before barrier s + 1; next written (stage s + 3) after it.
//                 image c & 1        written: chunk c's activations, issued after barrier 3 c - 2 (chunk 0: before barrier 0), landed
//                                    when barrier 3 c - 1 opens.  Read: from the last tap of stage (c - 1, 2), after barrier 3 c - 1,
//                                    to the end of stage (c, 2).  Last read before barrier 3 c + 3; next written (chunk c + 2) after
//                                    barrier 3 c + 4.
//                 zero areas         written once by threads 0..255 before barrier 0; only read afterwards.
//                 after the last stage  the read-ahead reads buffer 0 and the other image once more: nothing is in flight into them
//                                    and the values are not used.
//                 skip rows (HBM)    a lane reads the 16 bytes it later overwrites itself, and no other lane or workgroup writes them.
//   row skip  = with a tile being ONE board row, the taps dy = -1 of row 0 and dy = +1 of row 7 are whole all-zero B operands: a
//               top-half wave issues neither reads nor matrix instructions for its tile 0 in the stages dy = -1, a bottom-half wave
//               none for its tile 3 in the stages dy = +1 (6 of 72 tile-taps: 198 instead of 216 matrix instructions per wave and
//               chunk, v3 66 instead of 72).  A skipped instruction added exact zeros to an accumulator that started at +0, and the
//               others keep their order per accumulator, so no bit moves.  Waves w and w + 4 share a SIMD (HW_ID in the stamps:
//               profiles/r11), one of each row half, so every SIMD saves the same 6 tile-taps in 2 stages of 3
//   taps      = three per-lane LDS addresses (dx = -1, 0, +1) at board row 4 half - 1; tile j under dy adds (j + dy + 1) * 128 as an
//               immediate.  A file off the board reads a zero area instead, at the bank class of the slot it would have read (the
//               area spans every immediate), so there are no predicates and no halo in the image; no row off the board is ever read
//   LDS reads = ds_read_b128, conflict-free by construction: A - lanes 0-31 read consecutive 16-byte slots (channels), lanes 32-63
//               the other k-group's plane; B - 8 files x 4 positions, the positions 4,096 + 128 bytes apart (act_pos_off);
//               0.5 reads per MFMA
//   epilogue  = the wave's halves trade accumulators (tiles 2 k and 2 k + 1) so that a lane owns the 8 channels of one (position,
//               row, file); * 1/S, + bias, (+ skip), relu, split into (hi, lo), 16-byte stores in 128-byte runs (a row's 8 files).
//               Whether a lane stores and raises its position's range flag is the lane's own position's liveness; a wave leaves
//               early only when none of its four positions is live
//
// "raznet-forward-v3" (SPLIT = false below; opt-in, raz_net.reserved = 8) is v2 with every lo half taken as zero: activations and
// weights are the hi halfs alone, out = f16(relu(acc / S + bias [+ skip])) with ONE matrix instruction per product.  Same tiling,
// LDS image, HBM layouts, weight image and scales; the lo planes in HBM and the lo halves of the LDS image are holes that v3 never
// reads or writes (12 of a stage's 24 weight pieces and 2 of a chunk's 4 activation planes are moved).  Its error is f16's own
// (about 11 bits per activation): NOT within 1e-5 of the fp32 graph - include/raz.h raz_net_range_check.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "raz_bitboard.h"
#include "raz_detmath.h"
#include "raz_internal.h"
#include "raz_net_heads.h"
#include "raz_net_layout.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int OCT = 128;                         // output channels per workgroup
constexpr int NWAVE = 8;                         // waves per workgroup = positions per workgroup
constexpr int W_STAGE = 3 * 2 * 2 * OCT * 16;    // 24,576 B: [tap 3][k-group 2][hi/lo][oc 128][16 B]
constexpr int ACT_POS = 4 * 64 * 16;             // 4,096 B: [plane 4][square 64][16 B]
constexpr int Z_OFF = NWAVE * (ACT_POS + 128);   // the zero area inside an image, after the 8 positions (act_pos_off): 33,792
constexpr int Z_BYTES = 2048;                    // a bank-class slot (< 256) + a row offset (<= 5 * 128) + the lo plane's 1,024 + 16 B
constexpr int ACT_IMG = Z_OFF + Z_BYTES;         // one chunk's image: 8 positions + the zero area (35,840 B)
constexpr int LDS_W = 0;                         // three weight stages (stage st lives in buffer st % 3 = its tap group)
constexpr int LDS_ACT = 3 * W_STAGE;             // two activation images (chunk c lives in image c & 1)
constexpr int LDS_BYTES = LDS_ACT + 2 * ACT_IMG; // 145,408 B: one workgroup of 8 waves per CU
// Where position p (0..7) of the workgroup starts inside an image.  A B read takes 8 files x 4 positions; the LDS serves a 16-byte
// read in the lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (and the same + 32), i.e. files 0-3 of positions 0 and 3 with
// files 4-7 of positions 1 and 2, and the reverse.  With every position on the same 256-byte bank row those would meet two by two;
// with the positions 4,096 + 128 bytes apart (the odd ones half a bank row up), each group covers the 16 slots of a bank row once.
constexpr int act_pos_off(int p) { return p * (ACT_POS + 128); }

// Timeline instrumentation of the conv kernel, compiled in ONLY by tools/probe_conv.hip (which includes this file with
// RAZ_F16X3_STAMPS defined): per wave 8 words - s_memtime at entry [0], when stage 0 has landed [1], at the end of the K loop [2],
// after the last store was issued [3] and after the stores have drained [4]; the cycles spent inside the 48 stage barriers [5];
// HW_ID [6] (which CU / SIMD ran the wave); s_memrealtime at entry [7].  The product build has none of it.
#ifdef RAZ_F16X3_STAMPS
#define RAZ_STAMP_PARAM , unsigned long long* __restrict__ stamps
#define RAZ_STAMP_ARG , (unsigned long long*)nullptr
#define RAZ_STAMP_BEGIN                                                                                           \
    unsigned long long st_t[8];                                                                                   \
    st_t[0] = __builtin_amdgcn_s_memtime();                                                                       \
    st_t[7] = __builtin_amdgcn_s_memrealtime();                                                                   \
    st_t[6] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32); \
    st_t[5] = 0;                                                                                                  \
    st_t[1] = st_t[2] = st_t[3] = st_t[4] = 0;                                                                    \
    unsigned long long st_b = 0
#define RAZ_STAMP_BARRIER_IN st_b = __builtin_amdgcn_s_memtime()
#define RAZ_STAMP_BARRIER_OUT(st_)                                    \
    do {                                                              \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();   \
        st_t[5] += t_ - st_b;                                         \
        if ((st_) == 0) st_t[1] = t_;                                 \
    } while (0)
#define RAZ_STAMP_AT(i_) st_t[i_] = __builtin_amdgcn_s_memtime()
#define RAZ_STAMP_END                                                                                    \
    do {                                                                                                 \
        st_t[3] = __builtin_amdgcn_s_memtime();                                                          \
        __builtin_amdgcn_s_waitcnt(0x0070); /* vmcnt(0) */                                               \
        st_t[4] = __builtin_amdgcn_s_memtime();                                                          \
        if (lane == 0 && stamps)                                                                         \
            for (int i_ = 0; i_ < 8; ++i_) stamps[((size_t)blockIdx.x * NWAVE + wv) * 8 + i_] = st_t[i_]; \
    } while (0)
#else
#define RAZ_STAMP_PARAM
#define RAZ_STAMP_ARG
#define RAZ_STAMP_BEGIN
#define RAZ_STAMP_BARRIER_IN
#define RAZ_STAMP_BARRIER_OUT(st_)
#define RAZ_STAMP_AT(i_)
#define RAZ_STAMP_END
#endif

// The two halves of a wave trade one value each: lane l < 32 gives `b` to lane l + 32 and takes that lane's `a`.  Afterwards
// `first` holds (a of lane l, b of lane l - 32) and `second` (a of lane l + 32, b of lane l) in lanes (< 32, >= 32).  On the device
// this is ONE v_permlane32_swap_b32; the wave emulator has no such builtin and says the same with a shuffle.  The shuffle form on
// the device (ds_bpermute and three selects per value, 128 values per lane in the conv epilogue) was measured against it: the
// epilogue takes 12.8 k instead of 11.5 k cycles (profiles/r8/conv_f16x3_epilogue_trade_shuffle_vs_swap.json).  Pure data movement
// either way; tests/test_net_f16x3_bits_gpu.py holds the device form to the bits recorded before it existed.
__device__ __forceinline__ void halves_trade(float a, float b, int upper, float& first, float& second) {
#ifdef RAZ_WAVE_EMU
    const float got = __shfl_xor(upper ? a : b, 32);
    first = upper ? got : a;
    second = upper ? b : got;
#else
    (void)upper;
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    first = __uint_as_float(r[0]);
    second = __uint_as_float(r[1]);
#endif
}

#define GLDS16(gptr, lptr)                                                                                      \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),                     \
                                     (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

// The operands of ONE tap for the rows of a stage's main pass (up to 48 VGPRs; v3 half of that).  The main pass keeps two sets: the
// matrix instructions of a tap run from one while the other is being read from LDS for the tap after it - for a stage's last tap
// that is the FIRST tap (dx = -1) of the next stage, read before that stage's barrier.
struct TapOps {
    h8 bh[4], bl[4], ah[2], al[2];
};

// Read number k of a tap's operands, in the order the tap's matrix instructions first use them: al0, bh[J0], ah0, bl[J0], then
// (bh, bl) of the rows after J0, then al1, ah1 (!SPLIT: ah0, the bh, ah1).  wtap = the tap's place in its weight buffer + the lane's
// offset; btap = the lane's B address of that tap inside the image (abase + boff[tap]).
template <bool SPLIT, int TG, int J0, int J1>
__device__ __forceinline__ void tap_read(const unsigned char* lds, uint32_t wtap, uint32_t btap, int k, TapOps& p) {
    constexpr int R = J1 - J0;
    if constexpr (SPLIT) {
        if (k == 0) p.al[0] = *(const h8*)(lds + wtap + 2048);
        else if (k == 2) p.ah[0] = *(const h8*)(lds + wtap);
        else if (k == 2 * R + 2) p.al[1] = *(const h8*)(lds + wtap + 512 + 2048);
        else if (k == 2 * R + 3) p.ah[1] = *(const h8*)(lds + wtap + 512);
        else {
            const int b = k == 1 ? 0 : k == 3 ? 1 : k - 2;   // B read number: (row, hi / lo)
            const int j = J0 + (b >> 1);
            if (b & 1) p.bl[j] = *(const h8*)(lds + btap + (j + TG) * 128 + 1024);
            else p.bh[j] = *(const h8*)(lds + btap + (j + TG) * 128);
        }
    } else {
        if (k == 0) p.ah[0] = *(const h8*)(lds + wtap);
        else if (k == R + 1) p.ah[1] = *(const h8*)(lds + wtap + 512);
        else p.bh[J0 + k - 1] = *(const h8*)(lds + btap + (J0 + k - 1 + TG) * 128);
    }
}
template <bool SPLIT, int R>
constexpr int tap_reads() { return SPLIT ? 2 * R + 4 : R + 2; }

// Matrix instruction number q of a tap: 32-tile m, row j, and for SPLIT the term (al*bh, ah*bl, ah*bh in that order).
template <bool SPLIT, int J0, int J1>
__device__ __forceinline__ void tap_mfma(const TapOps& p, int q, f32x16 (&acc)[2][4]) {
    constexpr int R = J1 - J0;
    if constexpr (SPLIT) {
        const int m = q / (3 * R), j = J0 + (q / 3) % R, term = q % 3;
        acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 0 ? p.al[m] : p.ah[m], term == 1 ? p.bl[j] : p.bh[j], acc[m][j], 0, 0, 0);
    } else {
        const int m = q / R, j = J0 + q % R;
        acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p.ah[m], p.bh[j], acc[m][j], 0, 0, 0);
    }
}
template <bool SPLIT, int R>
constexpr int tap_mfmas() { return SPLIT ? 6 * R : 2 * R; }

// One tap of a main pass: its matrix instructions from `cur`, with the reads of the tap after it (tap group NTG, rows NJ0 .. NJ1 - 1)
// into `nxt` spread evenly over the first three quarters of them: the wait that opens the next tap is a full one (the compiler counts
// no LDS reads beside LDS-DMA), and the last quarter gives the last read time to land.  The order is pinned: left to itself the
// scheduler gathers a tap's reads into one burst right before that wait - measured, the K loop is then 14 % longer
// (profiles/r16/conv_f16x3_schedule_variants.json).
template <bool SPLIT, int J0, int J1, int NTG, int NJ0, int NJ1>
__device__ __forceinline__ void tap_pipelined(const unsigned char* lds, const TapOps& cur, TapOps& nxt, uint32_t nwtap, uint32_t nbtap,
                                              f32x16 (&acc)[2][4]) {
    constexpr int NL = tap_reads<SPLIT, NJ1 - NJ0>(), NM = tap_mfmas<SPLIT, J1 - J0>();
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        tap_read<SPLIT, NTG, NJ0, NJ1>(lds, nwtap, nbtap, i, nxt);
#pragma unroll
        for (int q = i * (NM - NM / 4) / NL; q < (i + 1 < NL ? (i + 1) * (NM - NM / 4) / NL : NM); ++q) tap_mfma<SPLIT, J0, J1>(cur, q, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The main pass of one stage (tap group TG = dy + 1: three taps dx = -1, 0, +1) of a wave's tile: 2 output-channel tiles x the board
// rows J0 .. J1 - 1 of its row half.  Row j under tap dy reads board row 4 half + j + dy, which lies (j + TG) * 128 bytes above the
// row the three per-lane addresses `boff` point at (4 half - 1).  On entry `ops` holds the stage's first tap, on exit the first tap of
// the NEXT stage's main pass (tap group NTG, rows NJ0 .. NJ1 - 1, weights at nwbase, image at nabase).  Per accumulator the
// instructions come in the order they always had: tap 0 .. 8, each al*bh, ah*bl, ah*bh.
template <bool SPLIT, int TG, int J0, int J1, int NTG, int NJ0, int NJ1>
__device__ __forceinline__ void conv_stage_main(const unsigned char* lds, uint32_t wbase, uint32_t abase, uint32_t nwbase, uint32_t nabase,
                                                const uint32_t (&boff)[3], f32x16 (&acc)[2][4], TapOps& ops) {
    TapOps t1, t2;
    tap_pipelined<SPLIT, J0, J1, TG, J0, J1>(lds, ops, t1, wbase + 8192, abase + boff[1], acc);
    tap_pipelined<SPLIT, J0, J1, TG, J0, J1>(lds, t1, t2, wbase + 2 * 8192, abase + boff[2], acc);
    tap_pipelined<SPLIT, J0, J1, NTG, NJ0, NJ1>(lds, t2, ops, nwbase, nabase + boff[0], acc);
}

// The pass of the row that may be skipped (J1 = J0 + 1), with every tap read in place: same addresses, same order per accumulator.
template <bool SPLIT, int TG, int J0, int J1>
__device__ __forceinline__ void conv_stage(const unsigned char* lds, uint32_t wbase, uint32_t abase, const uint32_t (&boff)[3],
                                           f32x16 (&acc)[2][4]) {
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
        h8 bh[4], bl[4];
#pragma unroll
        for (int j = J0; j < J1; ++j) {
            const uint32_t at = abase + boff[tt] + (j + TG) * 128;   // (summed in 32 bits: boff alone may lie below the image)
            bh[j] = *(const h8*)(lds + at);
            if constexpr (SPLIT) bl[j] = *(const h8*)(lds + at + 1024);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const h8 ah = *(const h8*)(lds + wbase + tt * 8192 + m * 512);
            if constexpr (SPLIT) {
                const h8 al = *(const h8*)(lds + wbase + tt * 8192 + m * 512 + 2048);
#pragma unroll
                for (int j = J0; j < J1; ++j) {
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[m][j], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int j = J0; j < J1; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[m][j], 0, 0, 0);
            }
        }
    }
}

// in / out / skip: split activations (header).  Wl: this layer's region-4 weights.  grid = ceil(n / 8) * F / 128, block 512.
// Pipeline: while stage s is computed, stage s+2's weights (and in a chunk's middle stage the next chunk's activations) are in
// flight as LDS-DMA and stage s+1's first tap is read into registers; ONE barrier per stage (it also drains this wave's share
// of the DMA issued a whole stage earlier).  The hazard table is in the header.
// SPLIT: true = raznet-forward-v2 (hi and lo halfs, three matrix instructions per product); false = v3 (hi halfs alone, one).
template <bool SPLIT>
__global__ __launch_bounds__(512, 2) void k_conv3x3_f16x3(const unsigned char* __restrict__ Wl, const float* __restrict__ bias,
                                                          const float* __restrict__ inv_scale_ptr, const unsigned char* in, unsigned char* out,
                                                          const unsigned char* skip, const uint8_t* __restrict__ active, int n, int F,
                                                          unsigned* __restrict__ flag, const uint32_t* __restrict__ n_ptr RAZ_STAMP_PARAM) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the row-half tests below are scalar branches
    RAZ_STAMP_BEGIN;
    if (n_ptr) n = (int)*n_ptr < n ? (int)*n_ptr : n;   // rows 0..n-1 of a compacted batch (raz_leaf_cache.hip): the count lives on the device
    const int noct = F / OCT, nchunks = F / 16;
    // blocks b and b + 8 run on the same XCD (round-robin dispatch): give them the oc tiles of the SAME positions, so the
    // later one finds the activations in that XCD's L2
    const int b = blockIdx.x;
    const int ot = (b >> 3) % noct;
    const int pg = (b / (8 * noct)) * 8 + (b & 7);
    const int p0 = pg * NWAVE, pos = p0 + wv;   // pos: the position whose activations this wave MOVES (it computes for four)
    if (p0 >= n) return;
    const size_t pos_bytes = (size_t)F * 256;
    const unsigned char* in_pos = in + (size_t)(pos < n ? pos : n - 1) * pos_bytes;
    if (tid < 2 * (Z_BYTES / 16)) {   // the zero areas of both images
        const int im = tid / (Z_BYTES / 16), k = tid % (Z_BYTES / 16);
        ((f32x4*)(lds + LDS_ACT + im * ACT_IMG + Z_OFF))[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // the wave's tile (header): waves w and w + 4 share a SIMD, so a SIMD holds one wave of each row half
    const int half = wv >> 2, grp = (wv >> 1) & 1, oh = wv & 1;
    // per-lane LDS byte offsets (inside an activation image) of the B operand for dx = -1, 0, +1, at board row 4 half - 1 (the row
    // tile 0 reads under dy = -1; for the top half it does not exist and is never read).  A file off the board reads the zero area
    // at the bank class of the slot it would have read.
    const int kg = lane >> 5, colpos = grp * 4 + ((lane & 31) >> 3), x = lane & 7;
    uint32_t boff[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int xx = x + t - 1;
        const int at = act_pos_off(colpos) + kg * 2048 + ((4 * half - 1) * 8 + xx) * 16;
        boff[t] = xx >= 0 && xx < 8 ? (uint32_t)at : (uint32_t)(Z_OFF + (at & 255));
    }
    const uint32_t aoff = (uint32_t)(kg * 4096 + oh * 1024 + (lane & 31) * 16);   // + tap*8192 + hl*2048 + mtile*512 inside a weight stage
    f32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;
    const unsigned char* wsrc = Wl + (size_t)ot * nchunks * 3 * W_STAGE + lane * 16;
    const unsigned char* asrc = in_pos + lane * 16;
    // stage `st` = (chunk st / 3, tap group st % 3): 24 weight pieces of 1 KiB (3 per wave) + with tap group 0 this wave's
    // position's four activation planes of that chunk.  !SPLIT: the 12 hi pieces alone (piece p holds the hi halfs when p & 2 is
    // clear: hi piece j is piece (j >> 1) * 4 + (j & 1); every wave moves hi piece wv, waves 0-3 also hi piece 8 + wv) and the two
    // hi planes (0 and 2), to the places they have in the v2 image
    auto issue_w = [&](int c, int tg) {   // into weight buffer tg
        const unsigned char* src = wsrc + (size_t)(c * 3 + tg) * W_STAGE;
        unsigned char* dst = lds + LDS_W + tg * W_STAGE;
        if constexpr (SPLIT) {
#pragma unroll
            for (int i = 0; i < 3; ++i) GLDS16(src + (wv * 3 + i) * 1024, dst + (wv * 3 + i) * 1024);
        } else {
            const int p0w = (wv >> 1) * 4 + (wv & 1);
            GLDS16(src + p0w * 1024, dst + p0w * 1024);
            if (wv < 4) GLDS16(src + (p0w + 16) * 1024, dst + (p0w + 16) * 1024);   // hi piece 8 + wv = piece 16 + p0w
        }
    };
    auto issue_a = [&](int c) {   // into image c & 1
        const unsigned char* a = asrc + (size_t)c * ACT_POS;
        unsigned char* ad = lds + LDS_ACT + (c & 1) * ACT_IMG + act_pos_off(wv);
#pragma unroll
        for (int pl = 0; pl < 4; pl += SPLIT ? 1 : 2) GLDS16(a + pl * 1024, ad + pl * 1024);
    };
    // The stage stream (hazard table in the header).  Weights run TWO stages ahead in three buffers, so at barrier st + 1 stage
    // st + 1 has been in LDS since barrier st, and the last tap of stage st reads its first tap (`ops`) before that barrier: after
    // it the matrix instructions start from registers.  A chunk's activations are issued in the middle stage of the chunk before.
    const uint32_t w0 = (uint32_t)LDS_W + aoff, w1 = w0 + W_STAGE, w2 = w1 + W_STAGE;
    issue_w(0, 0);
    issue_a(0);
    issue_w(0, 1);
    RAZ_STAMP_BARRIER_IN;
    __syncthreads();   // barrier 0: stages 0 and 1, image 0 and the zero areas are in LDS
    RAZ_STAMP_BARRIER_OUT(0);
    TapOps ops;   // the first tap of the coming stage's main pass
#pragma unroll
    for (int k = 0; k < tap_reads<SPLIT, 3>(); ++k) tap_read<SPLIT, 0, 1, 4>(lds, w0, (uint32_t)LDS_ACT + boff[0], k, ops);
    for (int c = 0; c < nchunks; ++c) {
        const uint32_t abase = (uint32_t)(LDS_ACT + (c & 1) * ACT_IMG), nabase = (uint32_t)(LDS_ACT + (~c & 1) * ACT_IMG);
        const bool more = c + 1 < nchunks;   // (uniform over the workgroup)
        // dy = -1 of board row 0 and dy = +1 of board row 7 are whole all-zero B operands: not read, not issued
        // (the row that may be skipped is a pass of its own over the stage's taps: only its two accumulators cross the branch)
        // stage (c, 0): barrier 3 c has been passed
        issue_w(c, 2);
        conv_stage_main<SPLIT, 0, 1, 4, 1, 0, 4>(lds, w0, abase, w1, abase, boff, acc, ops);
        if (half != 0) conv_stage<SPLIT, 0, 0, 1>(lds, w0, abase, boff, acc);
        RAZ_STAMP_BARRIER_IN;
        __syncthreads();   // barrier 3 c + 1: stage (c, 2) has landed (every wave drained its DMA before arriving); buffer 0 and, if c > 0, image c - 1 are free
        RAZ_STAMP_BARRIER_OUT(3 * c + 1);
        if (more) {
            issue_w(c + 1, 0);
            issue_a(c + 1);
        }
        conv_stage_main<SPLIT, 1, 0, 4, 2, 0, 3>(lds, w1, abase, w2, abase, boff, acc, ops);
        RAZ_STAMP_BARRIER_IN;
        __syncthreads();   // barrier 3 c + 2: stage (c + 1, 0) and image c + 1 have landed; buffer 1 is free
        RAZ_STAMP_BARRIER_OUT(3 * c + 2);
        if (more) issue_w(c + 1, 1);
        // (after the last chunk the read-ahead takes what lies in buffer 0 and the other image: nothing is in flight there and nobody uses it)
        conv_stage_main<SPLIT, 2, 0, 3, 0, 1, 4>(lds, w2, abase, w0, nabase, boff, acc, ops);
        if (half != 1) conv_stage<SPLIT, 2, 3, 4>(lds, w2, abase, boff, acc);
        if (more) {
            RAZ_STAMP_BARRIER_IN;
            __syncthreads();   // barrier 3 c + 3: stage (c + 1, 1) has landed; buffer 2 is free
            RAZ_STAMP_BARRIER_OUT(3 * c + 3);
        }
    }
    RAZ_STAMP_AT(2);
    // epilogue.  D layout: column = lane & 31 = (position, file) inside tile j, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = channel in
    // the 32-tile: a lane holds channels 4 kg .. 4 kg + 3 of every 8-channel group, for its column of the four board rows.  The halves
    // of the wave trade (halves_trade) tiles 2 k and 2 k + 1: afterwards lane l holds all 8 channels of its column in board row
    // 4 half + 2 k + kg, one whole 16-byte unit of the layout per plane, so a wave reads and writes 128-byte runs (the 8 files of a
    // row) of its four positions' planes.  The arithmetic per element is what it always was.
    const int lpos = p0 + colpos;   // the position this lane's column belongs to
    const bool live = lpos < n && (!active || active[lpos]);
    if (!__any(live)) return;
    const float inv_scale = *inv_scale_ptr;
    const size_t lane_off = (size_t)(live ? lpos : p0) * pos_bytes + (size_t)((4 * half + kg) * 8 + x) * 16;   // + k * 256: board row + 2
    unsigned char* out_pos = out + lane_off;
    const unsigned char* skip_pos = skip ? skip + lane_off : nullptr;
    // the skip rows of the next (32-tile, row pair) are asked for before this one is computed (out may BE skip: a lane reads exactly
    // the 16 bytes it overwrites later, so the loads may run ahead of the stores of other units)
    h8 skh[2][4], skl[2][4];
    auto load_skip = [&](int it) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int oc8 = ot * OCT + oh * 64 + (it >> 1) * 32 + q * 8;
            const size_t unit = (size_t)(oc8 >> 4) * ACT_POS + (size_t)((oc8 >> 3) & 1) * 2048 + (size_t)(it & 1) * 256;
            skh[it & 1][q] = *(const h8*)(skip_pos + unit);
            if constexpr (SPLIT) skl[it & 1][q] = *(const h8*)(skip_pos + unit + 1024);
        }
    };
    if (skip_pos && live) load_skip(0);
    bool over = false;
#pragma unroll
    for (int it = 0; it < 4; ++it) {   // it = (32-tile m, row pair k)
        const int m = it >> 1, k = it & 1;
        if (skip_pos && live && it + 1 < 4) load_skip(it + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int oc8 = ot * OCT + oh * 64 + m * 32 + q * 8;   // this lane's 8-channel group (wave-uniform: the bias comes by scalar loads)
            const size_t unit = (size_t)(oc8 >> 4) * ACT_POS + (size_t)((oc8 >> 3) & 1) * 2048 + (size_t)k * 256;
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) halves_trade(acc[m][2 * k][q * 4 + j], acc[m][2 * k + 1][q * 4 + j], kg, v[j], v[4 + j]);
            if (!live) continue;   // (after the trade: every lane takes part in it)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * inv_scale + bias[oc8 + j];
            if (skip_pos) {
                const h8 sh = skh[it & 1][q];
                if constexpr (SPLIT) {
                    const h8 sl = skl[it & 1][q];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = v[j] + ((float)sh[j] + (float)sl[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = v[j] + (float)sh[j];
                }
            }
            h8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float r = v[j] > 0.0f ? v[j] : 0.0f;
                over |= !(r < 60000.0f);
                hi[j] = (_Float16)r;
                lo[j] = (_Float16)(r - (float)hi[j]);
            }
            *(h8*)(out_pos + unit) = hi;
            if constexpr (SPLIT) *(h8*)(out_pos + unit + 1024) = lo;
        }
    }
    if (live && over) flag[(size_t)lpos * RAZ_NET_ROWFLAG_WORDS] = 1u;   // an activation beyond the f16 range: this ROW is evaluated again by the exact-f32 kernel (raz_net_repair_rows)
    RAZ_STAMP_END;
}

// Layer 0: 2 bit planes -> F channels, exact f32 chains as in k_conv0_wide (per output: acc = bias; for each tap fmaf(x0, w, acc)
// then fmaf(x1, w, acc)), written in the split layout.  A workgroup takes TWO rows (2 b and 2 b + 1); lane = square; the 16-channel
// chunks are spread over its 4 waves (wave w takes chunks w, w + 4, ...).  A lane carries the same output channel of both rows as
// one register pair, so a chain step is one v_pk_fma_f32 whose weight is a scalar register read by both halves: the weights reach
// the lanes by scalar loads, each fetched once for two rows.  8 output channels (one 16-byte unit per plane and row) are live at a
// time: under 80 VGPRs, so a SIMD holds 6 waves, and they hide the scalar loads and the store drain of one another - the kernel
// writes F * 256 bytes per row and is otherwise idle.  The fully unrolled 16 x 18 form before it took 256 VGPRs and spilled
// its weights: one wave per SIMD, every latency exposed.  !SPLIT (v3): the hi planes alone are written.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int CONV0_ROWS = 2;   // rows per workgroup

template <bool SPLIT>
__global__ __launch_bounds__(256, 6) void k_conv0_split(const float* __restrict__ W0, const raz_bb* __restrict__ own,
                                                        const raz_bb* __restrict__ enemy, const uint8_t* __restrict__ active,
                                                        unsigned char* out, int n, int F, unsigned* __restrict__ flag,
                                                        const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_ptr) {
    const int posA = blockIdx.x * CONV0_ROWS, posB = posA + 1, lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the weight reads below stay scalar loads
    // the forward's first kernel clears the per-row range flags (word 0 of every row's area) and the repair counter (word 1 of row 0's)
    if (threadIdx.x == 0) {
        flag[(size_t)posA * RAZ_NET_ROWFLAG_WORDS] = 0u;
        if (posB < n) flag[(size_t)posB * RAZ_NET_ROWFLAG_WORDS] = 0u;
        if (posA == 0) flag[1] = 0u;
    }
    __syncthreads();
    if (n_ptr) n = (int)*n_ptr < n ? (int)*n_ptr : n;
    const bool liveA = posA < n && (list || !active || active[posA]);
    const bool liveB = posB < n && (list || !active || active[posB]);
    if (!liveA && !liveB) return;
    // compacted batch: row `pos` holds the leaf of exchange row list[pos].  A row that is not live computes on an empty board and stores nothing
    raz_bb bo[2] = {0, 0}, be[2] = {0, 0};
    if (liveA) {
        const size_t src = list ? list[posA] : (size_t)posA;
        bo[0] = own[src];
        be[0] = enemy[src];
    }
    if (liveB) {
        const size_t src = list ? list[posB] : (size_t)posB;
        bo[1] = own[src];
        be[1] = enemy[src];
    }
    f32x2 x0[9], x1[9];   // (row A, row B)
#pragma unroll
    for (int t = 0; t < 9; ++t) {   // bb_tap_planes for two rows at once: one predicate and one shift count serve both
        int s;
        const bool ok = bb_tap(lane, t, &s);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            x0[t][k] = ok ? (float)(uint32_t)((bo[k] >> s) & 1) : 0.0f;
            x1[t][k] = ok ? (float)(uint32_t)((be[k] >> s) & 1) : 0.0f;
        }
    }
    const float* bias = W0 + (size_t)F * 18;
    unsigned char* op = out + (size_t)posA * F * 256 + lane * 16;   // row B: + F * 256
    bool overA = false, overB = false;
    for (int ocb = wv; ocb < F / 16; ocb += 4) {
#pragma unroll 1
        for (int g = 0; g < 2; ++g) {   // the chunk's two 8-channel groups
            f32x2 acc[8];
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const float b = bias[ocb * 16 + g * 8 + o];
                acc[o] = (f32x2){b, b};
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float* wt = W0 + ((size_t)ocb * 9 + t) * 32 + g * 8;
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const float w = wt[o];
                    acc[o] = __builtin_elementwise_fma(x0[t], (f32x2){w, w}, acc[o]);
                }
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const float w = wt[16 + o];
                    acc[o] = __builtin_elementwise_fma(x1[t], (f32x2){w, w}, acc[o]);
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!(k ? liveB : liveA)) continue;
                h8 hi, lo;
                bool over = false;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float r = acc[j][k] > 0.0f ? acc[j][k] : 0.0f;
                    over |= !(r < 60000.0f);
                    hi[j] = (_Float16)r;
                    lo[j] = (_Float16)(r - (float)hi[j]);
                }
                if (k) overB |= over;
                else overA |= over;
                unsigned char* o16 = op + (size_t)k * F * 256 + (size_t)ocb * ACT_POS + (g * 2) * 1024;
                *(h8*)o16 = hi;
                if constexpr (SPLIT) *(h8*)(o16 + 1024) = lo;
            }
        }
    }
    if (overA) flag[(size_t)posA * RAZ_NET_ROWFLAG_WORDS] = 1u;
    if (overB) flag[(size_t)posB * RAZ_NET_ROWFLAG_WORDS] = 1u;
}

// Heads (raz_net_heads.h: exact f32 chains), reading the trunk output in the split layout, 16 bytes a load: x = hi + lo (exact in
// f32); !SPLIT (v3): x = hi, the lo planes are not read.
template <bool SPLIT>
__global__ __launch_bounds__(64) void k_heads_split(const float* __restrict__ H, const unsigned char* trunk,
                                                    const uint8_t* __restrict__ active, float* __restrict__ policy,
                                                    float* __restrict__ value, int n, int F, int V,
                                                    const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_ptr) {
    extern __shared__ __attribute__((aligned(16))) float head[];  // ph[128] vh[64] h1[V]
    const int pos = blockIdx.x, lane = threadIdx.x;
    if (n_ptr) n = (int)*n_ptr < n ? (int)*n_ptr : n;
    if (pos >= n || (!list && active && !active[pos])) return;
    const size_t dst = list ? list[pos] : (size_t)pos;   // results go back to the leaf-exchange row
    const HeadWeights h = head_weights(H, F, V);
    const unsigned char* a = trunk + (size_t)pos * F * 256 + lane * 16;
    float p0 = h.pol_b[0], p1 = h.pol_b[1], v0 = h.val_b[0];
    for (int c = 0; c < F / 16; ++c) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const h8 hi = *(const h8*)(a + (size_t)c * ACT_POS + (g * 2 + 0) * 1024);
            h8 lo = hi;
            if constexpr (SPLIT) lo = *(const h8*)(a + (size_t)c * ACT_POS + (g * 2 + 1) * 1024);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                heads_1x1_step(h, F, c * 16 + g * 8 + j, SPLIT ? (float)hi[j] + (float)lo[j] : (float)hi[j], p0, p1, v0);
        }
    }
    heads_finish(h, V, p0, p1, v0, head, lane, policy + dst * 64, value + dst);
}

}  // namespace

// Host side of raz_net_load for region 4: `src` = the blob's float parameters, `dst` = the device image being built.
void raz_net_build_f16x3(const float* src, float* dst, int F, int R, int V) {
    const float* lsrc = src + ((size_t)F * 18 + F);   // layer 1
    float* scales = dst + f16x3_scale_off(F, R, V);
    const int nchunks = F / 16, noct = F / 128;
    for (int l = 1; l < 2 * R + 1; ++l) {
        float mx = 0.f;
        for (size_t i = 0; i < (size_t)F * F * 9; ++i) mx = fmaxf(mx, fabsf(lsrc[i]));
        int e = 0;
        if (mx > 0.f) frexpf(mx, &e);                 // mx = f * 2^e, f in [0.5, 1)  =>  mx * 2^(15 - e) in [2^14, 2^15)
        const float S = ldexpf(1.0f, 15 - e);
        scales[l - 1] = ldexpf(1.0f, e - 15);
        _Float16* w = (_Float16*)(dst + f16x3_layer_off(F, R, V, l));
        for (int ot = 0; ot < noct; ++ot)
            for (int c = 0; c < nchunks; ++c)
                for (int t = 0; t < 9; ++t)
                    for (int kg = 0; kg < 2; ++kg)
                        for (int o = 0; o < 128; ++o)
                            for (int j = 0; j < 8; ++j) {
                                const int oc = ot * 128 + o, ic = c * 16 + kg * 8 + j;
                                const float v = lsrc[((size_t)oc * F + ic) * 9 + t] * S;
                                const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
                                const size_t stage = ((size_t)ot * nchunks + c) * 3 + t / 3;
                                const size_t base = stage * (W_STAGE / 2) + ((size_t)(t % 3) * 2 + kg) * 2 * 128 * 8;
                                w[base + (size_t)o * 8 + j] = hi;
                                w[base + 128 * 8 + (size_t)o * 8 + j] = lo;
                            }
        lsrc += (size_t)F * F * 9 + F;
    }
}

// The heads over a trunk output in the split layout (split = false: over its hi planes alone, raznet-forward-v3).
static int heads_launch(bool split, const float* W, int F, int R, int V, const unsigned char* trunk, const uint8_t* active, float* policy,
                        float* value, size_t n, hipStream_t s, const uint32_t* list, const uint32_t* n_ptr) {
    const auto heads = split ? k_heads_split<true> : k_heads_split<false>;
    hipLaunchKernelGGL(heads, dim3((unsigned)n), dim3(64), heads_lds_floats(V) * sizeof(float), s,
                       W + heads_off(F, R), trunk, active, policy, value, (int)n, F, V, list, n_ptr);
    return raz_check_launch("raz_net_forward (split heads)");
}
int raz_net_heads_split(const float* W, int F, int R, int V, const unsigned char* trunk, const uint8_t* active, float* policy, float* value,
                        size_t n, hipStream_t s, const uint32_t* list, const uint32_t* n_ptr) {
    return heads_launch(true, W, F, R, V, trunk, active, policy, value, n, s, list, n_ptr);
}

// two activation buffers, then a 64-byte area per row for its range flag (raz_internal.h raz_net_repair_rows): linear in n
size_t raz_net_f16x3_scratch_bytes(int F, size_t n) { return n * ((size_t)2 * F * 256 + RAZ_NET_ROWFLAG_WORDS * 4); }

// !f16x3_repairs(F, V) (a row's f32 activations do not fit a CU's LDS, so there is no in-forward repair): any row out of range raises the sticky flag
__global__ __launch_bounds__(256) void k_flag_unrepaired(const unsigned* __restrict__ rowflag, unsigned* __restrict__ sticky, int n,
                                                         const uint32_t* __restrict__ n_ptr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int rows = n_ptr ? ((int)*n_ptr < n ? (int)*n_ptr : n) : n;
    if (i < rows && rowflag[(size_t)i * RAZ_NET_ROWFLAG_WORDS]) atomicOr(sticky, 1u);
}
static int raz_net_flag_unrepaired(const unsigned* rowflag, unsigned* sticky, size_t n, const uint32_t* n_ptr, hipStream_t s) {
    hipLaunchKernelGGL(k_flag_unrepaired, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rowflag, sticky, (int)n, n_ptr);
    return raz_check_launch("raz_net_forward (range flags)");
}

// The sticky range flag lives in the device weight image, after the per-layer scales (raz_net_layout.h leaves 64 floats there).
unsigned* raz_net_f16x3_flag(const float* W, int F, int R, int V) { return (unsigned*)(W + f16x3_scale_off(F, R, V) + (size_t)2 * R + 8); }

// split: true = raznet-forward-v2, false = raznet-forward-v3 (the hi halfs alone; same scratch layout, the lo planes stay untouched).
// list / n_ptr (both or neither; engine-internal, raz_leaf_cache.hip): evaluate only the exchange rows list[0 .. *n_ptr), packed
// densely in the activation buffers - *n_ptr lives on the device, so every launch keeps its full grid and surplus blocks exit.
int raz_net_forward_f16x3(const float* W, int F, int R, int V, const uint64_t* own, const uint64_t* enemy,
                          const uint8_t* active, float* policy, float* value, size_t n, void* scratch, size_t scratch_bytes,
                          hipStream_t s, const uint32_t* list, const uint32_t* n_ptr, bool split) {
    if (!scratch || scratch_bytes < raz_net_f16x3_scratch_bytes(F, n))
        return raz_fail(RAZ_ENOMEM, "raz_net_forward: scratch too small (raz_net_scratch_bytes)");
    unsigned char* bufA = (unsigned char*)scratch;
    unsigned char* bufT = bufA + (size_t)n * F * 256;
    unsigned* sticky = raz_net_f16x3_flag(W, F, R, V);
    unsigned* flag = (unsigned*)(bufT + (size_t)n * F * 256);   // per-row range flags
    const float* scales = W + f16x3_scale_off(F, R, V);
    const auto conv = split ? k_conv3x3_f16x3<true> : k_conv3x3_f16x3<false>;   // (v3 keeps v2's LDS image, lo halves unused)
    // the kernel's LDS image exceeds the default dynamic limit
    if (const int rc = raz_lds_opt_in((const void*)conv, LDS_BYTES, "raz_net_forward: hipFuncSetAttribute")) return rc;
    const unsigned conv_threads = NWAVE * 64;
    const auto conv0 = split ? k_conv0_split<true> : k_conv0_split<false>;
    hipLaunchKernelGGL(conv0, dim3((unsigned)((n + CONV0_ROWS - 1) / CONV0_ROWS)), dim3(256), 0, s, W + conv_off(F, 0), (const raz_bb*)own,
                       (const raz_bb*)enemy, active, bufA, (int)n, F, flag, list, n_ptr);
    const unsigned groups = (unsigned)((n + NWAVE - 1) / NWAVE);
    const unsigned tiles = ((groups + 7) / 8) * 8 * (unsigned)(F / 128);
    const unsigned grid = tiles;
    for (int r = 0; r < R; ++r) {
        const int l1 = 1 + 2 * r, l2 = 2 + 2 * r;
        hipLaunchKernelGGL(conv, dim3(grid), dim3(conv_threads), LDS_BYTES, s,
                           (const unsigned char*)(W + f16x3_layer_off(F, R, V, l1)), W + conv_off(F, l1) + (size_t)F * 9 * F,
                           scales + (l1 - 1), (const unsigned char*)bufA, bufT, (const unsigned char*)nullptr, list ? nullptr : active, (int)n, F, flag, n_ptr RAZ_STAMP_ARG);
        hipLaunchKernelGGL(conv, dim3(grid), dim3(conv_threads), LDS_BYTES, s,
                           (const unsigned char*)(W + f16x3_layer_off(F, R, V, l2)), W + conv_off(F, l2) + (size_t)F * 9 * F,
                           scales + (l2 - 1), (const unsigned char*)bufT, bufA, (const unsigned char*)bufA, list ? nullptr : active, (int)n, F, flag, n_ptr RAZ_STAMP_ARG);
    }
    const int rc = heads_launch(split, W, F, R, V, bufA, active, policy, value, n, s, list, n_ptr);
    if (rc != RAZ_OK) return rc;
    // rows whose activations left the f16 range: the same position through the exact-f32 chains (raznet-forward-v1), so a row's
    // answer is a function of its position alone - v2's when it stays in range, v1's when it does not
    if (!f16x3_repairs(F, V))   // (F > 256, or 256 with V > 8000: a row does not fit a CU's LDS - not repaired, see raz_net_range_check)
        return raz_net_flag_unrepaired(flag, sticky, n, n_ptr, s);
    return raz_net_repair_rows(W, F, R, V, own, enemy, policy, value, n, flag, sticky, list, n_ptr, s);
}
