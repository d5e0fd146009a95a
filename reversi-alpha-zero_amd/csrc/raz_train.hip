// raz_train.hip — raznet-train-v1: one training step of the policy/value net on the device, exact f32.
//
// The trainer keeps the UNFOLDED graph (Conv2D + bias, BatchNorm in training mode, ReLU, residual add, the two heads), the
// momentum buffers and the moving statistics in caller-owned device memory, beside the saved tensors of one batch of at most
// max_batch rows.  The three 3x3 products of every trunk layer run on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: a
// k-ordered fmaf chain) for every supported width (F % 16 == 0):
//   k_tconv<false>   forward          out[b][oc][sq]  = bias[oc] + sum_{ic,t} W[oc][ic][t] in[b][ic][sq + off(t)]
//   k_tconv<true>    input gradient   dx[b][ic][sq]   = sum_{oc,t} W[oc][ic][8-t] dy[b][oc][sq + off(t)]  (taps rotated, roles swapped:
//                                     the weights are re-indexed while they are staged, no second copy exists)
//   k_twgrad         weight gradient  dW[oc][ic][t]   = sum_{b,sq} dy[b][oc][sq] x[b][ic][sq + off(t)]; positions are split over
//                                     at most 32 workgroups that write partial sums, k_twgrad_fold adds them in split order
// Activations are [B][C][64] f32; zero-haloed LDS planes (row stride 12) make the taps immediate offsets, as in raz_net_wide.hip.
// Everything else is bandwidth-bound and written plainly: one workgroup per channel for the BatchNorm sums, one thread per
// element for the dense layers.  No floating-point atomics anywhere: every sum over the batch has one fixed order, so two
// trainers given the same state and batches hold the same bytes.  Per-channel and per-weight sums over the batch outside the
// matrix products accumulate in f64 and round once.
//
// raznet-train-v2 (precision RAZ_TRAIN_F16X3, opt-in through raz_trainer_create2) is the same step with the three trunk products on
// the f16 matrix cores over split operands: raz_train_f16x3.h.  Precision RAZ_TRAIN_F32 launches exactly what it always did.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <new>
#include <vector>
#include "raz_bitboard.h"
#include "raz_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int PS = 136;    // haloed plane stride of k_tconv (floats)
constexpr int PSW = 132;   // ... of k_twgrad
constexpr int DS = 68;     // row stride of k_twgrad's dy tile
constexpr int MAX_SPLIT = 32;
constexpr float BN_EPS = 1e-3f;

__device__ __forceinline__ int pidx(int sq) { return ((sq >> 3) + 1) * 12 + (sq & 7) + 4; }

// fixed-order sum of one double per thread over a 256-thread block; every thread receives the total
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s);
    return v;
}

// ---- the stem: 2 bit-planes gathered by idx -> F raw channels.  grid = B, block = 64 (lane = square) -------------------------
__global__ __launch_bounds__(64) void k_stem_fwd(const float* __restrict__ W /*[F][2][9]*/, const float* __restrict__ bias,
                                                 const raz_bb* __restrict__ own, const raz_bb* __restrict__ enemy,
                                                 const uint32_t* __restrict__ idx, float* __restrict__ y, int F) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const uint32_t row = idx[b];
    const raz_bb bo = own[row], be = enemy[row];
    float x0[9], x1[9];
    bb_tap_planes(bo, be, lane, x0, x1);
    for (int oc = 0; oc < F; ++oc) {
        float acc = bias[oc];
        const float* w = W + (size_t)oc * 18;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(x0[t], w[t], acc);
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(x1[t], w[9 + t], acc);
        y[((size_t)b * F + oc) * 64 + lane] = acc;
    }
}

// dW0[oc][c][t] = sum_{b,sq} dy[b][oc][sq] plane_c[b][sq + off(t)] + 2 l2 w.  grid = F, block = 64.
__global__ __launch_bounds__(64) void k_stem_wgrad(const float* __restrict__ dy, const raz_bb* __restrict__ own,
                                                   const raz_bb* __restrict__ enemy, const uint32_t* __restrict__ idx,
                                                   const float* __restrict__ W, float* __restrict__ dW, int B, int F, float l2) {
    const int oc = blockIdx.x, lane = threadIdx.x;
    double acc[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) acc[i] = 0.0;
    for (int b = 0; b < B; ++b) {
        const uint32_t row = idx[b];
        const raz_bb bo = own[row], be = enemy[row];
        const double g = (double)dy[((size_t)b * F + oc) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int s;
            const bool ok = bb_tap(lane, t, &s);
            if (ok && ((bo >> s) & 1)) acc[t] = acc[t] + g;
            if (ok && ((be >> s) & 1)) acc[9 + t] = acc[9 + t] + g;
        }
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) dW[(size_t)oc * 18 + i] = (float)(s + 2.0 * (double)l2 * (double)W[(size_t)oc * 18 + i]);
    }
}

// ---- 3x3 convolution on the f32 matrix instruction.  in [B][Cin][64] -> out [B][Cout][64] (+ add).  T: the input-gradient
// form (weights read as W[cin][cout][8 - t]).  grid = (ceil(B / 4), Cout / 16), block = 256: wave = 1 position x 16 channels
// x 64 squares = 4 accumulators of 16x16. ------------------------------------------------------------------------------------
template <bool T>
__global__ __launch_bounds__(256) void k_tconv(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ in,
                                               float* out, const float* add, int B, int Cin, int Cout) {
    __shared__ __attribute__((aligned(16))) float actP[4 * 16 * PS];
    __shared__ float wS[9 * 16 * 16];   // [t][ic][oc]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int p0 = blockIdx.x * 4, oc0 = blockIdx.y * 16;
    const int pos = p0 + wv;
    for (int j = tid; j < 4 * 16 * PS / 4; j += 256) ((f32x4*)actP)[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float bv = bias ? bias[oc0 + 4 * (lane >> 4) + r] : 0.0f;
#pragma unroll
        for (int st = 0; st < 4; ++st) acc[st][r] = bv;
    }
    const float* bbase = actP + (wv * 16 + (lane >> 4)) * PS;
    int sqoff[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) sqoff[st] = pidx(st * 16 + (lane & 15));
    for (int c = 0; c < Cin / 16; ++c) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int pp = q >> 8, ch = (q >> 4) & 15, r4 = q & 15;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (p0 + pp < B) v = *(const f32x4*)(in + ((size_t)(p0 + pp) * Cin + c * 16 + ch) * 64 + r4 * 4);
            *(f32x4*)(actP + (pp * 16 + ch) * PS + ((r4 >> 1) + 1) * 12 + 4 + (r4 & 1) * 4) = v;
        }
        for (int e = tid; e < 2304; e += 256) {
            const int oc = e / 144, r = e % 144, ic = r / 9, t = r % 9;
            const float w = T ? W[((size_t)(c * 16 + ic) * Cout + oc0 + oc) * 9 + (8 - t)]
                              : W[((size_t)(oc0 + oc) * Cin + c * 16 + ic) * 9 + t];
            wS[(t * 16 + ic) * 16 + oc] = w;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int toff = (t / 3 - 1) * 12 + (t % 3 - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = wS[(t * 16 + 4 * j + (lane >> 4)) * 16 + (lane & 15)];
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const float bvl = bbase[4 * j * PS + sqoff[st] + toff];
                    acc[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bvl, acc[st], 0, 0, 0);
                }
            }
        }
    }
    if (pos >= B) return;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int oc = oc0 + 4 * (lane >> 4) + r;
            const size_t o = ((size_t)pos * Cout + oc) * 64 + st * 16 + (lane & 15);
            float v = acc[st][r];
            if (add) v = v + add[o];
            out[o] = v;
        }
}

// Weight gradient, partial sums.  grid = (ceil(Cout / 64), Cin / 16, S), block = 256: wave = 16 out channels x 16 in channels
// x 9 taps; split s takes positions s, s + S, ...  partial: [S][Cout][Cin][9].
__global__ __launch_bounds__(256) void k_twgrad(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                int B, int Cin, int Cout) {
    __shared__ __attribute__((aligned(16))) float xP[16 * PSW];
    __shared__ __attribute__((aligned(16))) float dS[64 * DS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ocg = blockIdx.x * 64, ic0 = blockIdx.y * 16, s = blockIdx.z, S = gridDim.z;
    const bool work = ocg + wv * 16 < Cout;
    for (int j = tid; j < 16 * PSW / 4; j += 256) ((f32x4*)xP)[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int b = s; b < B; b += S) {
        __syncthreads();
        {
            const int ch = tid >> 4, r4 = tid & 15;
            const f32x4 v = *(const f32x4*)(x + ((size_t)b * Cin + ic0 + ch) * 64 + r4 * 4);
            *(f32x4*)(xP + ch * PSW + ((r4 >> 1) + 1) * 12 + 4 + (r4 & 1) * 4) = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int oc = q >> 4, r4 = q & 15;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (ocg + oc < Cout) v = *(const f32x4*)(dy + ((size_t)b * Cout + ocg + oc) * 64 + r4 * 4);
            *(f32x4*)(dS + oc * DS + r4 * 4) = v;
        }
        __syncthreads();
        if (work) {
#pragma unroll 4
            for (int k = 0; k < 16; ++k) {
                const int sq = 4 * k + (lane >> 4);
                const float a = dS[(wv * 16 + (lane & 15)) * DS + sq];
                const float* xb = xP + (lane & 15) * PSW + pidx(sq);
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[(t / 3 - 1) * 12 + (t % 3 - 1)], acc[t], 0, 0, 0);
            }
        }
    }
    if (!work) return;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int oc = ocg + wv * 16 + 4 * (lane >> 4) + r, ic = ic0 + (lane & 15);
            partial[(((size_t)s * Cout + oc) * Cin + ic) * 9 + t] = acc[t][r];
        }
}

// dW[e] = (partial[0][e] + partial[1][e] + ...) + 2 l2 w[e]
__global__ __launch_bounds__(256) void k_twgrad_fold(const float* __restrict__ partial, const float* __restrict__ W, float* __restrict__ dW,
                                                     size_t n, int S, float l2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = partial[e];
    for (int i = 1; i < S; ++i) s = s + partial[(size_t)i * n + e];
    dW[e] = s + (2.0f * l2) * W[e];
}

// ---- BatchNorm in training mode.  grid = C, block = 256.  y [B][C][64] -> a = relu(gamma (y - mean) inv + beta (+ skip)) ------
__global__ __launch_bounds__(256) void k_bn_fwd(const float* __restrict__ y, float* __restrict__ a, const float* __restrict__ skip,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ bmean,
                                                float* __restrict__ bvar, float* __restrict__ binv, float* mov_mean, float* mov_var, int B,
                                                int C) {
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x, n = B * 64;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s = s + (double)y[((size_t)(i >> 6) * C + c) * 64 + (i & 63)];
    const double mean = block_sum(s, red) / (double)n;
    s = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double d = (double)y[((size_t)(i >> 6) * C + c) * 64 + (i & 63)] - mean;
        s = s + d * d;
    }
    const double var = block_sum(s, red) / (double)n;
    const float fmean = (float)mean, finv = (float)(1.0 / sqrt(var + (double)BN_EPS));
    const float g = gamma[c], be = beta[c];
    for (int i = tid; i < n; i += 256) {
        const size_t o = ((size_t)(i >> 6) * C + c) * 64 + (i & 63);
        float v = (y[o] - fmean) * finv * g + be;
        if (skip) v = v + skip[o];
        a[o] = v > 0.0f ? v : 0.0f;
    }
    if (tid == 0) {
        bmean[c] = fmean;
        bvar[c] = (float)var;
        binv[c] = finv;
        if (mov_mean) {   // momentum 0.99; the moving variance takes the unbiased batch variance
            const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
            mov_mean[c] = 0.99f * mov_mean[c] + 0.01f * fmean;
            mov_var[c] = 0.99f * mov_var[c] + 0.01f * (float)unb;
        }
    }
}

// g: gradient at the ReLU's output; masked with a > 0 (written back when keep), then through the normalisation:
// dbeta = sum g, dgamma = sum g xhat, dy = gamma inv (g - dbeta / n - xhat dgamma / n).  grid = C, block = 256.
__global__ __launch_bounds__(256) void k_bn_bwd(float* g, const float* __restrict__ a, const float* __restrict__ y,
                                                const float* __restrict__ bmean, const float* __restrict__ binv,
                                                const float* __restrict__ gamma, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                float* __restrict__ dy, int keep, int B, int C) {
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x, n = B * 64;
    const float mean = bmean[c], inv = binv[c];
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t o = ((size_t)(i >> 6) * C + c) * 64 + (i & 63);
        const float gm = a[o] > 0.0f ? g[o] : 0.0f;
        const float xh = (y[o] - mean) * inv;
        s1 = s1 + (double)gm;
        s2 = s2 + (double)gm * (double)xh;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float m1 = (float)(s1 / (double)n), m2 = (float)(s2 / (double)n), k = gamma[c] * inv;
    for (int i = tid; i < n; i += 256) {
        const size_t o = ((size_t)(i >> 6) * C + c) * 64 + (i & 63);
        const float gm = a[o] > 0.0f ? g[o] : 0.0f;
        const float xh = (y[o] - mean) * inv;
        dy[o] = k * (gm - m1 - xh * m2);
        if (keep) g[o] = gm;
    }
    if (tid == 0) {
        dgamma[c] = (float)s2;
        dbeta[c] = (float)s1;
    }
}

// ---- the heads' 1x1 convolutions.  grid = B, block = 64 ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hconv_fwd(const float* __restrict__ Wp, const float* __restrict__ bp, const float* __restrict__ Wv,
                                                  const float* __restrict__ bv, const float* __restrict__ trunk, float* __restrict__ yp,
                                                  float* __restrict__ yv, int F) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* a = trunk + (size_t)b * F * 64 + lane;
    float p0 = bp[0], p1 = bp[1], v0 = bv[0];
    for (int ic = 0; ic < F; ++ic) {
        const float xv = a[(size_t)ic * 64];
        p0 = fmaf(xv, Wp[ic], p0);
        p1 = fmaf(xv, Wp[F + ic], p1);
        v0 = fmaf(xv, Wv[ic], v0);
    }
    yp[((size_t)b * 2) * 64 + lane] = p0;
    yp[((size_t)b * 2 + 1) * 64 + lane] = p1;
    yv[(size_t)b * 64 + lane] = v0;
}

// grid = F (input channel), block = 64 (lane = square)
__global__ __launch_bounds__(64) void k_hconv_wgrad(const float* __restrict__ dyp, const float* __restrict__ dyv, const float* __restrict__ trunk,
                                                    const float* __restrict__ Wp, const float* __restrict__ Wv, float* __restrict__ dWp,
                                                    float* __restrict__ dWv, int B, int F, float l2) {
    const int ic = blockIdx.x, lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double xv = (double)trunk[((size_t)b * F + ic) * 64 + lane];
        s0 = s0 + xv * (double)dyp[((size_t)b * 2) * 64 + lane];
        s1 = s1 + xv * (double)dyp[((size_t)b * 2 + 1) * 64 + lane];
        s2 = s2 + xv * (double)dyv[(size_t)b * 64 + lane];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        dWp[ic] = (float)(s0 + 2.0 * (double)l2 * (double)Wp[ic]);
        dWp[F + ic] = (float)(s1 + 2.0 * (double)l2 * (double)Wp[F + ic]);
        dWv[ic] = (float)(s2 + 2.0 * (double)l2 * (double)Wv[ic]);
    }
}

// dtrunk[b][ic][sq] = Wp[0][ic] dyp[b][0][sq] + Wp[1][ic] dyp[b][1][sq] + Wv[ic] dyv[b][sq]
__global__ __launch_bounds__(256) void k_hconv_dgrad(const float* __restrict__ dyp, const float* __restrict__ dyv, const float* __restrict__ Wp,
                                                     const float* __restrict__ Wv, float* __restrict__ g, size_t n, int F) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int sq = (int)(e & 63), ic = (int)((e >> 6) % (size_t)F);
    const size_t b = (e >> 6) / (size_t)F;
    float v = Wp[ic] * dyp[(b * 2) * 64 + sq];
    v = fmaf(Wp[F + ic], dyp[(b * 2 + 1) * 64 + sq], v);
    v = fmaf(Wv[ic], dyv[b * 64 + sq], v);
    g[e] = v;
}

// ---- dense layers, kernels stored (in, out) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_fwd(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ Y, int B, int In, int Out, int relu) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * Out) return;
    const int o = (int)(e % (size_t)Out);
    const size_t b = e / (size_t)Out;
    float acc = bias[o];
    for (int i = 0; i < In; ++i) acc = fmaf(X[b * In + i], W[(size_t)i * Out + o], acc);
    Y[e] = (relu && acc <= 0.0f) ? 0.0f : acc;
}

// dW[i][o] = sum_b X[b][i] dY[b][o] + 2 l2 W[i][o];  db[o] = sum_b dY[b][o]  (thread e = i * Out + o, i == In: the bias)
__global__ __launch_bounds__(256) void k_dense_wgrad(const float* __restrict__ X, const float* __restrict__ dY, const float* __restrict__ W,
                                                     float* __restrict__ dW, float* __restrict__ db, int B, int In, int Out, float l2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)(In + 1) * Out) return;
    const int o = (int)(e % (size_t)Out), i = (int)(e / (size_t)Out);
    double s = 0.0;
    if (i < In) {
        for (int b = 0; b < B; ++b) s = s + (double)X[(size_t)b * In + i] * (double)dY[(size_t)b * Out + o];
        dW[e] = (float)(s + 2.0 * (double)l2 * (double)W[e]);
    } else {
        for (int b = 0; b < B; ++b) s = s + (double)dY[(size_t)b * Out + o];
        db[o] = (float)s;
    }
}

// dX[b][i] = sum_o W[i][o] dY[b][o], zero where mask[b][i] <= 0 (mask: the ReLU's output, nullable)
__global__ __launch_bounds__(256) void k_dense_dgrad(const float* __restrict__ dY, const float* __restrict__ W, const float* __restrict__ mask,
                                                     float* __restrict__ dX, int B, int In, int Out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * In) return;
    const int i = (int)(e % (size_t)In);
    const size_t b = e / (size_t)In;
    float acc = 0.0f;
    for (int o = 0; o < Out; ++o) acc = fmaf(W[(size_t)i * Out + o], dY[b * Out + o], acc);
    dX[e] = (mask && mask[e] <= 0.0f) ? 0.0f : acc;
}

// ---- softmax, tanh, the two losses per row and their gradients at the logits.  grid = B, block = 64 (lane = action) ------------
__global__ __launch_bounds__(64) void k_loss(float* __restrict__ pol /* logits in, softmax out */, const float* __restrict__ vpre,
                                             float* __restrict__ val, const float* __restrict__ target_p, const int8_t* __restrict__ target_z,
                                             const uint32_t* __restrict__ idx, float* __restrict__ dlogit, float* __restrict__ dvpre,
                                             float* __restrict__ lp, float* __restrict__ lv, int B) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const uint32_t row = idx[b];
    const float logit = pol[(size_t)b * 64 + lane];
    float m = logit;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    const double ex = exp((double)(logit - m));
    const double sum = wave_sum(ex);
    const float p = (float)(ex / sum);
    pol[(size_t)b * 64 + lane] = p;
    const float pi = target_p[(size_t)row * 64 + lane];
    const float pe = p + 1e-7f;
    const double loss = wave_sum(-(double)pi * log((double)pe));
    const double dp = -(double)pi / (double)pe;            // d loss / d p
    const double dot = wave_sum(dp * (double)p);
    dlogit[(size_t)b * 64 + lane] = (float)((double)p * (dp - dot) / (double)B);
    if (lane == 0) {
        const float v = (float)tanh((double)vpre[b]);
        const float z = (float)target_z[row];
        val[b] = v;
        lp[b] = (float)loss;
        lv[b] = (v - z) * (v - z);
        dvpre[b] = (float)(2.0 * (double)(v - z) * (1.0 - (double)v * (double)v) / (double)B);
    }
}

__global__ __launch_bounds__(256) void k_loss_sum(const float* __restrict__ lp, const float* __restrict__ lv, float* __restrict__ out, int B) {
    __shared__ double red[256];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        s0 = s0 + (double)lp[i];
        s1 = s1 + (double)lv[i];
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(s0 / (double)B);
        out[1] = (float)(s1 / (double)B);
    }
}

// Keras SGD(momentum 0.9): m <- 0.9 m - lr g;  w <- w + m
__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ w, float* __restrict__ m, const float* __restrict__ g, size_t n, float lr) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float mv = 0.9f * m[e] - lr * g[e];
    m[e] = mv;
    w[e] = w[e] + mv;
}

#include "raz_train_f16x3.h"

inline size_t up64(size_t floats) { return (floats + 63) & ~(size_t)63; }   // 256-byte granules

}  // namespace

struct raz_train_layer {   // one Conv2D + BatchNormalization pair
    int cin, cout, taps;
    size_t w, b, g, be;   // offsets into the parameters
    size_t st;            // offset of the moving mean into the statistics (variance at + cout)
    float *y, *a, *bmean, *bvar, *binv;
};

struct raz_trainer {
    int F, R, V, max_batch, last_batch;
    size_t np, ns;
    std::vector<raz_train_layer> L;   // 0 stem, 1..2R trunk, 2R+1 policy conv, 2R+2 value conv
    size_t pfc_w, pfc_b, v1_w, v1_b, v2_w, v2_b;
    float *P, *ST, *M, *G;
    float *pol, *h1, *vpre, *val, *dlogit, *dh1, *dvpre, *dph, *dvh, *dyp, *dyv, *lp, *lv;
    float *gb, *db, *eb, *partial;
    int precision;           // RAZ_TRAIN_F32 (v1) or RAZ_TRAIN_F16X3 (v2); the rest: v2 alone
    unsigned char* wimg;     // one split weight image (raz_train_f16x3.h), rebuilt ahead of every product that reads one
    float* sc;               // per pair 8 floats: (S, 1 / S) of its kernel, of its input activations, of its output gradient
    unsigned* amax;          // partial maxima of k_absmax_part
};

namespace {

bool shape_ok(int F, int R, int V, int mb) {
    return F >= 16 && F <= 1024 && F % 16 == 0 && R >= 0 && R <= 64 && V >= 1 && V <= 16192 && mb >= 1 && mb <= 65536;
}

// Lays the trainer out over `base` (nullptr: sizes only).  Returns the number of floats.
size_t layout(raz_trainer* t, float* base) {
    const int F = t->F, R = t->R, V = t->V;
    const size_t mb = (size_t)t->max_batch;
    const int NL = 2 * R + 3;
    t->L.assign(NL, raz_train_layer());
    size_t p = 0, st = 0;
    for (int i = 0; i < NL; ++i) {
        raz_train_layer& l = t->L[i];
        l.cin = i == 0 ? 2 : F;
        l.cout = i == NL - 2 ? 2 : i == NL - 1 ? 1 : F;
        l.taps = i >= NL - 2 ? 1 : 9;
        l.w = p; p += (size_t)l.cout * l.cin * l.taps;
        l.b = p; p += l.cout;
        l.g = p; p += l.cout;
        l.be = p; p += l.cout;
        l.st = st; st += 2 * (size_t)l.cout;
    }
    t->pfc_w = p; p += 128 * 64;
    t->pfc_b = p; p += 64;
    t->v1_w = p; p += (size_t)64 * V;
    t->v1_b = p; p += V;
    t->v2_w = p; p += V;
    t->v2_b = p; p += 1;
    t->np = p;
    t->ns = st;
    size_t o = 0;
    auto take = [&](size_t n) { float* r = base ? base + o : nullptr; o += up64(n); return r; };
    t->P = take(2 * p + st);   // the train blob: parameters | moving statistics | momentum
    t->ST = base ? t->P + p : nullptr;
    t->M = base ? t->ST + st : nullptr;
    t->G = take(p);
    for (int i = 0; i < NL; ++i) {
        raz_train_layer& l = t->L[i];
        l.y = take(mb * l.cout * 64);
        l.a = take(mb * l.cout * 64);
        l.bmean = take(l.cout);
        l.bvar = take(l.cout);
        l.binv = take(l.cout);
    }
    t->pol = take(mb * 64); t->h1 = take(mb * V); t->vpre = take(mb); t->val = take(mb);
    t->dlogit = take(mb * 64); t->dh1 = take(mb * V); t->dvpre = take(mb);
    t->dph = take(mb * 128); t->dvh = take(mb * 64); t->dyp = take(mb * 128); t->dyv = take(mb * 64);
    t->lp = take(mb); t->lv = take(mb);
    t->gb = take(mb * F * 64); t->db = take(mb * F * 64); t->eb = take(mb * F * 64);
    const size_t S = mb < (size_t)MAX_SPLIT ? mb : (size_t)MAX_SPLIT;
    t->partial = take(S * F * F * 9);
    if (t->precision == RAZ_TRAIN_F16X3) {   // appended: precision 0 keeps its layout to the byte
        t->wimg = (unsigned char*)take((size_t)((F + X3_OCT - 1) / X3_OCT) * (F / 16) * (X3_WCHUNK / 4));
        t->sc = take((size_t)NL * 8);
        t->amax = (unsigned*)take(X3_MAX_PARTS);
    }
    return o;
}

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

void bn_fwd(raz_trainer* t, int i, const float* skip, int B, bool update, hipStream_t s) {
    const raz_train_layer& l = t->L[i];
    hipLaunchKernelGGL(k_bn_fwd, dim3(l.cout), dim3(256), 0, s, (const float*)l.y, l.a, skip, (const float*)(t->P + l.g),
                       (const float*)(t->P + l.be), l.bmean, l.bvar, l.binv, update ? t->ST + l.st : (float*)nullptr,
                       update ? t->ST + l.st + l.cout : (float*)nullptr, B, l.cout);
}

void bn_bwd(raz_trainer* t, int i, float* g, float* dy, int keep, int B, hipStream_t s) {
    const raz_train_layer& l = t->L[i];
    hipLaunchKernelGGL(k_bn_bwd, dim3(l.cout), dim3(256), 0, s, g, (const float*)l.a, (const float*)l.y, (const float*)l.bmean,
                       (const float*)l.binv, (const float*)(t->P + l.g), t->G + l.g, t->G + l.be, dy, keep, B, l.cout);
}

// ---- raznet-train-v2: the scale of a tensor, and the three products of trunk pair i ------------------------------------------------
void x3_scale(raz_trainer* t, const float* x, size_t n, float* sc, hipStream_t s) {
    const size_t want = (n + 1023) / 1024;
    const unsigned parts = (unsigned)(want < (size_t)X3_MAX_PARTS ? want : (size_t)X3_MAX_PARTS);
    hipLaunchKernelGGL(k_absmax_part, dim3(parts), dim3(256), 0, s, x, n, t->amax);
    hipLaunchKernelGGL(k_scale_f16x3, dim3(1), dim3(256), 0, s, (const unsigned*)t->amax, (int)parts, sc);
}

// transposed: the input-gradient form.  scin: the scale of `in`.
void x3_conv(raz_trainer* t, int i, bool transposed, const float* in, const float* scin, const float* bias, float* out, const float* add,
             int B, hipStream_t s) {
    const int F = t->F, ntile = (F + X3_OCT - 1) / X3_OCT;
    const float* scw = t->sc + (size_t)i * 8;
    hipLaunchKernelGGL(k_wimage_f16x3, dim3(blocks((size_t)ntile * (F / 16) * 9 * 128)), dim3(256), 0, s, (const float*)(t->P + t->L[i].w), scw,
                       t->wimg, F, transposed ? 1 : 0);
    hipLaunchKernelGGL(k_tconv_f16x3, dim3((unsigned)((B + 3) / 4), (unsigned)ntile), dim3(256), 0, s, (const unsigned char*)t->wimg, scw, scin,
                       bias, in, out, add, B, F, F);
}

void forward(raz_trainer* t, const uint64_t* own, const uint64_t* enemy, const float* policy, const int8_t* z, const uint32_t* idx,
             int B, bool update, float* d_losses, hipStream_t s) {
    const int F = t->F, R = t->R, V = t->V, T = 2 * R, IP = 2 * R + 1, IV = 2 * R + 2;
    float* P = t->P;
    std::vector<raz_train_layer>& L = t->L;
    hipLaunchKernelGGL(k_stem_fwd, dim3(B), dim3(64), 0, s, (const float*)(P + L[0].w), (const float*)(P + L[0].b), (const raz_bb*)own,
                       (const raz_bb*)enemy, idx, L[0].y, F);
    bn_fwd(t, 0, nullptr, B, update, s);
    const dim3 grid((unsigned)((B + 3) / 4), (unsigned)(F / 16));
    for (int i = 1; i <= T; ++i) {
        if (t->precision == RAZ_TRAIN_F16X3) {
            float* sc = t->sc + (size_t)i * 8;
            x3_scale(t, P + L[i].w, (size_t)F * F * 9, sc, s);
            x3_scale(t, L[i - 1].a, (size_t)B * F * 64, sc + 2, s);
            x3_conv(t, i, false, L[i - 1].a, sc + 2, P + L[i].b, L[i].y, nullptr, B, s);
        } else
        hipLaunchKernelGGL(k_tconv<false>, grid, dim3(256), 0, s, (const float*)(P + L[i].w), (const float*)(P + L[i].b),
                           (const float*)L[i - 1].a, L[i].y, (const float*)nullptr, B, F, F);
        bn_fwd(t, i, (i & 1) ? nullptr : L[i - 2].a, B, update, s);
    }
    hipLaunchKernelGGL(k_hconv_fwd, dim3(B), dim3(64), 0, s, (const float*)(P + L[IP].w), (const float*)(P + L[IP].b),
                       (const float*)(P + L[IV].w), (const float*)(P + L[IV].b), (const float*)L[T].a, L[IP].y, L[IV].y, F);
    bn_fwd(t, IP, nullptr, B, update, s);
    bn_fwd(t, IV, nullptr, B, update, s);
    hipLaunchKernelGGL(k_dense_fwd, dim3(blocks((size_t)B * 64)), dim3(256), 0, s, (const float*)L[IP].a, (const float*)(P + t->pfc_w),
                       (const float*)(P + t->pfc_b), t->pol, B, 128, 64, 0);
    hipLaunchKernelGGL(k_dense_fwd, dim3(blocks((size_t)B * V)), dim3(256), 0, s, (const float*)L[IV].a, (const float*)(P + t->v1_w),
                       (const float*)(P + t->v1_b), t->h1, B, 64, V, 1);
    hipLaunchKernelGGL(k_dense_fwd, dim3(blocks((size_t)B)), dim3(256), 0, s, (const float*)t->h1, (const float*)(P + t->v2_w),
                       (const float*)(P + t->v2_b), t->vpre, B, V, 1, 0);
    hipLaunchKernelGGL(k_loss, dim3(B), dim3(64), 0, s, t->pol, (const float*)t->vpre, t->val, policy, z, idx, t->dlogit, t->dvpre, t->lp,
                       t->lv, B);
    hipLaunchKernelGGL(k_loss_sum, dim3(1), dim3(256), 0, s, (const float*)t->lp, (const float*)t->lv, d_losses, B);
}

void conv_wgrad(raz_trainer* t, int i, const float* dy, const float* x, int B, float l2, hipStream_t s) {
    const int F = t->F, S = B < MAX_SPLIT ? B : MAX_SPLIT;
    if (t->precision == RAZ_TRAIN_F16X3) {   // dy's scale first: the input gradient of the same pair reads it too
        float* sc = t->sc + (size_t)i * 8;
        x3_scale(t, dy, (size_t)B * F * 64, sc + 4, s);
        hipLaunchKernelGGL(k_twgrad_f16x3, dim3((unsigned)((F + 63) / 64), (unsigned)((F + 31) / 32), (unsigned)S), dim3(256), 0, s, dy, x,
                           (const float*)(sc + 4), (const float*)(sc + 2), t->partial, B, F, F);
    } else
    hipLaunchKernelGGL(k_twgrad, dim3((unsigned)((F + 63) / 64), (unsigned)(F / 16), (unsigned)S), dim3(256), 0, s, dy, x, t->partial, B, F, F);
    const size_t n = (size_t)F * F * 9;
    hipLaunchKernelGGL(k_twgrad_fold, dim3(blocks(n)), dim3(256), 0, s, (const float*)t->partial, (const float*)(t->P + t->L[i].w),
                       t->G + t->L[i].w, n, S, l2);
}

int backward(raz_trainer* t, const uint64_t* own, const uint64_t* enemy, const uint32_t* idx, int B, float l2, hipStream_t s) {
    const int F = t->F, R = t->R, V = t->V, T = 2 * R, IP = 2 * R + 1, IV = 2 * R + 2;
    float *P = t->P, *G = t->G;
    std::vector<raz_train_layer>& L = t->L;
    RAZ_HIP_TRY(hipMemsetAsync(G, 0, t->np * sizeof(float), s), "raz_trainer: hipMemsetAsync");   // conv biases ahead of BatchNorm: exactly 0
    // policy head
    hipLaunchKernelGGL(k_dense_wgrad, dim3(blocks((size_t)129 * 64)), dim3(256), 0, s, (const float*)L[IP].a, (const float*)t->dlogit,
                       (const float*)(P + t->pfc_w), G + t->pfc_w, G + t->pfc_b, B, 128, 64, l2);
    hipLaunchKernelGGL(k_dense_dgrad, dim3(blocks((size_t)B * 128)), dim3(256), 0, s, (const float*)t->dlogit, (const float*)(P + t->pfc_w),
                       (const float*)nullptr, t->dph, B, 128, 64);
    // value head
    hipLaunchKernelGGL(k_dense_wgrad, dim3(blocks((size_t)V + 1)), dim3(256), 0, s, (const float*)t->h1, (const float*)t->dvpre,
                       (const float*)(P + t->v2_w), G + t->v2_w, G + t->v2_b, B, V, 1, l2);
    hipLaunchKernelGGL(k_dense_dgrad, dim3(blocks((size_t)B * V)), dim3(256), 0, s, (const float*)t->dvpre, (const float*)(P + t->v2_w),
                       (const float*)t->h1, t->dh1, B, V, 1);
    hipLaunchKernelGGL(k_dense_wgrad, dim3(blocks((size_t)65 * V)), dim3(256), 0, s, (const float*)L[IV].a, (const float*)t->dh1,
                       (const float*)(P + t->v1_w), G + t->v1_w, G + t->v1_b, B, 64, V, l2);
    hipLaunchKernelGGL(k_dense_dgrad, dim3(blocks((size_t)B * 64)), dim3(256), 0, s, (const float*)t->dh1, (const float*)(P + t->v1_w),
                       (const float*)nullptr, t->dvh, B, 64, V);
    bn_bwd(t, IP, t->dph, t->dyp, 0, B, s);
    bn_bwd(t, IV, t->dvh, t->dyv, 0, B, s);
    hipLaunchKernelGGL(k_hconv_wgrad, dim3(F), dim3(64), 0, s, (const float*)t->dyp, (const float*)t->dyv, (const float*)L[T].a,
                       (const float*)(P + L[IP].w), (const float*)(P + L[IV].w), G + L[IP].w, G + L[IV].w, B, F, l2);
    const size_t nact = (size_t)B * F * 64;
    hipLaunchKernelGGL(k_hconv_dgrad, dim3(blocks(nact)), dim3(256), 0, s, (const float*)t->dyp, (const float*)t->dyv,
                       (const float*)(P + L[IP].w), (const float*)(P + L[IV].w), t->gb, nact, F);
    const dim3 grid((unsigned)((B + 3) / 4), (unsigned)(F / 16));
    for (int r = R - 1; r >= 0; --r) {
        const int l1 = 1 + 2 * r, l2i = 2 + 2 * r;
        bn_bwd(t, l2i, t->gb, t->db, 1, B, s);   // gb keeps the masked gradient: the skip path's share
        conv_wgrad(t, l2i, t->db, L[l1].a, B, l2, s);
        if (t->precision == RAZ_TRAIN_F16X3) x3_conv(t, l2i, true, t->db, t->sc + (size_t)l2i * 8 + 4, nullptr, t->eb, nullptr, B, s);
        else
        hipLaunchKernelGGL(k_tconv<true>, grid, dim3(256), 0, s, (const float*)(P + L[l2i].w), (const float*)nullptr, (const float*)t->db,
                           t->eb, (const float*)nullptr, B, F, F);
        bn_bwd(t, l1, t->eb, t->db, 0, B, s);
        conv_wgrad(t, l1, t->db, L[l1 - 1].a, B, l2, s);
        if (t->precision == RAZ_TRAIN_F16X3) x3_conv(t, l1, true, t->db, t->sc + (size_t)l1 * 8 + 4, nullptr, t->gb, t->gb, B, s);
        else
        hipLaunchKernelGGL(k_tconv<true>, grid, dim3(256), 0, s, (const float*)(P + L[l1].w), (const float*)nullptr, (const float*)t->db,
                           t->gb, (const float*)t->gb, B, F, F);
    }
    bn_bwd(t, 0, t->gb, t->db, 0, B, s);
    hipLaunchKernelGGL(k_stem_wgrad, dim3(F), dim3(64), 0, s, (const float*)t->db, (const raz_bb*)own, (const raz_bb*)enemy, idx,
                       (const float*)(P + L[0].w), G + L[0].w, B, F, l2);
    return RAZ_OK;
}

int check_batch(raz_trainer* t, const void* own, const void* enemy, const void* policy, const void* z, const void* idx, size_t B,
                const void* losses) {
    if (!t) return raz_fail(RAZ_EINVAL, "raz_trainer: NULL trainer");
    if (!own || !enemy || !policy || !z || !idx || !losses) return raz_fail(RAZ_EINVAL, "raz_trainer: NULL array");
    if (((uintptr_t)own | (uintptr_t)enemy) & 7 || ((uintptr_t)policy | (uintptr_t)idx | (uintptr_t)losses) & 3)
        return raz_fail(RAZ_EINVAL, "raz_trainer: misaligned array");
    if (B == 0 || B > (size_t)t->max_batch) return raz_fail(RAZ_EINVAL, "raz_trainer: batch must be 1..max_batch");
    return RAZ_OK;
}

}  // namespace

extern "C" {

size_t raz_trainer_bytes2(int filters, int res_layers, int value_fc, size_t max_batch, int precision) {
    if (precision != RAZ_TRAIN_F32 && precision != RAZ_TRAIN_F16X3) {
        raz_fail(RAZ_EINVAL, "raz_trainer_bytes2: precision is RAZ_TRAIN_F32 (0) or RAZ_TRAIN_F16X3 (1)");
        return 0;
    }
    if (max_batch > 65536 || !shape_ok(filters, res_layers, value_fc, (int)max_batch)) return 0;
    raz_trainer t;
    t.F = filters; t.R = res_layers; t.V = value_fc; t.max_batch = (int)max_batch; t.precision = precision;
    return layout(&t, nullptr) * sizeof(float);
}

size_t raz_trainer_bytes(int filters, int res_layers, int value_fc, size_t max_batch) {
    return raz_trainer_bytes2(filters, res_layers, value_fc, max_batch, RAZ_TRAIN_F32);
}

size_t raz_trainer_state_bytes(int filters, int res_layers, int value_fc) {
    if (!shape_ok(filters, res_layers, value_fc, 1)) return 0;
    raz_trainer t;
    t.F = filters; t.R = res_layers; t.V = value_fc; t.max_batch = 1; t.precision = RAZ_TRAIN_F32;
    layout(&t, nullptr);
    return (2 * t.np + t.ns) * sizeof(float);
}

// Both create entries.  `who`: the entry called, `spec` / `sizer`: the specification and the size entry its messages name.
static int trainer_create(const char* who, const char* spec, const char* sizer, int filters, int res_layers, int value_fc, size_t max_batch,
                          int precision, void* d_workspace, size_t workspace_bytes, raz_trainer** out, raz_stream_t stream) {
    char msg[256];
    auto fail = [&](int code, const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return raz_fail(code, msg);
    };
    if (!out) return fail(RAZ_EINVAL, "NULL out");
    *out = nullptr;
    if (precision != RAZ_TRAIN_F32 && precision != RAZ_TRAIN_F16X3)
        return fail(RAZ_EINVAL, "precision is RAZ_TRAIN_F32 (0) or RAZ_TRAIN_F16X3 (1)");
    if (max_batch > 65536 || !shape_ok(filters, res_layers, value_fc, (int)max_batch)) {
        snprintf(msg, sizeof msg, "%s: %s takes filters %% 16 == 0 (16..1024), cnn_filter_size 3, value_fc 1..16192, max_batch 1..65536", who, spec);
        return raz_fail(RAZ_EINVAL, msg);
    }
    const size_t need = raz_trainer_bytes2(filters, res_layers, value_fc, max_batch, precision);
    if (!d_workspace || ((uintptr_t)d_workspace & 255)) return fail(RAZ_EINVAL, "workspace NULL or not 256-byte aligned");
    if (workspace_bytes < need) {
        snprintf(msg, sizeof msg, "%s: workspace too small (%s)", who, sizer);
        return raz_fail(RAZ_EINVAL, msg);
    }
    raz_trainer* t = new (std::nothrow) raz_trainer;
    if (!t) return fail(RAZ_ENOMEM, "no host memory");
    t->F = filters; t->R = res_layers; t->V = value_fc; t->max_batch = (int)max_batch; t->last_batch = 0;
    t->precision = precision; t->wimg = nullptr; t->sc = nullptr; t->amax = nullptr;
    layout(t, (float*)d_workspace);
    hipError_t e = hipMemsetAsync(d_workspace, 0, need, (hipStream_t)stream);
    if (e != hipSuccess) {
        delete t;
        snprintf(msg, sizeof msg, "%s: hipMemsetAsync", who);
        return raz_fail_hip(e, msg);
    }
    *out = t;
    return RAZ_OK;
}

int raz_trainer_create2(int filters, int res_layers, int value_fc, size_t max_batch, int precision, void* d_workspace,
                        size_t workspace_bytes, raz_trainer** out, raz_stream_t stream) {
    return trainer_create("raz_trainer_create2", precision == RAZ_TRAIN_F16X3 ? "raznet-train-v2 (precision RAZ_TRAIN_F16X3)" : "raznet-train-v1",
                          "raz_trainer_bytes2 at this precision", filters, res_layers, value_fc, max_batch, precision, d_workspace,
                          workspace_bytes, out, stream);
}

int raz_trainer_create(int filters, int res_layers, int value_fc, size_t max_batch, void* d_workspace, size_t workspace_bytes,
                       raz_trainer** out, raz_stream_t stream) {
    return trainer_create("raz_trainer_create", "raznet-train-v1", "raz_trainer_bytes", filters, res_layers, value_fc, max_batch, RAZ_TRAIN_F32,
                          d_workspace, workspace_bytes, out, stream);
}

int raz_trainer_precision(const raz_trainer* t) { return t ? t->precision : RAZ_EINVAL; }

void raz_trainer_destroy(raz_trainer* t) { delete t; }

int raz_trainer_set_state(raz_trainer* t, const float* d_blob, size_t bytes, raz_stream_t stream) {
    if (!t || !d_blob || ((uintptr_t)d_blob & 3)) return raz_fail(RAZ_EINVAL, "raz_trainer_set_state: NULL or misaligned argument");
    if (bytes != (2 * t->np + t->ns) * sizeof(float)) return raz_fail(RAZ_EINVAL, "raz_trainer_set_state: size is not raz_trainer_state_bytes");
    RAZ_HIP_TRY(hipMemcpyAsync(t->P, d_blob, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "raz_trainer_set_state");
    return RAZ_OK;
}

int raz_trainer_get_state(raz_trainer* t, float* d_blob, size_t bytes, raz_stream_t stream) {
    if (!t || !d_blob || ((uintptr_t)d_blob & 3)) return raz_fail(RAZ_EINVAL, "raz_trainer_get_state: NULL or misaligned argument");
    if (bytes != (2 * t->np + t->ns) * sizeof(float)) return raz_fail(RAZ_EINVAL, "raz_trainer_get_state: size is not raz_trainer_state_bytes");
    RAZ_HIP_TRY(hipMemcpyAsync(d_blob, t->P, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "raz_trainer_get_state");
    return RAZ_OK;
}

int raz_trainer_backward(raz_trainer* t, const uint64_t* d_own, const uint64_t* d_enemy, const float* d_policy, const int8_t* d_z,
                         const uint32_t* d_idx, size_t batch, float l2, float* d_losses, raz_stream_t stream) {
    const int rc = check_batch(t, d_own, d_enemy, d_policy, d_z, d_idx, batch, d_losses);
    if (rc != RAZ_OK) return rc;
    forward(t, d_own, d_enemy, d_policy, d_z, d_idx, (int)batch, false, d_losses, (hipStream_t)stream);
    const int rb = backward(t, d_own, d_enemy, d_idx, (int)batch, l2, (hipStream_t)stream);
    if (rb != RAZ_OK) return rb;
    t->last_batch = (int)batch;
    return raz_check_launch("raz_trainer_backward");
}

int raz_trainer_step(raz_trainer* t, const uint64_t* d_own, const uint64_t* d_enemy, const float* d_policy, const int8_t* d_z,
                     const uint32_t* d_idx, size_t batch, float lr, float l2, float* d_losses, raz_stream_t stream) {
    const int rc = check_batch(t, d_own, d_enemy, d_policy, d_z, d_idx, batch, d_losses);
    if (rc != RAZ_OK) return rc;
    forward(t, d_own, d_enemy, d_policy, d_z, d_idx, (int)batch, true, d_losses, (hipStream_t)stream);
    const int rb = backward(t, d_own, d_enemy, d_idx, (int)batch, l2, (hipStream_t)stream);
    if (rb != RAZ_OK) return rb;
    hipLaunchKernelGGL(k_sgd, dim3(blocks(t->np)), dim3(256), 0, (hipStream_t)stream, t->P, t->M, (const float*)t->G, t->np, lr);
    t->last_batch = (int)batch;
    return raz_check_launch("raz_trainer_step");
}

int raz_trainer_read(raz_trainer* t, int which, int layer_index, void* d_out, size_t bytes, raz_stream_t stream) {
    if (!t || !d_out) return raz_fail(RAZ_EINVAL, "raz_trainer_read: NULL argument");
    const size_t B = (size_t)t->last_batch;
    const float* src = nullptr;
    size_t n = 0;
    const bool lok = layer_index >= 0 && layer_index < (int)t->L.size();
    switch (which) {
        case RAZ_TRAIN_READ_GRADS: src = t->G; n = t->np; break;
        case RAZ_TRAIN_READ_ACT: if (lok) { src = t->L[layer_index].a; n = B * t->L[layer_index].cout * 64; } break;
        case RAZ_TRAIN_READ_MEAN: if (lok) { src = t->L[layer_index].bmean; n = t->L[layer_index].cout; } break;
        case RAZ_TRAIN_READ_VAR: if (lok) { src = t->L[layer_index].bvar; n = t->L[layer_index].cout; } break;
        case RAZ_TRAIN_READ_HIDDEN: src = t->h1; n = B * t->V; break;
        case RAZ_TRAIN_READ_POLICY: src = t->pol; n = B * 64; break;
        case RAZ_TRAIN_READ_VALUE: src = t->val; n = B; break;
        default: break;
    }
    if (!src) return raz_fail(RAZ_EINVAL, "raz_trainer_read: unknown selector or layer");
    if (which != RAZ_TRAIN_READ_GRADS && which != RAZ_TRAIN_READ_MEAN && which != RAZ_TRAIN_READ_VAR && B == 0)
        return raz_fail(RAZ_ESTATE, "raz_trainer_read: no step has run");
    if (bytes != n * sizeof(float)) return raz_fail(RAZ_EINVAL, "raz_trainer_read: size does not match the tensor");
    RAZ_HIP_TRY(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "raz_trainer_read");
    return RAZ_OK;
}

}  // extern "C"
