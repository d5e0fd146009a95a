// raz_net_heads.h — the policy and value heads of raznet-forward-v1 for ONE position on ONE wave (lane = board square), stated once
// for the kernels that differ only in where the trunk's output lives: k_net_wave (raz_net.hip), k_heads_wide (raz_net_wide.hip)
// and k_heads_split (raz_net_f16x3.hip).  A kernel walks the trunk's channels in ascending order, hands every value of its lane's
// square to heads_1x1_step, and gives the three sums to heads_finish.  `head` is heads_lds_floats(V) floats of LDS owned by the
// wave (the caller declares it).  The tuned form of the same chains (k_net_mfma, k_tree_net) is net_heads_tuned in raz_net_wave.h.
#pragma once
#include <hip/hip_runtime.h>
#include "raz_detmath.h"
#include "raz_net_layout.h"

namespace {

// the three 1x1 convolutions (two policy planes, one value plane) at input channel ic
__device__ __forceinline__ void heads_1x1_step(const HeadWeights& h, int F, int ic, float xv, float& p0, float& p1, float& v0) {
    p0 = fmaf(xv, h.pol_w[ic], p0);
    p1 = fmaf(xv, h.pol_w[F + ic], p1);
    v0 = fmaf(xv, h.val_w[ic], v0);
}

// relu of the 1x1 sums into the head scratch, for the dense layers to read
__device__ __forceinline__ void heads_relu_1x1(float* head, int lane, float p0, float p1, float v0) {
    head[lane] = p0 > 0.0f ? p0 : 0.0f;
    head[64 + lane] = p1 > 0.0f ? p1 : 0.0f;
    head[HEAD_VH + lane] = v0 > 0.0f ? v0 : 0.0f;
}

// Everything after the 1x1 convolutions: policy dense 128 -> 64 (lane = output square), softmax (max, det_expf, xor-butterfly sum,
// divide) into policy_row[lane]; value dense 64 -> V with relu (lane = hidden unit, looping when V > 64), the output chain and
// det_tanhf into *value_out.
__device__ __forceinline__ void heads_finish(const HeadWeights& h, int V, float p0, float p1, float v0, float* head, int lane,
                                             float* __restrict__ policy_row, float* __restrict__ value_out) {
    const float* ph = head;
    const float* vh = head + HEAD_VH;
    float* h1 = head + HEAD_H1;
    heads_relu_1x1(head, lane, p0, p1, v0);
    __syncthreads();
    float logit = h.pfc_b[lane];
#pragma unroll 16
    for (int j = 0; j < 128; ++j) logit = fmaf(ph[j], h.pfc_w[j * 64 + lane], logit);
    float m = logit;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) m = fmaxf(m, __shfl_xor(m, s));
    const float e = raz_det_expf(logit - m);
    float sum = e;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) sum = sum + __shfl_xor(sum, s);
    policy_row[lane] = e / sum;
    for (int o0 = 0; o0 < V; o0 += 64) {
        const int o = o0 + lane;
        if (o < V) {
            float acc = h.v1_b[o];
#pragma unroll 8
            for (int j = 0; j < 64; ++j) acc = fmaf(vh[j], h.v1_w[j * V + o], acc);
            h1[o] = acc > 0.0f ? acc : 0.0f;
        }
    }
    __syncthreads();
    float acc = h.v2_b[0];
    for (int j = 0; j < V; ++j) acc = fmaf(h1[j], h.v2_w[j], acc);
    if (lane == 0) *value_out = raz_det_tanhf(acc);
}

}  // namespace
