// raz_spec_probe.hip — diagnostics: raz-math-v1, raz-rng-v1 (raz_detmath.h) and the wave-level reductions of the tree kernels
// (raz_engine_core.h) applied to caller-supplied device buffers (include/raz.h raz_spec_probe).  Nothing is re-implemented here:
// the kernels below call the functions the tree kernels call, so what a test sees is what a game computes.
#include "raz_engine_core.h"
#include "raz_detmath.h"

namespace {

constexpr int kElemBlock = 256;

// one thread per element, grid-stride
__global__ __launch_bounds__(kElemBlock) void k_probe_elem(int what, const void* __restrict__ in0, const void* __restrict__ in1,
                                                           void* __restrict__ out, size_t n) {
    const uint32_t* u0 = (const uint32_t*)in0;
    const uint32_t* u1 = (const uint32_t*)in1;
    const double* d0 = (const double*)in0;
    const double* d1 = (const double*)in1;
    const float* f0 = (const float*)in0;
    double* od = (double*)out;
    float* of = (float*)out;
    uint32_t* ou = (uint32_t*)out;
    const size_t stride = (size_t)gridDim.x * kElemBlock;
    for (size_t i = (size_t)blockIdx.x * kElemBlock + threadIdx.x; i < n; i += stride) {
        switch (what) {
            case RAZ_PROBE_PHILOX: {
                const uint32_t* p = u0 + 6 * i;
                const raz_u32x4 r = raz_philox4x32_10(p[0], p[1], p[2], p[3], p[4], p[5]);
                ou[4 * i + 0] = r.x;
                ou[4 * i + 1] = r.y;
                ou[4 * i + 2] = r.z;
                ou[4 * i + 3] = r.w;
                break;
            }
            case RAZ_PROBE_RNG_PAIR: {
                const uint32_t* p = u0 + 6 * i;
                double a, b;
                raz_rng_pair(p[0], p[1], p[2], p[3], p[4], p[5], a, b);
                od[2 * i] = a;
                od[2 * i + 1] = b;
                break;
            }
            case RAZ_PROBE_LOG: od[i] = raz_det_log(d0[i]); break;
            case RAZ_PROBE_EXP: od[i] = raz_det_exp(d0[i]); break;
            case RAZ_PROBE_COS2: od[i] = raz_det_cos2(d0[i]); break;
            case RAZ_PROBE_POW: od[i] = raz_det_pow(d0[i], d1[i]); break;
            case RAZ_PROBE_EXPF: of[i] = raz_det_expf(f0[i]); break;
            case RAZ_PROBE_TANHF: of[i] = raz_det_tanhf(f0[i]); break;
            case RAZ_PROBE_GAMMA_HALF_PAIR: {
                const uint32_t* p = u0 + 4 * i;
                double a, b;
                raz_gamma_half_pair(p[0], p[1], p[2], p[3], a, b);
                od[2 * i] = a;
                od[2 * i + 1] = b;
                break;
            }
            case RAZ_PROBE_GAMMA_ATTEMPT: {
                const uint32_t* p = u1 + 5 * i;
                double X = 0.0;
                const bool ok = raz_gamma_attempt(d0[i], p[0], p[1], p[2], p[3], p[4], X);
                od[2 * i] = X;
                od[2 * i + 1] = ok ? 1.0 : 0.0;
                break;
            }
            default: break;
        }
    }
}

// one 64-lane workgroup per row, lane = column
__global__ __launch_bounds__(64) void k_probe_wave(int what, const void* __restrict__ in0, const void* __restrict__ in1,
                                                   void* __restrict__ out, size_t n) {
    __shared__ float lds64[64];
    const int lane = (int)threadIdx.x;
    const size_t row = blockIdx.x;
    if (row >= n) return;
    switch (what) {
        case RAZ_PROBE_NP_SUM_F32: {
            const float s = wave_np_sum_f32(((const float*)in0)[row * 64 + lane], lane, lds64);
            if (lane == 0) ((float*)out)[row] = s;
            break;
        }
        case RAZ_PROBE_ARGMAX_F64: {
            const int a = wave_argmax_f64(((const double*)in0)[row * 64 + lane], lane);
            if (lane == 0) ((int*)out)[row] = a;
            break;
        }
        case RAZ_PROBE_ARGMAX_NONNEG_F64: {
            const int a = wave_argmax_nonneg_f64(((const double*)in0)[row * 64 + lane]);
            if (lane == 0) ((int*)out)[row] = a;
            break;
        }
        case RAZ_PROBE_MAX_F64: {
            const double m = wave_max_f64(((const double*)in0)[row * 64 + lane]);
            if (lane == 0) ((double*)out)[row] = m;
            break;
        }
        case RAZ_PROBE_SUM_U32: {
            const uint32_t s = wave_sum_u32(((const uint32_t*)in0)[row * 64 + lane]);
            if (lane == 0) ((uint32_t*)out)[row] = s;
            break;
        }
        case RAZ_PROBE_ROOT_GAMMAS: {
            const double alpha = ((const double*)in0)[row];
            const uint32_t* p = (const uint32_t*)in1 + 4 * row;
            const uint32_t k = p[0];
            double gam = 0.0, noise = 0.0;
            uint32_t rounds = 0;
            // (the sampler has no exit for a shape that is not a positive number, and no lanes for k > 64: such rows read zeros)
            if (k >= 1u && k <= 64u && alpha > 0.0 && alpha < 0x1p+1023) root_noise<true>(alpha, p[1], p[2], p[3], (int)k, lane, gam, noise, rounds);
            double* g = (double*)out;
            g[row * 64 + lane] = gam;
            g[(n + row) * 64 + lane] = noise;
            if (lane == 0) ((uint32_t*)(g + 2 * n * 64))[row] = rounds;
            break;
        }
        case RAZ_PROBE_CHOICE: {
            const int a = choice_of(((const double*)in0)[row * 64 + lane], [&]() { return ((const double*)in1)[row]; }, lane);
            if (lane == 0) ((int*)out)[row] = a;
            break;
        }
        default: break;
    }
}

}  // namespace

extern "C" int raz_spec_probe(int what, const void* in0, const void* in1, void* out, size_t n, raz_stream_t stream) {
    if (what < RAZ_PROBE_PHILOX || what > RAZ_PROBE_CHOICE) return raz_fail(RAZ_EINVAL, "raz_spec_probe: unknown selector");
    if (n == 0) return RAZ_OK;
    const bool two = what == RAZ_PROBE_POW || what == RAZ_PROBE_GAMMA_ATTEMPT || what == RAZ_PROBE_ROOT_GAMMAS || what == RAZ_PROBE_CHOICE;
    if (!in0 || !out || (two && !in1)) return raz_fail(RAZ_EINVAL, "raz_spec_probe: NULL buffer");
    if (what >= RAZ_PROBE_NP_SUM_F32) {
        if (n >= ((size_t)1 << 24)) return raz_fail(RAZ_EINVAL, "raz_spec_probe: too many rows");
        hipLaunchKernelGGL(k_probe_wave, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, what, in0, in1, out, n);
    } else {
        size_t blocks = (n + kElemBlock - 1) / kElemBlock;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_probe_elem, dim3((unsigned)blocks), dim3(kElemBlock), 0, (hipStream_t)stream, what, in0, in1, out, n);
    }
    return raz_check_launch("raz_spec_probe");
}
