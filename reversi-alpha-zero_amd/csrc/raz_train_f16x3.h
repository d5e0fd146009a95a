// raz_train_f16x3.h — raznet-train-v2: the three 3x3 products of every trunk layer on the f16 matrix cores
// with split operands.  Included by raz_train.hip inside its unnamed namespace; everything else of the step is raznet-train-v1's.
//
// Every f32 operand x of a product is carried as (hi, lo) = (f16(x S), f16(x S - hi)) - 22 significant bits - and a product is
// evaluated as  lo_a hi_b + hi_a lo_b + hi_a hi_b  by three v_mfma_f32_32x32x16_f16 into ONE f32 accumulator, which is multiplied
// once by the exact 1 / (S_a S_b).  S is a power of two PER TENSOR (a layer's kernel, a layer's input activations, a layer's output
// gradient) with max |x| S in [2^14, 2^15), S = 1 for an all-zero tensor: k_absmax_part / k_scale_f16x3, an integer maximum of the
// absolute values' bits in a fixed tree - no floating-point atomics, and a maximum does not depend on the order anyway.
//   k_wimage_f16x3   a layer's kernel -> the split weight image of one product, in the order the LDS image wants it: forward
//                    W[oc][ic][t], input gradient (mirrored, transposed) W[ic][oc][8 - t]; rebuilt ahead of every product that reads one
//                    (once per step, layer and direction), into one shared buffer
//   k_tconv_f16x3    forward and input gradient: out[b][oc][sq] = (bias[oc]) + sum_{ic,t} Wimg[oc][ic][t] in[b][ic][sq + off(t)] (+ add)
//                    workgroup = 4 positions x 64 output channels, wave = 1 position x 2 x 2 tiles of 32 x 32; the loader reads f32
//                    activations, splits them and writes channel-innermost 16-byte slots; taps are per-lane LDS addresses, off-board
//                    taps read a zero row (no predicates), as in raz_net_f16x3.hip
//   k_twgrad_f16x3   weight gradient, partial sums per split of positions (v1's split and v1's k_twgrad_fold): k = the 64 squares of a
//                    position, 8 consecutive k = one board row = one 16-byte operand; the x plane is staged as three column-shifted
//                    copies (dx = -1, 0, +1) between zero halo rows, so that every tap is an aligned ds_read_b128
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int X3_OCT = 64;                             // output channels per workgroup of k_tconv_f16x3
constexpr int X3_WCHUNK = 9 * 2 * 2 * 2 * 32 * 16;     // 36,864 B: [tap 9][m tile 2][hi/lo][k-group 2][oc 32][16 B] per (oc tile, 16-channel chunk)
constexpr int X3_ACT_POS = 4096;                       // [k-group 2][hi/lo][square 64][16 B]
constexpr int X3_ZOFF = 4 * X3_ACT_POS;                // two zero rows of 256 B, 1,024 B apart (hi and lo reads of an off-board tap)
constexpr int X3_ACT_IMG = X3_ZOFF + 1280;
// k_twgrad_f16x3's LDS rows are an ODD number of 16-byte slots: the 16 lanes that share an LDS cycle of a ds_read_b128 read
// consecutive channels at one board row, and then fall into 16 different groups of 4 banks
constexpr int X3_DYROW = 144;                          // bytes per (hi/lo, out channel) of the dy tile: 64 halfs + one slot
constexpr int X3_XROW = 176;                           // ... per (copy, hi/lo, in channel) of the x planes: 10 rows (two halo rows) + one slot
constexpr int X3_MAX_PARTS = 1024;

__device__ __forceinline__ void split_f16x3(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// max |x| as the integer maximum of the bit patterns with the sign cleared.  grid = parts, block = 256.
__global__ __launch_bounds__(256) void k_absmax_part(const float* __restrict__ x, size_t n, unsigned* __restrict__ part) {
    __shared__ unsigned red[256];
    const int tid = threadIdx.x;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned u = __float_as_uint(x[i]) & 0x7fffffffu;
        m = u > m ? u : m;
    }
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// sc[0] = S = 2^k with max * S in [2^14, 2^15) (k held to +-100; 1 for a tensor of zeros), sc[1] = 1 / S.  grid = 1, block = 256.
__global__ __launch_bounds__(256) void k_scale_f16x3(const unsigned* __restrict__ part, int parts, float* __restrict__ sc) {
    __shared__ unsigned red[256];
    const int tid = threadIdx.x;
    unsigned m = 0u;
    for (int i = tid; i < parts; i += 256) m = part[i] > m ? part[i] : m;
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    if (tid == 0) {
        const float mx = __uint_as_float(red[0]);
        int k = 0;
        if (mx > 0.0f) {
            int e = 0;
            frexpf(mx, &e);   // mx = f 2^e, f in [0.5, 1)
            k = 15 - e;
            k = k > 100 ? 100 : k < -100 ? -100 : k;
        }
        sc[0] = ldexpf(1.0f, k);
        sc[1] = ldexpf(1.0f, -k);
    }
}

// One thread per 16-byte slot pair (hi, lo) of the image: 8 consecutive reduction channels of one output channel and tap.
// T: the input-gradient image (output channel = the kernel's input channel, taps mirrored).  Output channels beyond F are zeros.
__global__ __launch_bounds__(256) void k_wimage_f16x3(const float* __restrict__ W, const float* __restrict__ sc, unsigned char* __restrict__ img,
                                                      int F, int T) {
    const int nch = F / 16, ntile = (F + X3_OCT - 1) / X3_OCT;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)ntile * nch * 9 * 128) return;
    const int o32 = (int)(e & 31), kg = (int)(e >> 5) & 1, m = (int)(e >> 6) & 1;
    const size_t r = e >> 7;
    const int t = (int)(r % 9), c = (int)((r / 9) % (size_t)nch), ot = (int)(r / 9 / (size_t)nch);
    const int oc = ot * X3_OCT + m * 32 + o32;
    const float S = sc[0];
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ic = c * 16 + kg * 8 + j;
        float w = 0.0f;
        if (oc < F) w = T ? W[((size_t)ic * F + oc) * 9 + (8 - t)] : W[((size_t)oc * F + ic) * 9 + t];
        _Float16 h, l;
        split_f16x3(w * S, h, l);
        hi[j] = h;
        lo[j] = l;
    }
    unsigned char* dst = img + ((size_t)ot * nch + c) * X3_WCHUNK + (size_t)((t * 2 + m) * 4 + kg) * 512 + o32 * 16;
    *(h8*)dst = hi;
    *(h8*)(dst + 1024) = lo;
}

// in [B][Cin][64] f32 -> out [B][Cout][64] f32 = acc / (S_w S_in) (+ bias) (+ add).  grid = (ceil(B / 4), ceil(Cout / 64)), block = 256.
__global__ __launch_bounds__(256) void k_tconv_f16x3(const unsigned char* __restrict__ Wimg, const float* __restrict__ scw,
                                                     const float* __restrict__ scin, const float* __restrict__ bias,
                                                     const float* __restrict__ in, float* out, const float* add, int B, int Cin, int Cout) {
    __shared__ __attribute__((aligned(16))) unsigned char wS[X3_WCHUNK];
    __shared__ __attribute__((aligned(16))) unsigned char aS[X3_ACT_IMG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kg = lane >> 5;
    const int p0 = blockIdx.x * 4, ot = blockIdx.y, oc0 = ot * X3_OCT, pos = p0 + wv;
    const int nch = Cin / 16;
    const int mt = Cout - oc0 > 32 ? 2 : 1;   // live 32-row tiles of this workgroup
    if (tid < 32) ((f32x4*)(aS + X3_ZOFF + (tid >> 4) * 1024))[tid & 15] = (f32x4){0.f, 0.f, 0.f, 0.f};
    uint32_t boff[2][9];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int sq = nt * 32 + (lane & 31), y = sq >> 3, x = sq & 7;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            const bool ok = yy >= 0 && yy < 8 && xx >= 0 && xx < 8;
            const int s2 = sq + (t / 3 - 1) * 8 + (t % 3 - 1);
            boff[nt][t] = ok ? (uint32_t)(wv * X3_ACT_POS + kg * 2048 + s2 * 16) : (uint32_t)(X3_ZOFF + (s2 & 15) * 16);
        }
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][nt][r] = 0.f;
    const float S = scin[0];
    for (int c = 0; c < nch; ++c) {
        __syncthreads();
        {
            const f32x4* src = (const f32x4*)(Wimg + ((size_t)ot * nch + c) * X3_WCHUNK);
#pragma unroll
            for (int i = 0; i < X3_WCHUNK / 16 / 256; ++i) ((f32x4*)wS)[tid + 256 * i] = src[tid + 256 * i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = tid + 256 * i;
            const int pp = q >> 7, g = (q >> 6) & 1, sq = q & 63;
            h8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) hi[j] = lo[j] = (_Float16)0.0f;
            if (p0 + pp < B) {
                const float* s = in + ((size_t)(p0 + pp) * Cin + c * 16 + g * 8) * 64 + sq;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    _Float16 h, l;
                    split_f16x3(s[j * 64] * S, h, l);
                    hi[j] = h;
                    lo[j] = l;
                }
            }
            unsigned char* d = aS + pp * X3_ACT_POS + g * 2048 + sq * 16;
            *(h8*)d = hi;
            *(h8*)(d + 1024) = lo;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            h8 bh[2], bl[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                bh[nt] = *(const h8*)(aS + boff[nt][t]);
                bl[nt] = *(const h8*)(aS + boff[nt][t] + 1024);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (m < mt) {
                    const h8 ah = *(const h8*)(wS + (t * 2 + m) * 2048 + lane * 16);
                    const h8 al = *(const h8*)(wS + (t * 2 + m) * 2048 + 1024 + lane * 16);
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[nt], acc[m][nt], 0, 0, 0);
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[nt], acc[m][nt], 0, 0, 0);
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[nt], acc[m][nt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (pos >= B) return;
    const float iw = scw[1], ix = scin[1];
    // D: column = lane & 31 = square inside tile nt, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) = channel inside the 32-row tile
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int oc = oc0 + m * 32 + 8 * (v >> 2) + 4 * kg + (v & 3);
                if (oc < Cout) {
                    const size_t o = ((size_t)pos * Cout + oc) * 64 + nt * 32 + (lane & 31);
                    float r = acc[m][nt][v] * iw * ix;
                    if (bias) r = r + bias[oc];
                    if (add) r = r + add[o];
                    out[o] = r;
                }
            }
}

// Weight gradient, partial sums: partial[s][oc][ic][t] = sum over the positions s, s + S, ... and their 64 squares of
// dy[b][oc][sq] x[b][ic][sq + off(t)], un-scaled by 1 / (S_dy S_x).  grid = (ceil(Cout / 64), ceil(Cin / 32), S), block = 256:
// wave = one 32 x 32 tile (out x in channels) of taps 0-4 (waves 0, 1) or 5-8 (waves 2, 3).
__global__ __launch_bounds__(256) void k_twgrad_f16x3(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ scdy,
                                                      const float* __restrict__ scx, float* __restrict__ partial, int B, int Cin, int Cout) {
    __shared__ __attribute__((aligned(16))) unsigned char dS[2 * 64 * X3_DYROW];      // [hi/lo][oc 64][row 8][8 halfs] (+ 16 B)
    __shared__ __attribute__((aligned(16))) unsigned char xS[3 * 2 * 32 * X3_XROW];   // [dx 3][hi/lo][ic 32][halo row, 8 rows, halo row][8 halfs]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kg = lane >> 5;
    const int ocg = blockIdx.x * 64, ic0 = blockIdx.y * 32, s = blockIdx.z, S = gridDim.z;
    const int mtile = wv & 1, tg = wv >> 1;
    const bool work = ocg + mtile * 32 < Cout;
    for (int j = tid; j < 3 * 2 * 32 * X3_XROW / 16; j += 256) ((f32x4*)xS)[j] = (f32x4){0.f, 0.f, 0.f, 0.f};   // the halo rows stay zero
    f32x16 acc[5];
#pragma unroll
    for (int tt = 0; tt < 5; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
    const float Sd = scdy[0], Sx = scx[0];
    for (int b = s; b < B; b += S) {
        __syncthreads();
        {   // x: thread = (in channel, board row); the row goes to the three copies shifted by dx = -1, 0, +1
            const int ic = tid >> 3, r = tid & 7;
            f32x4 v0 = (f32x4){0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (ic0 + ic < Cin) {
                const float* src = x + ((size_t)b * Cin + ic0 + ic) * 64 + r * 8;
                v0 = *(const f32x4*)src;
                v1 = *(const f32x4*)(src + 4);
            }
            _Float16 h[10], l[10];   // columns -1 .. 8
            h[0] = h[9] = l[0] = l[9] = (_Float16)0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) split_f16x3((j < 4 ? v0[j & 3] : v1[j & 3]) * Sx, h[j + 1], l[j + 1]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                h8 hi, lo;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    hi[j] = h[j + d];
                    lo[j] = l[j + d];
                }
                *(h8*)(xS + ((d * 2 + 0) * 32 + ic) * X3_XROW + (r + 1) * 16) = hi;
                *(h8*)(xS + ((d * 2 + 1) * 32 + ic) * X3_XROW + (r + 1) * 16) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {   // dy: 64 out channels x 8 board rows
            const int q = tid + 256 * i;
            const int oc = q >> 3, r = q & 7;
            f32x4 v0 = (f32x4){0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (ocg + oc < Cout) {
                const float* src = dy + ((size_t)b * Cout + ocg + oc) * 64 + r * 8;
                v0 = *(const f32x4*)src;
                v1 = *(const f32x4*)(src + 4);
            }
            h8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                _Float16 hh, ll;
                split_f16x3((j < 4 ? v0[j & 3] : v1[j & 3]) * Sd, hh, ll);
                hi[j] = hh;
                lo[j] = ll;
            }
            *(h8*)(dS + oc * X3_DYROW + r * 16) = hi;
            *(h8*)(dS + (64 + oc) * X3_DYROW + r * 16) = lo;
        }
        __syncthreads();
        if (work) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {   // 16 squares = board rows 2 ks (lanes 0-31) and 2 ks + 1 (lanes 32-63)
                const int row = 2 * ks + kg;
                const h8 ah = *(const h8*)(dS + (mtile * 32 + (lane & 31)) * X3_DYROW + row * 16);
                const h8 al = *(const h8*)(dS + (64 + mtile * 32 + (lane & 31)) * X3_DYROW + row * 16);
#pragma unroll
                for (int tt = 0; tt < 5; ++tt) {
                    const int t = tg * 5 + tt;
                    if (t < 9) {
                        const int d = t % 3, rr = row + t / 3;   // row + (t / 3 - 1) + the halo row
                        const h8 bh = *(const h8*)(xS + ((d * 2 + 0) * 32 + (lane & 31)) * X3_XROW + rr * 16);
                        const h8 bl = *(const h8*)(xS + ((d * 2 + 1) * 32 + (lane & 31)) * X3_XROW + rr * 16);
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[tt], 0, 0, 0);
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[tt], 0, 0, 0);
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[tt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!work) return;
    const float id = scdy[1], ix = scx[1];
    const int ic = ic0 + (lane & 31);
#pragma unroll
    for (int tt = 0; tt < 5; ++tt) {
        const int t = tg * 5 + tt;
        if (t < 9 && ic < Cin) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int oc = ocg + mtile * 32 + 8 * (v >> 2) + 4 * kg + (v & 3);
                if (oc < Cout) partial[(((size_t)s * Cout + oc) * Cin + ic) * 9 + t] = acc[tt][v] * id * ix;
            }
        }
    }
}
