// pt_regress_kernels.h — kernels of the blockwise feature regression (include/pt/pt_denoise_regress.h).
//
//   k_regress_fit    one 256-thread workgroup per 32 x 32 image block: the block's guides and colour
//                    staged in LDS, lo / hi of the samples' positions by a wave reduction, the Gram
//                    matrix of Z = [F | C | 0] (n x 16) with v_mfma_f32_16x16x4_f32, and the 10 x 10
//                    ridge system factored and solved by wave 0, one lane per column
//   k_regress_apply  16 x 16 pixel tiles: the four block records a tile lies in read once into LDS,
//                    every thread evaluates its pixel's four fits and the tent blend, multiplies
//                    the albedo back and writes the float3 host layout and the 8-bit PBO
//
// The filter is defined in include/pt/pt_denoise_regress.h; tests/test_denoise_regress.py restates
// it in numpy.  No atomics; every sum has a fixed order.
#pragma once

#include "pt_denoise_kernels.h"

namespace ptd {

constexpr int RG_STRIDE = 16;                      // block stride in pixels; a block is 2 x 2 strides
constexpr int RG_SIDE = 2 * RG_STRIDE;
constexpr int RG_SLOTS = RG_SIDE * RG_SIDE;        // 1024 pixel slots per block, 4 per thread
constexpr int RG_FEATURES = 10;
constexpr int RG_BLOCK_FLOATS = 7 + 3 * RG_FEATURES;   // n | lo | hi | beta[10][3] = PT_REGRESS_BLOCK_FLOATS
constexpr int RG_REC = 64;                         // floats per record of the block table (256 B)
// the staged block, one LDS row per quantity (normal 0-2, position 3-5, colour 6-8, sample flag 9).
// Rows are 1024 + 4 floats apart: in the Gram loop lane (f, k) reads row(f)[4 s + k], bank
// 4 row + k + const -- the 40 (row, k) pairs of a step fall in 40 different banks
constexpr int RG_LD = RG_SLOTS + 4;
constexpr int RG_ROWS = 10, RG_ROW_X = 3, RG_ROW_C = 6, RG_ROW_FLAG = 9;

struct RegressArgs {
    const float* image;        // the accumulated image (float3 per pixel)
    const float4* gn;          // normal | t
    const float4* gx;          // position | hit flag
    const float4* ga;          // albedo | material
    const DevMaterial* mats;
    float* tab;                // the block table, RG_REC floats per block, blocks (j, i) row-major
    float* out3;               // the result in the host layout (float3 per pixel)
    pt_uchar4* pbo;            // sendImageToPBO(result, 1), or null
    int W, H, nbx, num_mats;
    int demod;
    float samples;             // c0 = image / samples
    float ridge;
};

struct RegressPixel {
    float c[3];      // c0 (divided by the albedo where demodulated)
    bool hit;        // the albedo was divided out (with demod)
    bool surface;    // hit, and the material emits nothing
    bool finite;     // c0 finite in all three channels
};

PT_DEV RegressPixel rg_pixel(const RegressArgs& a, int idx, float hit_flag, float4 al) {
    RegressPixel p;
    p.hit = hit_flag > 0.5f;
    p.finite = at_c0(a.image, idx, a.samples, a.demod, p.hit, al, p.c[0], p.c[1], p.c[2]);
    const int m = (int)al.w;
    p.surface = p.hit && m >= 0 && m < a.num_mats && !(a.mats[m].emittance > 0.0f);
    return p;
}

// xs of one axis: (x - lo) / (hi - lo), 0 where hi = lo
PT_DEV float rg_unit(float x, float lo, float hi) {
    const float d = hi - lo;
    return d > 0.0f ? (x - lo) / d : 0.0f;
}

// ---- wave-level exchange: ds_swizzle butterflies within 32 lanes, v_readlane across the halves ----
template <int XOR>
PT_DEV float rg_swizzle(float v) {   // bit-mask mode: and 0x1f, or 0, xor XOR
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (XOR << 10) | 0x1f));
}
PT_DEV float rg_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

PT_DEV float rg_wave_min(float v) {
    v = __builtin_fminf(v, rg_swizzle<1>(v));
    v = __builtin_fminf(v, rg_swizzle<2>(v));
    v = __builtin_fminf(v, rg_swizzle<4>(v));
    v = __builtin_fminf(v, rg_swizzle<8>(v));
    v = __builtin_fminf(v, rg_swizzle<16>(v));
    return __builtin_fminf(rg_lane(v, 0), rg_lane(v, 32));
}
PT_DEV float rg_wave_max(float v) { return -rg_wave_min(-v); }

typedef float rg_f4 __attribute__((ext_vector_type(4)));

// both kernels are compiled without packed fp32 arithmetic (v_pk_add / mul / fma_f32), whatever the
// translation unit's vectorizer settings: every sum and product is the scalar IEEE operation
#ifdef __HIP_DEVICE_COMPILE__
#define RG_KERNEL __global__ __launch_bounds__(BLOCK) __attribute__((target("no-packed-fp32-ops")))
#else
#define RG_KERNEL __global__ __launch_bounds__(BLOCK)
#endif

RG_KERNEL void k_regress_fit(RegressArgs a) {
    __shared__ float s_v[RG_ROWS * RG_LD];      // 41 KB
    __shared__ float s_red[4][6];               // lo, hi of every wave
    __shared__ float s_g[4][256];               // the waves' partial Gram matrices
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int x0 = (int)blockIdx.x * RG_STRIDE - RG_STRIDE, y0 = (int)blockIdx.y * RG_STRIDE - RG_STRIDE;

    // 1. stage: slot = ly * 32 + lx; a thread takes slots t, t + 256, ... (a row of 32 pixels per
    // half wave).  What is no sample (outside the image, a miss, an emitter, a non-finite colour)
    // is a zero row of Z
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < RG_SLOTS / BLOCK; ++q) {
        const int slot = t + q * BLOCK;
        const int x = x0 + (slot & (RG_SIDE - 1)), y = y0 + slot / RG_SIDE;
        float v[RG_ROWS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
            const int idx = y * a.W + x;
            const float4 xp = a.gx[idx];
            const RegressPixel p = rg_pixel(a, idx, xp.w, a.ga[idx]);
            if (p.surface && p.finite) {
                const float4 np = a.gn[idx];
                v[0] = np.x, v[1] = np.y, v[2] = np.z;
                v[3] = xp.x, v[4] = xp.y, v[5] = xp.z;
                v[6] = p.c[0], v[7] = p.c[1], v[8] = p.c[2];
                v[9] = 1.0f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    lo[k] = __builtin_fminf(lo[k], v[RG_ROW_X + k]);
                    hi[k] = __builtin_fmaxf(hi[k], v[RG_ROW_X + k]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RG_ROWS; ++r) s_v[r * RG_LD + slot] = v[r];
    }

    // 2. lo, hi: within the wave, then the four waves in wave order
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = rg_wave_min(lo[k]);
        hi[k] = rg_wave_max(hi[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_red[wave][k] = lo[k], s_red[wave][3 + k] = hi[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = __builtin_fminf(__builtin_fminf(s_red[0][k], s_red[1][k]), __builtin_fminf(s_red[2][k], s_red[3][k]));
        hi[k] = __builtin_fmaxf(__builtin_fmaxf(s_red[0][3 + k], s_red[1][3 + k]),
                                __builtin_fmaxf(s_red[2][3 + k], s_red[3][3 + k]));
    }
    // positions -> xs, in place, every thread its own slots
#pragma unroll
    for (int q = 0; q < RG_SLOTS / BLOCK; ++q) {
        const int slot = t + q * BLOCK;
        if (s_v[RG_ROW_FLAG * RG_LD + slot] != 0.0f) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float* px = &s_v[(RG_ROW_X + k) * RG_LD + slot];
                *px = rg_unit(*px, lo[k], hi[k]);
            }
        }
    }
    __syncthreads();

    // 3. G = Z^T Z.  One v_mfma_f32_16x16x4_f32 multiplies a 16 x 4 by a 4 x 16 matrix; its A operand
    // holds A[f][k] in lane 16 k + f and its B operand B[k][f] in the same lane, so with A = B^T (four
    // rows of Z) one register feeds both.  Lane (f, k) forms column f of Z for slot 4 s + k of the
    // wave's quarter: f 0 the constant (the sample flag), 1-3 the normal, 4-6 xs, 7-9 xs^2,
    // 10-12 the colour, 13-15 the zero padding.
    const int f = lane & 15, k4 = lane >> 4;
    const int row = f == 0 ? RG_ROW_FLAG : (f < 7 ? f - 1 : (f < 13 ? f - 4 : 0));
    const bool square = f >= 7 && f < 10, pad = f >= 13;
    const float* src = s_v + row * RG_LD + wave * (RG_SLOTS / 4) + k4;
    rg_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int s = 0; s < RG_SLOTS / 16; ++s) {
        float z = src[4 * s];
        z = square ? z * z : z;
        z = pad ? 0.0f : z;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(z, z, acc, 0, 0, 0);
    }
    // the result: lane 16 k + f holds G[4 k + r][f] in element r
#pragma unroll
    for (int r = 0; r < 4; ++r) s_g[wave][(4 * k4 + r) * 16 + f] = acc[r];
    __syncthreads();
    if (wave != 0) return;

    // 4. wave 0: lane j holds column j of [F^T F + ridge n D | F^T C] (columns 0-9 | 10-12; the
    // lanes past 12 compute along on padding and write nothing).  Cholesky A = R^T R row by row:
    // row k divided by sqrt of its diagonal, then taken out of the rows below, R[k][i] broadcast
    // from lane i.  The right-hand columns go through the same steps, which leaves R^-T F^T C in them.
    const int j = lane;
    float col[RG_FEATURES];
#pragma unroll
    for (int i = 0; i < RG_FEATURES; ++i)
        col[i] = ((s_g[0][i * 16 + j] + s_g[1][i * 16 + j]) + s_g[2][i * 16 + j]) + s_g[3][i * 16 + j];
    const float n = rg_lane(col[0], 0);          // a sum of ones: exact
    float* rec = a.tab + ((size_t)blockIdx.y * a.nbx + blockIdx.x) * RG_REC;
    if (n == 0.0f) {                             // no sample, no fit
        if (lane < RG_BLOCK_FLOATS) rec[lane] = 0.0f;
        return;
    }
    const float rn = __builtin_fminf(a.ridge * n, 3.0e38f);
#pragma unroll
    for (int i = 1; i < RG_FEATURES; ++i) col[i] = j == i ? col[i] + rn : col[i];
#pragma unroll
    for (int k = 0; k < RG_FEATURES; ++k) {
        // in exact arithmetic pivot k >= 1 is at least ridge n (a Schur complement of F^T F, which is
        // positive semidefinite, plus ridge n) and pivot 0 is n: rounding may not take it below that
        const float pivot = rg_lane(col[k], k);
        const float d = __builtin_sqrtf(k == 0 ? n : __builtin_fmaxf(pivot, rn));
        col[k] = col[k] / d;
#pragma unroll
        for (int i = k + 1; i < RG_FEATURES; ++i) col[i] = col[i] - rg_lane(col[k], i) * col[k];
    }
    // R beta = R^-T F^T C, from the last row up; every right-hand lane its own channel
    float beta[RG_FEATURES];
#pragma unroll
    for (int k = RG_FEATURES - 1; k >= 0; --k) {
        float s = col[k];
#pragma unroll
        for (int i = k + 1; i < RG_FEATURES; ++i) s = s - rg_lane(col[k], i) * beta[i];
        beta[k] = s / rg_lane(col[k], k);
    }
    // 5. the record: n | lo | hi | beta[10][3]
    if (lane == 0) {
        rec[0] = n;
#pragma unroll
        for (int k = 0; k < 3; ++k) rec[1 + k] = lo[k], rec[4 + k] = hi[k];
    }
    if (lane >= RG_FEATURES && lane < RG_FEATURES + 3) {
#pragma unroll
        for (int i = 0; i < RG_FEATURES; ++i) rec[7 + 3 * i + (lane - RG_FEATURES)] = beta[i];
    }
}

RG_KERNEL void k_regress_apply(RegressArgs a) {
    // the records of blocks (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1), i, j this tile's indices:
    // the four blocks every pixel of the tile lies in, in (j, i) order
    __shared__ float s_rec[4][RG_BLOCK_FLOATS + 3];
    const int t = threadIdx.x;
    if (t < 4 * RG_BLOCK_FLOATS) {
        const int b = t / RG_BLOCK_FLOATS, e = t - b * RG_BLOCK_FLOATS;
        const int bi = (int)blockIdx.x + (b & 1), bj = (int)blockIdx.y + (b >> 1);   // bi <= ceil(W / 16) = nbx - 1
        s_rec[b][e] = a.tab[((size_t)bj * a.nbx + bi) * RG_REC + e];
    }
    __syncthreads();
    const int x = (int)blockIdx.x * RG_STRIDE + t % RG_STRIDE, y = (int)blockIdx.y * RG_STRIDE + t / RG_STRIDE;
    if (x >= a.W || y >= a.H) return;
    const int idx = y * a.W + x;
    const float4 xp = a.gx[idx], al = a.ga[idx];
    const RegressPixel p = rg_pixel(a, idx, xp.w, al);
    float o[3] = {0.f, 0.f, 0.f};
    if (!p.surface) {            // a miss or an emitter passes through
        if (p.finite) o[0] = p.c[0], o[1] = p.c[1], o[2] = p.c[2];
    } else {
        const float4 np = a.gn[idx];
        const float pos[3] = {xp.x, xp.y, xp.z};
        float sum[3] = {0.f, 0.f, 0.f}, wsum = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float* rec = s_rec[b];
            if (!(rec[0] > 0.0f)) continue;      // n = 0: no fit
            const int bi = (int)blockIdx.x + (b & 1), bj = (int)blockIdx.y + (b >> 1);
            const float wx = 1.0f - __builtin_fabsf((float)x - ((float)(RG_STRIDE * bi) - 0.5f)) * (1.0f / RG_STRIDE);
            const float wy = 1.0f - __builtin_fabsf((float)y - ((float)(RG_STRIDE * bj) - 0.5f)) * (1.0f / RG_STRIDE);
            const float w = wx * wy;             // multiples of 1/32: exact
            float fr[RG_FEATURES];
            fr[0] = 1.0f, fr[1] = np.x, fr[2] = np.y, fr[3] = np.z;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                fr[4 + k] = rg_unit(pos[k], rec[1 + k], rec[4 + k]);
                fr[7 + k] = fr[4 + k] * fr[4 + k];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float v = rec[7 + ch];           // the constant's coefficient
#pragma unroll
                for (int i = 1; i < RG_FEATURES; ++i) v = v + fr[i] * rec[7 + 3 * i + ch];
                sum[ch] = sum[ch] + w * (at_finite(v) ? __builtin_fmaxf(v, 0.0f) : 0.0f);   // a fit that overflowed counts as 0
            }
            wsum = wsum + w;
        }
        if (wsum != 0.0f) o[0] = sum[0] / wsum, o[1] = sum[1] / wsum, o[2] = sum[2] / wsum;
    }
    if (a.demod && p.hit) {      // the albedo back where it was divided out
        o[0] = o[0] * __builtin_fmaxf(al.x, AT_ALBEDO_MIN);
        o[1] = o[1] * __builtin_fmaxf(al.y, AT_ALBEDO_MIN);
        o[2] = o[2] * __builtin_fmaxf(al.z, AT_ALBEDO_MIN);
    }
    a.out3[3 * (size_t)idx] = o[0];
    a.out3[3 * (size_t)idx + 1] = o[1];
    a.out3[3 * (size_t)idx + 2] = o[2];
    if (a.pbo) {
        pt_uchar4 u;
        u.x = at_to_u8(o[0]);
        u.y = at_to_u8(o[1]);
        u.z = at_to_u8(o[2]);
        u.w = 0;
        a.pbo[idx] = u;
    }
}

}  // namespace ptd
