// pt_denoise_kernels.h — kernels of the edge-avoiding a-trous denoiser (include/pt/pt_denoise.h).
//
//   k_gbuffer   first hit of camera_ray(iteration) per pixel: the production camera, primitive
//               tests, BVH traversal and finish_hit (intersect_scene, as k_intersect runs it), so
//               normal and t are the record the wavefront writes for the same ray, bit for bit
//   k_atrous    one level of the filter: 5 x 5 taps at step s, weights from colour, normal and
//               position; steps 1 and 2 stage the block's tile + halo in LDS, steps >= 4 read
//               their (strided) taps directly, a tap row's loads issued together
//
// The filter is defined in include/pt/pt_denoise.h; tests/test_denoise.py restates it in numpy.
#pragma once

#include "pt_kernels.h"

namespace ptd {

// the three feature planes, one float4 per pixel each
struct GBuf {
    float4* nt;    // normal.xyz | t             (0, -1 on a miss)
    float4* pos;   // origin + t * dir | hit flag 1 / 0   (0 on a miss)
    float4* alb;   // albedo.rgb | materialId as float    (0, -1 on a miss)
};

template <bool HAS_BVH, bool BVH_FAST>
__global__ __launch_bounds__(BLOCK) void k_gbuffer(SceneDev sc, GBuf g, int iter, int n) {
    extern __shared__ int s_stack[];
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= n) return;
    const PathReg p = camera_ray(sc.cam, iter, sc.trace_depth, gid);
    const Hit h = intersect_scene<HAS_BVH, BVH_FAST>(sc, p.o, p.d, s_stack + threadIdx.x);
    float4 pos = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 alb = make_float4(0.f, 0.f, 0.f, -1.0f);
    if (h.t > 0.0f) {
        const f3 x = p.o + p.d * h.t;   // the shading point, rounded as shade_path rounds it
        pos = make_float4(x.x, x.y, x.z, 1.0f);
        const DevMaterial m = sc.mats[h.mat];
        f3 c = mk(m.color[0], m.color[1], m.color[2]);
        if (m.hasTexture) {             // sampleTexture as shade_path calls it (pathtrace.cu:505-519)
            if (m.textureID < 0 || m.textureID >= sc.num_textures) {
                c = mk(1.0f, 0.0f, 1.0f);
            } else {
                const HitAttr a = hit_attr(sc, h);
                float t[4];
                tex_fetch(sc, m.textureID, a.u, 1.f - a.v, t);
                c = mk(t[0], t[1], t[2]);
            }
        }
        alb = make_float4(c.x, c.y, c.z, (float)h.mat);
    }
    g.nt[gid] = make_float4(h.n.x, h.n.y, h.n.z, h.t);
    g.pos[gid] = pos;
    g.alb[gid] = alb;
}

// ---- the filter ----------------------------------------------------------------------------
constexpr int AT_TILE = 16;               // a block filters a 16 x 16 pixel tile (256 threads)
constexpr float AT_ALBEDO_MIN = 1e-3f;    // demodulation divides by max(albedo, this)

struct AtrousArgs {
    const float* image;    // first level: the accumulated image (float3 per pixel)
    const float4* cin;     // later levels: colour rgb | 1 (finite) or 0 0 0 | 0 (not finite)
    float4* cout;          // all but the last level
    float* out3;           // last level: the result in the host layout (float3 per pixel)
    pt_uchar4* pbo;        // last level: sendImageToPBO(result, 1), or null
    const float4* gn;      // normal | t
    const float4* gx;      // position | hit flag
    const float4* ga;      // albedo | material
    int W, H;
    int step;
    int first, last, demod;
    float samples;         // c0 = image / samples
    float k_color, k_normal, k_position;   // 1 / sigma^2 (colour: of this level)
};

PT_DEV bool at_finite(float v) { return v - v == 0.0f; }

// the level's input colour at pixel idx
PT_DEV float4 at_load_color(const AtrousArgs& a, int idx, float hit) {
    if (!a.first) return a.cin[idx];
    float r = a.image[3 * (size_t)idx] / a.samples;
    float g = a.image[3 * (size_t)idx + 1] / a.samples;
    float b = a.image[3 * (size_t)idx + 2] / a.samples;
    if (a.demod && hit > 0.5f) {
        const float4 al = a.ga[idx];
        r = r / __builtin_fmaxf(al.x, AT_ALBEDO_MIN);
        g = g / __builtin_fmaxf(al.y, AT_ALBEDO_MIN);
        b = b / __builtin_fmaxf(al.z, AT_ALBEDO_MIN);
    }
    const bool fin = at_finite(r) && at_finite(g) && at_finite(b);
    return fin ? make_float4(r, g, b, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.0f);
}

struct AtrousAcc {
    float r, g, b, w;
};

// one tap: (colour | finite, normal, position | hit) of q against the centre's; hh = h[i] h[j]
PT_DEV void at_tap(AtrousAcc& s, const AtrousArgs& a, float hh, float4 cp, float4 np, float4 xp, float4 cq,
                   float4 nq, float4 xq) {
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float dc = cp.w > 0.5f ? (dr * dr + dg * dg) + db * db : 0.0f;   // non-finite centre: colour term 1
    const float n0 = np.x - nq.x, n1 = np.y - nq.y, n2 = np.z - nq.z;
    const float x0 = xp.x - xq.x, x1 = xp.y - xq.y, x2 = xp.z - xq.z;
    const float dn = (n0 * n0 + n1 * n1) + n2 * n2;   // two misses: planes hold 0, the terms are 1
    const float dx = (x0 * x0 + x1 * x1) + x2 * x2;
    const float e = (dc * a.k_color + dn * a.k_normal) + dx * a.k_position;
    // outside taps carry hit flag -1 and finite flag 0; a non-finite tap's colour is stored as 0
    const bool on = xq.w == xp.w && cq.w > 0.5f;
    const float w = on ? hh * __expf(-e) : 0.0f;
    s.r += w * cq.x;
    s.g += w * cq.y;
    s.b += w * cq.z;
    s.w += w;
}

PT_DEV uint8_t at_to_u8(float v) {   // sendImageToPBO's conversion with iteration 1 (k_to_pbo)
    const double d = (double)(v / 1.0f) * 255.0;
    const int i = (d != d) ? 0 : (d >= 2147483647.0 ? 2147483647 : (d <= -2147483648.0 ? (-2147483647 - 1) : (int)d));
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

PT_DEV void at_store(const AtrousArgs& a, int idx, const AtrousAcc& s, float hit) {
    float r = 0.f, g = 0.f, b = 0.f;
    if (s.w != 0.0f) {
        r = s.r / s.w;
        g = s.g / s.w;
        b = s.b / s.w;
    }
    if (!a.last) {
        const bool fin = at_finite(r) && at_finite(g) && at_finite(b);
        a.cout[idx] = fin ? make_float4(r, g, b, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.0f);
        return;
    }
    if (a.demod && hit > 0.5f) {   // the albedo back where it was divided out
        const float4 al = a.ga[idx];
        r = r * __builtin_fmaxf(al.x, AT_ALBEDO_MIN);
        g = g * __builtin_fmaxf(al.y, AT_ALBEDO_MIN);
        b = b * __builtin_fmaxf(al.z, AT_ALBEDO_MIN);
    }
    a.out3[3 * (size_t)idx] = r;
    a.out3[3 * (size_t)idx + 1] = g;
    a.out3[3 * (size_t)idx + 2] = b;
    if (a.pbo) {
        pt_uchar4 o;
        o.x = at_to_u8(r);
        o.y = at_to_u8(g);
        o.z = at_to_u8(b);
        o.w = 0;
        a.pbo[idx] = o;
    }
}

PT_DEV float at_h(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }

// steps 1 and 2: the tile and its halo of 2 S pixels, staged once in LDS (S = 2: 24 x 24 entries
// of 48 B = 27 KB), every tap an LDS read
template <int S>
__global__ __launch_bounds__(BLOCK) void k_atrous_lds(AtrousArgs a) {
    constexpr int R = 2 * S, TW = AT_TILE + 2 * R;
    __shared__ float4 s_c[TW * TW], s_n[TW * TW], s_x[TW * TW];
    const int bx = blockIdx.x * AT_TILE, by = blockIdx.y * AT_TILE;
    for (int i = threadIdx.x; i < TW * TW; i += BLOCK) {
        const int ly = i / TW, lx = i - ly * TW;
        const int x = bx - R + lx, y = by - R + ly;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.0f), n = c, p = make_float4(0.f, 0.f, 0.f, -1.0f);
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
            const int idx = y * a.W + x;
            n = a.gn[idx];
            p = a.gx[idx];
            c = at_load_color(a, idx, p.w);
        }
        s_c[i] = c;
        s_n[i] = n;
        s_x[i] = p;
    }
    __syncthreads();
    const int tx = threadIdx.x % AT_TILE, ty = threadIdx.x / AT_TILE;
    const int x = bx + tx, y = by + ty;
    if (x >= a.W || y >= a.H) return;
    const int lc = (ty + R) * TW + tx + R;
    const float4 cp = s_c[lc], np = s_n[lc], xp = s_x[lc];
    AtrousAcc s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int l = lc + (j * TW + i) * S;
            at_tap(s, a, at_h(i) * at_h(j), cp, np, xp, s_c[l], s_n[l], s_x[l]);
        }
    }
    at_store(a, y * a.W + x, s, xp.w);
}

// steps >= 4: taps read directly (a halo of 2 s pixels no longer pays); the 15 loads of a tap
// row are independent of the arithmetic before them
__global__ __launch_bounds__(BLOCK) void k_atrous_direct(AtrousArgs a) {
    const int tx = threadIdx.x % AT_TILE, ty = threadIdx.x / AT_TILE;
    const int x = blockIdx.x * AT_TILE + tx, y = blockIdx.y * AT_TILE + ty;
    if (x >= a.W || y >= a.H) return;
    const int pc = y * a.W + x;
    const float4 np = a.gn[pc], xp = a.gx[pc];
    const float4 cp = at_load_color(a, pc, xp.w);
    AtrousAcc s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * a.step;
        const bool row = qy >= 0 && qy < a.H;
        const int cy = row ? qy : y;
        float4 cq[5], nq[5], xq[5];
        bool in[5];
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * a.step;
            in[i + 2] = row && qx >= 0 && qx < a.W;
            const int q = in[i + 2] ? cy * a.W + qx : pc;   // outside: a valid address, weight 0 below
            nq[i + 2] = a.gn[q];
            xq[i + 2] = a.gx[q];
            cq[i + 2] = at_load_color(a, q, xq[i + 2].w);
        }
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            if (!in[i + 2]) cq[i + 2].w = 0.0f;
            at_tap(s, a, at_h(i) * at_h(j), cp, np, xp, cq[i + 2], nq[i + 2], xq[i + 2]);
        }
    }
    at_store(a, pc, s, xp.w);
}

}  // namespace ptd
