// pt_temporal_kernels.h — kernels of the denoiser's temporal stage (include/pt/pt_denoise_temporal.h).
//
//   k_reproject           once per capture: every hit pixel's first-hit point through the history's
//                         camera, four bilinear taps of the history's planes tested against the
//                         pixel's material, normal and plane -> the base colour | N and moments.
//                         A gather at data-dependent addresses: nothing to stage, one thread a pixel
//   k_temporal_integrate  every call: base + c0 -> integrated colour | N, moments and variance.  A
//                         block takes a 16 x 16 tile; L(c0) and a key (material, or "not usable")
//                         of the tile + a 3-pixel halo (22 x 22) go through LDS, computed from the
//                         image on the way in, so c0 is formed once per pixel and halo pixel and the
//                         7 x 7 window of the spatial variance reads LDS only
//
// The variance-guided a-trous levels are k_atrous_*_var of pt_denoise_kernels.h.  The stages are
// defined in the header; tests/test_denoise_temporal.py restates them in numpy.
#pragma once

#include "pt_denoise_kernels.h"

namespace ptd {

PT_DEV float tp_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

struct ReprojectArgs {
    GBuf cur, hist;              // the capture's planes, the history's planes
    const float4* hcol;          // history colour rgb | N (0 0 0 | 0: not finite)
    const float4* hmom;          // history mu1, mu2, variance, 0
    float4* bcol;                // base colour rgb | N_base
    float4* bmom;                // base mu1, mu2, 0, 0
    CamDev cam;                  // the history's camera
    int n;
    int has_history;             // 0: every pixel's base is 0
    float max_history, normal_cos_min, plane_tol;
};

__global__ __launch_bounds__(BLOCK) void k_reproject(ReprojectArgs a) {
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= a.n) return;
    float4 oc = make_float4(0.f, 0.f, 0.f, 0.f), om = oc;
    const float4 xp = a.cur.pos[gid];
    if (a.has_history && xp.w > 0.5f) {
        const float4 nt = a.cur.nt[gid];
        const float m = a.cur.alb[gid].w;
        const f3 X = mk(xp.x, xp.y, xp.z), n = mk(nt.x, nt.y, nt.z);
        const f3 v = X - a.cam.position;
        const float d = dot(v, a.cam.view);
        if (d > 1e-6f) {
            const float W = (float)a.cam.resx, H = (float)a.cam.resy;
            float u = (-dot(v, a.cam.right) / (d * a.cam.plx) + W * 0.5f) - 0.5f;
            float w = (-dot(v, a.cam.up) / (d * a.cam.ply) + H * 0.5f) - 0.5f;
            // far outside (or NaN): every tap is outside either way; keeps the int conversion defined
            u = __builtin_fminf(__builtin_fmaxf(u, -2.0f), W + 1.0f);
            w = __builtin_fminf(__builtin_fmaxf(w, -2.0f), H + 1.0f);
            const float fx0 = __builtin_floorf(u), fy0 = __builtin_floorf(w);
            const float fx = u - fx0, fy = w - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float tol = a.plane_tol * nt.w;
            float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    if (qx < 0 || qx >= a.cam.resx || qy < 0 || qy >= a.cam.resy) continue;
                    const int q = qy * a.cam.resx + qx;
                    const float4 hx = a.hist.pos[q], hn = a.hist.nt[q], hc = a.hcol[q];
                    const float hm = a.hist.alb[q].w;
                    const float cosn = dot(n, mk(hn.x, hn.y, hn.z));
                    const float pd = __builtin_fabsf(dot(mk(hx.x, hx.y, hx.z) - X, n));
                    const bool fin = at_finite(hc.x) && at_finite(hc.y) && at_finite(hc.z) && hc.w > 0.0f;
                    if (!(hx.w > 0.5f && hm == m && cosn >= a.normal_cos_min && pd <= tol && fin)) continue;
                    const float bw = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                    const float4 hmo = a.hmom[q];
                    sw += bw;
                    sr += bw * hc.x;
                    sg += bw * hc.y;
                    sb += bw * hc.z;
                    sn += bw * hc.w;
                    s1 += bw * hmo.x;
                    s2 += bw * hmo.y;
                }
            }
            if (sw >= 1e-3f) {
                oc = make_float4(sr / sw, sg / sw, sb / sw, __builtin_fminf(sn / sw, a.max_history));
                om = make_float4(s1 / sw, s2 / sw, 0.f, 0.f);
            }
        }
    }
    a.bcol[gid] = oc;
    a.bmom[gid] = om;
}

// ---- integration + variance ----------------------------------------------------------------
constexpr int TP_HALO = 3;                          // the 7 x 7 variance window
constexpr int TP_TW = AT_TILE + 2 * TP_HALO;        // 22
constexpr int TP_NHALO = TP_TW * TP_TW - AT_TILE * AT_TILE;   // 228 halo cells, < BLOCK
constexpr int TP_KEY_NONE = -2;                     // outside the image or not finite (a miss has material -1)

struct IntegrateArgs {
    const float* image;          // the accumulated image (float3 per pixel)
    const float4* ga;            // albedo | material (>= 0 exactly at hit pixels)
    const float4* bcol;          // base
    const float4* bmom;
    float4* col;                 // integrated colour rgb | N (0 0 0 | 0: not finite and no history)
    float4* mom;                 // mu1, mu2, variance, 0
    int W, H;
    int demod;
    float samples;
    float var_hist_min;          // temporal variance where N_base >= this
};

// c0 of pixel idx (at_c0; a hit is a material >= 0 here); returns the material
PT_DEV float tp_load_c0(const IntegrateArgs& a, int idx, float& r, float& g, float& b, bool& fin) {
    const float4 al = a.ga[idx];
    fin = at_c0(a.image, idx, a.samples, a.demod, al.w >= 0.0f, al, r, g, b);
    return al.w;
}

__global__ __launch_bounds__(BLOCK) void k_temporal_integrate(IntegrateArgs a) {
    __shared__ float s_l[TP_TW * TP_TW];
    __shared__ int s_key[TP_TW * TP_TW];
    const int bx = blockIdx.x * AT_TILE, by = blockIdx.y * AT_TILE;
    const int tx = threadIdx.x % AT_TILE, ty = threadIdx.x / AT_TILE;
    const int x = bx + tx, y = by + ty;
    const bool inside = x < a.W && y < a.H;
    const int lc = (ty + TP_HALO) * TP_TW + tx + TP_HALO;
    // pass 1: the thread's own pixel; c0 stays in registers for the integration
    float r = 0.f, g = 0.f, b = 0.f, lum = 0.f, mat = -1.0f;
    bool fin = false;
    if (inside) {
        mat = tp_load_c0(a, y * a.W + x, r, g, b, fin);
        lum = fin ? tp_luma(r, g, b) : 0.0f;
    }
    s_l[lc] = lum;
    s_key[lc] = fin ? (int)mat : TP_KEY_NONE;
    // pass 2: the 228 halo cells, one each for the first 228 threads: 3 rows above, 3 below, then
    // 3 + 3 columns beside each of the tile's 16 rows
    if (threadIdx.x < TP_NHALO) {
        const int i = threadIdx.x;
        int lx, ly;
        if (i < 2 * TP_HALO * TP_TW) {
            const int k = i < TP_HALO * TP_TW ? i : i - TP_HALO * TP_TW;
            ly = k / TP_TW + (i < TP_HALO * TP_TW ? 0 : TP_HALO + AT_TILE);
            lx = k % TP_TW;
        } else {
            const int k = i - 2 * TP_HALO * TP_TW, c = k % (2 * TP_HALO);
            ly = TP_HALO + k / (2 * TP_HALO);
            lx = c < TP_HALO ? c : c + AT_TILE;
        }
        const int hx = bx - TP_HALO + lx, hy = by - TP_HALO + ly;
        float hl = 0.f;
        int key = TP_KEY_NONE;
        if (hx >= 0 && hx < a.W && hy >= 0 && hy < a.H) {
            float hr, hg, hb;
            bool hf;
            const float hm = tp_load_c0(a, hy * a.W + hx, hr, hg, hb, hf);
            if (hf) {
                hl = tp_luma(hr, hg, hb);
                key = (int)hm;
            }
        }
        s_l[ly * TP_TW + lx] = hl;
        s_key[ly * TP_TW + lx] = key;
    }
    __syncthreads();
    if (!inside) return;
    const int idx = y * a.W + x;
    const float4 bc = a.bcol[idx], bm = a.bmom[idx];
    float4 oc = bc, om = make_float4(bm.x, bm.y, 0.f, 0.f);
    if (fin) {
        const float N = bc.w + a.samples;
        const float al = a.samples / N, be = 1.0f - al;
        oc = make_float4(be * bc.x + al * r, be * bc.y + al * g, be * bc.z + al * b, N);
        om.x = be * bm.x + al * lum;
        om.y = be * bm.y + al * (lum * lum);
    }
    float var;
    if (bc.w >= a.var_hist_min) {
        var = om.y - om.x * om.x;
    } else {
        const int key = (int)mat;
        float sl = 0.f, sl2 = 0.f, cnt = 0.f;
#pragma unroll
        for (int j = -TP_HALO; j <= TP_HALO; ++j) {
#pragma unroll
            for (int i = -TP_HALO; i <= TP_HALO; ++i) {
                const int l = lc + j * TP_TW + i;
                const float ql = s_l[l];
                const bool on = s_key[l] == key;
                sl += on ? ql : 0.0f;
                sl2 += on ? ql * ql : 0.0f;
                cnt += on ? 1.0f : 0.0f;
            }
        }
        var = 0.0f;
        if (cnt > 0.0f) {
            const float mean = sl / cnt;
            var = sl2 / cnt - mean * mean;
        }
    }
    om.z = __builtin_fmaxf(var, 0.0f);
    a.col[idx] = oc;
    a.mom[idx] = om;
}

}  // namespace ptd
