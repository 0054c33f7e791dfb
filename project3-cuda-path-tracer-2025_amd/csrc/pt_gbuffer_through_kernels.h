// pt_gbuffer_through_kernels.h — kernels of the through-capture (include/pt/pt_gbuffer_through.h):
// the feature planes of the first non-specular surface behind up to K delta surfaces.
//
// Only a few pixels of a frame sit on mirrors or glass, so the chain is not a per-pixel loop (most
// lanes of most waves would idle for K rounds) but a small wavefront of its own:
//
//   k_chain_reset      clears the K + 1 queue counters (one 128-B line each)
//   k_gbuffer_seed     k_gbuffer's body (camera ray, intersect_scene, gbuffer_write) for pixels whose
//                      first hit is final; a delta hit forms its continuation ray instead and appends
//                      {origin | pixel, direction | t_sum} to queue 0
//   k_gbuffer_follow   round k = 1..K over ping-pong queues: dense waves of queued rays through the
//                      same intersect_scene (BVH stack in LDS, as k_intersect holds it); a ray that
//                      ends writes its pixel's planes, the rest go to the other queue; in round K
//                      everything ends.  The count is read on the device and the grid is sized for
//                      the worst case with an early exit (k_intersect's way): no host round trip.
//
// Appends are wave-aggregated: one ballot, one atomic per wave on the round's counter, ranks by
// mbcnt.  Queue order is therefore not deterministic; the planes are, every ray writing only its own
// pixel.  A pixel has at most one ray in flight, so a queue of `pixels` entries cannot overflow.
#pragma once

#include "pt_denoise_kernels.h"

namespace ptd {

// one round's rays: a[i] = origin.xyz | pixel (int bits), b[i] = direction.xyz | t_sum
struct ChainQueue {
    float4* a;
    float4* b;
    int* count;     // on a 128-B line of its own
};

struct ChainArgs {
    ChainQueue in, out;    // seed: `in` unused
    int* followed;         // delta surfaces followed, per pixel
    int cap;               // entries a queue holds (= pixels)
};

// the definition's "delta": shade_path scatters it (no emission) on a branch without random numbers
PT_DEV bool chain_is_delta(const DevMaterial& m) {
    return m.emittance <= 0.0f && (m.hasReflective > 0.0f || m.hasRefractive > 0.0f);
}

// The ray (o, d) that hit the delta surface h continues: shade_path's shading point and bump-map
// normal (pathtrace.cu:579-607), then scatter()'s transmissive branch for every refractive material
// (glass included: it always refracts) or its mirror branch, operation for operation.
PT_DEV void chain_continue(const SceneDev& sc, const Hit& h, const DevMaterial& m, f3& o, f3& d) {
    const f3 intersect = o + d * h.t;
    f3 normal = h.n;
    if (m.hasBumpMap && m.bumpID >= 0 && m.bumpID < sc.num_textures) {
        const HitAttr ha = hit_attr(sc, h);
        const f3 ng = h.n;
        const int4 ti = sc.texinfo[m.bumpID];
        const float du = 1.0f / float(ti.y);
        const float dv = 1.0f / float(ti.z);
        float t0[4], tu[4], tv[4];
        tex_fetch(sc, m.bumpID, ha.u, 1.f - ha.v, t0);
        tex_fetch(sc, m.bumpID, ha.u + du, 1.f - ha.v, tu);
        tex_fetch(sc, m.bumpID, ha.u, 1.f - (ha.v + dv), tv);
        const float dhdu = (tu[0] - t0[0]) / du;
        const float dhdv = (tv[0] - t0[0]) / dv;
        const float scale = m.bumpScale;
        const f3 dpdu_p = ha.dpdu + ng * (scale * dhdu);
        const f3 dpdv_p = ha.dpdv + ng * (scale * dhdv);
        normal = normalize(cross(dpdu_p, dpdv_p));
        if (dot(normal, ng) < 0.0f) normal = -normal;
    }
    f3 wiW = mk(0.f, 0.f, 0.f);
    if (m.hasRefractive > 0.0f) {                      // Transmissive (and Glass on this branch)
        (void)sample_spec_trans(mk(1.f, 1.f, 1.f), normal, d, m.ior, wiW);
        d = normalize_unit(wiW);
        o = intersect + d * LARGER_EPSILON;
    } else {                                           // Mirror
        wiW = reflect(d, normal);
        d = normalize_unit(wiW);
        o = intersect + normal * BABY_EPSILON;
    }
}

// The calling lanes (a divergent subset of the wave) append their rays: one atomic per wave.
PT_DEV void chain_append(const ChainQueue& q, int cap, f3 o, int pix, f3 d, float t_sum) {
    const uint64_t m = __ballot(1);
    const int lead = __builtin_ctzll(m);
    int base = 0;
    if ((int)(threadIdx.x & 63) == lead) base = atomicAdd(q.count, __popcll(m));
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int slot = __builtin_amdgcn_readlane(base, lead) + rank;
    if (slot >= cap) return;   // cannot happen (one ray per pixel); never write past the queue
    q.a[slot] = make_float4(o.x, o.y, o.z, __int_as_float(pix));
    q.b[slot] = make_float4(d.x, d.y, d.z, t_sum);
}

// One segment of a chain, shared by both kernels: the ray (o, d) of pixel `pix` has followed
// `followed` delta surfaces over a length t_prev and now hit h.  It ends here (miss, non-delta, or
// `followed` == the cap: planes written) or goes on in queue `c.out`.
PT_DEV void chain_segment(const SceneDev& sc, const GBuf& g, const ChainArgs& c, int pix, f3 o, f3 d, const Hit& h,
                          float t_prev, int followed, bool may_follow) {
    const float t_sum = t_prev + h.t;
    if (may_follow && h.t > 0.0f) {
        const DevMaterial m = sc.mats[h.mat];
        if (chain_is_delta(m)) {
            chain_continue(sc, h, m, o, d);
            chain_append(c.out, c.cap, o, pix, d, t_sum);
            return;
        }
    }
    gbuffer_write(sc, g, pix, o, d, h, t_sum);
    c.followed[pix] = followed;
}

__global__ void k_chain_reset(int* counters, int rounds) {
    if ((int)threadIdx.x < rounds) counters[threadIdx.x * CNT_PAD] = 0;
}

template <bool HAS_BVH, bool BVH_FAST>
__global__ __launch_bounds__(BLOCK) void k_gbuffer_seed(SceneDev sc, GBuf g, ChainArgs c, int iter, int n, int max_specular) {
    extern __shared__ int s_stack[];
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= n) return;
    const PathReg p = camera_ray(sc.cam, iter, sc.trace_depth, gid);
    const Hit h = intersect_scene<HAS_BVH, BVH_FAST>(sc, p.o, p.d, s_stack + threadIdx.x);
    chain_segment(sc, g, c, gid, p.o, p.d, h, 0.0f, 0, max_specular > 0);
}

// round `round` of `max_specular`: the rays that have followed `round` delta surfaces
template <bool HAS_BVH, bool BVH_FAST>
__global__ __launch_bounds__(BLOCK) void k_gbuffer_follow(SceneDev sc, GBuf g, ChainArgs c, int round, int max_specular) {
    extern __shared__ int s_stack[];
    const int n = min(*c.in.count, c.cap);
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (blockIdx.x * BLOCK >= n || gid >= n) return;
    const float4 a = c.in.a[gid], b = c.in.b[gid];
    const f3 o = mk(a.x, a.y, a.z), d = mk(b.x, b.y, b.z);
    const int pix = __float_as_int(a.w);
    const Hit h = intersect_scene<HAS_BVH, BVH_FAST>(sc, o, d, s_stack + threadIdx.x);
    chain_segment(sc, g, c, pix, o, d, h, b.w, round, round < max_specular);
}

}  // namespace ptd
