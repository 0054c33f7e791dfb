// pt_naive_mesh_kernels.h — the kernel of the NAIVE_MESH_LOADING mode (include/pt/pt_naive_mesh.h).
//
//   k_naive_mesh   the brute-force mesh loop of computeIntersections (pathtrace.cu:365-393): every
//                  triangle in array order against every live path, once per bounce, after the
//                  primitives-only k_intersect wrote its records.  A record is replaced only when
//                  a triangle has t > 0 && t < t_min (t_min: the primitive winner's t, or FLT_MAX
//                  on a miss), the first triangle of minimal t winning.
//
// Every lane of a wave tests the same triangle at the same time, so the block stages tiles of
// NAIVE_TILE triangles in LDS -- v0 and the two edges v1 - v0, v2 - v0, the differences
// tri_test() forms, rounded once by the staging thread -- and every lane reads them with
// same-address (broadcast) loads: 9 floats per triangle, 9 KB per tile.  Per-lane state in the
// loop is the ray, t_min and the winner's index; u, v, the normal, the material and the
// tangents come from ONE more test of the winner after the loop, through make_hit / hit_attr (the
// code finish_hit runs for a BVH hit), ray-facing flip included.
// The tile loop's trip count depends on num_tris alone, so every thread of a block that runs at
// all reaches both barriers, lanes past the end of the path array included.
#pragma once

#include "pt_kernels.h"

namespace ptd {

constexpr int NAIVE_TILE = 256;   // triangles per LDS tile

__global__ __launch_bounds__(BLOCK) void k_naive_mesh(SceneDev sc, const DevTriHot* __restrict__ tris, int num_tris,
                                                      PathBuf in, float4* hit_nt, int* hit_mat, float4* hit_uvd0,
                                                      float4* hit_uvd1, const int* n_ptr) {
    __shared__ float4 s_a[NAIVE_TILE];   // v0.xyz | e1.x
    __shared__ float4 s_b[NAIVE_TILE];   // e1.yz | e2.xy
    __shared__ float s_c[NAIVE_TILE];    // e2.z
    const int n = *n_ptr;
    if (blockIdx.x * BLOCK >= n) return;   // the whole block leaves: no barrier is left waiting
    const int tid = threadIdx.x;
    const int gid = blockIdx.x * BLOCK + tid;
    const bool live = gid < n;
    f3 ro = mk(0.f, 0.f, 0.f), rd = mk(0.f, 0.f, 0.f);
    float t_min = 0.0f;                    // a lane past n accepts nothing (t > 0 && t < 0)
    if (live) {
        const float4 a = in.A[gid], b = in.B[gid];
        ro = mk(a.x, a.y, a.z);
        rd = mk(b.x, b.y, b.z);
        const float tp = hit_nt[gid].w;    // the primitive winner's t, -1 on a miss
        t_min = tp > 0.0f ? tp : FLT_MAX_;
    }
    int best = -1;
    for (int base = 0; base < num_tris; base += NAIVE_TILE) {
        const int cnt = min(NAIVE_TILE, num_tris - base);
        __syncthreads();                   // the previous tile has been read by every wave
        for (int k = tid; k < cnt; k += BLOCK) {
            const DevTriHot th = tris[base + k];
            const f3 v0 = mk(th.a.x, th.a.y, th.a.z);
            const f3 e1 = mk(th.a.w, th.b.x, th.b.y) - v0;
            const f3 e2 = mk(th.b.z, th.b.w, th.c.x) - v0;
            s_a[k] = make_float4(v0.x, v0.y, v0.z, e1.x);
            s_b[k] = make_float4(e1.y, e1.z, e2.x, e2.y);
            s_c[k] = e2.z;
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const float4 a = s_a[i], b = s_b[i];
            const float c = s_c[i];
            float t, u, v;
            if (tri_test_e(ro, rd, mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, c), t, u, v) && t > 0.0f &&
                t < t_min) {
                t_min = t;
                best = base + i;
            }
        }
    }
    if (!live || best < 0) return;
    // the winner once more, for u and v (the same operations on the same bits), then the
    // production record: normal, material, uv and the triangle's own tangents
    const DevTriHot th = tris[best];
    float t = -1.0f, u = 0.0f, v = 0.0f;
    tri_test(ro, rd, mk(th.a.x, th.a.y, th.a.z), mk(th.a.w, th.b.x, th.b.y), mk(th.b.z, th.b.w, th.c.x), t, u, v);
    const Hit h = make_hit(sc, rd, FLT_MAX_, -1, mk(0.f, 0.f, 0.f), t, u, v, best, tris);
    hit_nt[gid] = make_float4(h.n.x, h.n.y, h.n.z, h.t);
    hit_mat[gid] = h.mat;
    if (hit_uvd0) {
        const HitAttr at = hit_attr(sc, h);
        hit_uvd0[gid] = make_float4(at.u, at.v, at.dpdu.x, at.dpdu.y);
        hit_uvd1[gid] = make_float4(at.dpdu.z, at.dpdv.x, at.dpdv.y, at.dpdv.z);
    }
}

}  // namespace ptd
