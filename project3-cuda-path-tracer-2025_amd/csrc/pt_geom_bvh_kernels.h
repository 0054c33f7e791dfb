// pt_geom_bvh_kernels.h — primitive intersection through the 4-wide hierarchy over the geoms
// (include/pt/pt_geom_bvh.h; the tree: host/geom_bvh.cpp, the record: DevGeomNode in pt_records.h).
//
//   intersect_prims_bvh   the per-lane traversal: the primitive winner (t_min, win, seed)
//   intersect_scene_gbvh  ... + the mesh part, as intersect_scene
//   k_intersect_gbvh      the staged pipeline's intersection stage (in place of k_intersect)
//   k_bounce<.., VAR | VAR_GEOM_BVH>  (pt_pass_kernels.h) calls intersect_scene_gbvh
//
// Included by pt_runtime.hip alone, at global scope after its `using namespace ptd`, before
// pt_pass_kernels.h.
//
// Why the result is the flat loop's, bit for bit.  intersect_scene runs, per geom in array order,
// cull_geom (a conservative pre-test that is true only when the exact test is CERTAIN not to
// change (t_min, win)) and then geom_test with `t > 0 && t_min > t`: the winner is the geom of
// smallest exact t > 0, the smallest index among equal t.  Here the exact tests run in another
// order with the rule `t > 0 && (t < t_min || (t == t_min && i < win))`, which names the same
// winner whatever the order (intersect_scene_q's NEAR_FIRST rule), provided no geom is skipped that
// could have won or tied.  A geom is skipped in two ways:
//  1. at its leaf, by cull_geom on the geom's own box against the lane's current t_min -- the
//     flat loop's own test, against a t_min that is never below the final one;
//  2. with a whole subtree, when a node's slot box fails the SAME arithmetic (slab4 below is
//     cull_geom's, expression by expression: fma slabs on the CullRay, the -1e-2 floor, the
//     `t1 >= t0` miss rule, the "certainly farther" cut t0 > 0 && t0 rdlen (1 - 1e-5) - 1e-4 > t_min).
//     A slot box contains every box below it exactly (float min / max unions, no rounding), and
//     every operation of the test is monotone in the box bounds: a correctly rounded fma(b, id,
//     -rid) is non-decreasing in b for id >= 0 and non-increasing for id < 0, so per axis the near
//     value min(a, b) of a contained box is >= the container's and the far value max(a, b) is <=;
//     max / min over the axes and the floor keep the order, so t0(inner) >= t0(outer) and
//     t1(inner) <= t1(outer).  Hence !(t1 >= t0) for the outer box implies it for every box below,
//     and with rdlen >= 0 the products and the subtraction of the cut are monotone in t0 too: an
//     outer box that is certainly farther than t_min makes every box below certainly farther,
//     now and later (t_min only shrinks).  A NaN enters a slab value only through the ray (rid, or
//     0 x inf cannot arise: the mode requires every bound below 1e17 in magnitude and 1 / d is
//     clamped to 1e20, so bound x id is finite); it then does so on that axis for EVERY box, outer
//     and inner alike, where min / max drop it for both, and the remaining axes stay ordered.  A NaN
//     rdlen makes the cut false for the outer box, which then skips nothing.
//     So whatever the flat loop's pre-test would have kept below a failing node, it would have
//     skipped too: the exact tests run here are a subset of those the flat loop could run, and the
//     skipped ones cannot win or tie.
// The min / max slabs do not see a box's orientation, so an empty slot's inverted box would pass
// them: it is recognised by lo.x > hi.x, folded into the pass mask without a branch.
//
// Traversal: the root record is popped from the lane's LDS stack (stack[depth * BLOCK], the mesh
// traversals' layout).  A record's seven float4 are loaded (dwordx4) before any arithmetic; the
// four slots are tested, the survivors ordered by entry distance t0 with a fixed five-exchange
// network, the nearest is visited next without touching the stack and the others are pushed
// farthest first.  At most three pushes per level: 3 x height + 1 entries (the builder asserts it).
// A popped node is not re-tested against the t_min of the time (its box is not on the stack); its
// children are.  A leaf child runs its exact test at once (the immediate form; a form that parks a
// pending leaf per lane and runs the exact tests when a ballot shows enough lanes waiting has not
// been built).
//
// The tree's pointer and scalars reach the kernels through c_gbvh, not through SceneDev: the
// existing kernels' arguments, and with them their code objects, stay what they were.  One context
// per device uses it (the mode is inactive for multi-device contexts).
#pragma once

#include "pt_kernels.h"

namespace ptd {

struct GeomBvhDev {
    const float4* nodes;     // DevGeomNode records as 8 float4 each; node 0 is the root
    int num_nodes, height;
    int stack_entries;       // LDS stack entries per lane
};
__constant__ GeomBvhDev c_gbvh;

// cull_geom for the four slots of a record: key[i] = entry distance t0 of a slot the ray may hit
// nearer than t_min (clamped to FLT_MAX so that it stays below the failure mark), +inf otherwise
PT_DEV void slab4(const v4f* q, const CullRay& c, float t_min, float key[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a0 = __builtin_fmaf(q[0][i], c.id.x, -c.rid.x), b0 = __builtin_fmaf(q[3][i], c.id.x, -c.rid.x);
        const float a1 = __builtin_fmaf(q[1][i], c.id.y, -c.rid.y), b1 = __builtin_fmaf(q[4][i], c.id.y, -c.rid.y);
        const float a2 = __builtin_fmaf(q[2][i], c.id.z, -c.rid.z), b2 = __builtin_fmaf(q[5][i], c.id.z, -c.rid.z);
        const float t0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a0, b0), __builtin_fminf(a1, b1)),
                                         __builtin_fmaxf(__builtin_fminf(a2, b2), -1e-2f));
        const float t1 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a0, b0), __builtin_fmaxf(a1, b1)),
                                         __builtin_fmaxf(a2, b2));
        const bool farther = t0 > 0.0f && t0 * c.rdlen * (1.0f - 1e-5f) - 1e-4f > t_min;
        const bool pass = (q[0][i] <= q[3][i]) & (t1 >= t0) & !farther;
        key[i] = pass ? __builtin_fminf(t0, FLT_MAX_) : __builtin_inff();
    }
}

// the primitive winner of one ray: exact t (FLT_MAX: none), geom index (-1), normal seed
PT_DEV void intersect_prims_bvh(const SceneDev& sc, const GeomBvhDev& gb, f3 ro, f3 rd, int* stack, float& t_min,
                                int& win, f3& seed) {
    t_min = FLT_MAX_;
    win = -1;
    seed = mk(0.f, 0.f, 0.f);
    const CullRay cr = cull_ray(ro, rd);
    const v4f* N = reinterpret_cast<const v4f*>(gb.nodes);
    int sp = 1;
    stack[0] = 0;
    while (sp > 0) {
        int cur = stack[(--sp) * BLOCK];
        for (;;) {
            if (cur < 0) {   // a leaf: the flat loop's pre-test on the geom's own box, then the exact test
                const int i = ~cur;
                const DevGeom& g = sc.geoms[i];
                if (!cull_geom(g, cr, t_min)) {
                    f3 s;
                    const float t = geom_test(hot(g), ro, rd, s);
                    if (t > 0.0f && (t < t_min || (t == t_min && i < win))) {
                        t_min = t;
                        win = i;
                        seed = s;
                    }
                }
                break;
            }
            // a node: its four slots, nearest first
            const v4f* Q = N + 8 * (size_t)cur;
            v4f q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) q[k] = Q[k];
            float key[4];
            int ref[4];
            slab4(q, cr, t_min, key);
#pragma unroll
            for (int i = 0; i < 4; ++i) ref[i] = __float_as_int(q[6][i]);
            auto cx = [&](int a, int b) {
                if (key[b] < key[a]) {
                    const float tk = key[a]; key[a] = key[b]; key[b] = tk;
                    const int tr = ref[a]; ref[a] = ref[b]; ref[b] = tr;
                }
            };
            cx(0, 1); cx(2, 3); cx(0, 2); cx(1, 3); cx(1, 2);
            if (!(key[0] < __builtin_inff())) break;   // no slot passes: pop
            // (sp < stack_entries always holds, by the builder's bound; the test keeps a wrong bound
            // from writing outside the block's LDS)
#pragma unroll
            for (int i = 3; i >= 1; --i)
                if (key[i] < __builtin_inff() && sp < gb.stack_entries) stack[(sp++) * BLOCK] = ref[i];
            cur = ref[0];
        }
    }
}

// computeIntersections for one ray, as intersect_scene: the primitive winner from the hierarchy,
// then the mesh (finish_hit, unchanged).  `stack`: the mesh traversal's column, `gstack`: this one's.
template <bool HAS_BVH, bool BVH_FAST>
PT_DEV Hit intersect_scene_gbvh(const SceneDev& sc, const GeomBvhDev& gb, f3 ro, f3 rd, int* stack, int* gstack) {
    float t_min;
    int win;
    f3 seed;
    intersect_prims_bvh(sc, gb, ro, rd, gstack, t_min, win, seed);
    return finish_hit<HAS_BVH, BVH_FAST>(sc, ro, rd, stack, t_min, win, seed);
}

}  // namespace ptd

// The staged pipeline's intersection stage with the hierarchy: k_intersect's records, bit for bit.
// Dynamic LDS: [HAS_BVH: mesh stack, sc.stack_depth x BLOCK ints][c_gbvh.stack_entries x BLOCK ints]
template <bool HAS_BVH, bool BVH_FAST>
__global__ __launch_bounds__(BLOCK) void k_intersect_gbvh(SceneDev sc, PathBuf in, float4* __restrict__ nt,
                                                          int* __restrict__ mat, float4* __restrict__ uvd0,
                                                          float4* __restrict__ uvd1, const int* n_ptr) {
    extern __shared__ int s_gbvh_stack[];
    const int n = *n_ptr;
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= n) return;
    const GeomBvhDev gb = c_gbvh;
    int* s_mesh = s_gbvh_stack + threadIdx.x;
    int* s_geom = s_mesh + (HAS_BVH ? sc.stack_depth * BLOCK : 0);
    const float4 a = in.A[gid], b = in.B[gid];
    const Hit h = intersect_scene_gbvh<HAS_BVH, BVH_FAST>(sc, gb, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), s_mesh, s_geom);
    nt[gid] = make_float4(h.n.x, h.n.y, h.n.z, h.t);
    mat[gid] = h.mat;
    if (uvd0) {
        const HitAttr at = hit_attr(sc, h);
        uvd0[gid] = make_float4(at.u, at.v, at.dpdu.x, at.dpdu.y);
        uvd1[gid] = make_float4(at.dpdu.z, at.dpdv.x, at.dpdv.y, at.dpdv.z);
    }
}
