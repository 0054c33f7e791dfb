/*
 * pt_naive_mesh.h — the reference's NAIVE_MESH_LOADING mode (pathtrace.cu:365-393) as a run-time
 * option: after the primitive loop every triangle of the scene is tested in ARRAY order
 * (triangles[0 .. N)) with intersectTriangle, no BVH involved.  It is the reference's "no BVH" row
 * and a ground truth for any tree: a mesh scene renders without trusting a hierarchy.
 *
 * Semantics (pathtrace.cu:336-446).  A triangle hit is taken when t > 0 && t < t_min, so a
 * primitive wins a tie with a triangle and the first triangle in array order wins a tie between
 * triangles.  Normal (flat when a vertex normal is shorter than 1e-6, else interpolated and
 * normalised), uv and material follow pathtrace.cu:380-391; the reference's `vertices` array is
 * `triangles` flattened (scene.cpp:323-353), so pt_scene_view needs no new member and
 * PT_ABI_VERSION stays 3.  This is bvhMeshIntersectionTest on a one-leaf tree (one root node,
 * start 0, triCount N, identity triIndices, an enclosing box), bit for bit.
 *   One stated departure: the reference leaves dpdu / dpdv uninitialised on a naive hit; here the
 *   record carries the hit triangle's own dpdu / dpdv, as the BVH path does.
 *   With the mode on, the BVH test is skipped whatever pt_options.bvh says and whatever BVH arrays
 *   the scene view carries (the reference would run it second with strict `<` over the same
 *   triangles, where it can never replace the naive hit).  num_bvh_nodes == 0 with triangles
 *   present is valid; num_triangles == 0 is "no mesh".
 *
 * The mode runs on the STAGED pipeline of one unsharded device context: k_naive_mesh
 * (csrc/pt_naive_mesh_kernels.h) runs once per bounce over the live paths, after the
 * primitives-only intersection pass and before sort and shade.  pt_trace, pt_trace_frames,
 * pt_profile_frames, stream compaction and material sort work as on the staged pipeline;
 * pt_test_intersect honours the mode.
 *
 * pt_init with the mode on fails with PT_E_UNSUPPORTED when
 *   - pt_options.pipeline == PT_PIPELINE_FUSED was chosen explicitly,
 *   - pt_options.num_devices > 1,
 *   - pt_options.shard_mode != PT_SHARD_NONE.
 * "Explicitly" is told apart from the default like this: while the mode is on for the next
 * pt_init, pt_default_options (and so pt_init(scene, NULL)) yields PT_PIPELINE_STAGED.  A
 * PT_PIPELINE_FUSED that reaches pt_init was therefore written by the caller -- or stems from
 * options filled in before pt_set_naive_mesh(1); fetch them again after the call.
 * pt_gbuffer_capture returns PT_E_UNSUPPORTED in this mode (the denoiser's k_gbuffer has no naive
 * form).
 *
 * pt_profile_frames in this mode: pt_kernel_times.bvh_ms[b] holds the average duration of ONE
 * k_naive_mesh launch of bounce b; intersect_ms includes k_naive_mesh.
 */
#ifndef PT_NAIVE_MESH_H
#define PT_NAIVE_MESH_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Process-global, read by the NEXT pt_init, sticky until changed (enabled != 0: on).  The initial
 * value comes from the environment variable PT_NAIVE_MESH (1 = on; default off), read once at the
 * first use of either call, pt_default_options or pt_init.  Never fails; needs no device. */
int32_t pt_set_naive_mesh(int32_t enabled);

/* *next_init: what the next pt_init will use.  *active: what the live context was initialised
 * with (0 without a context).  Either pointer may be NULL.  Needs no device. */
int32_t pt_get_naive_mesh(int32_t* next_init, int32_t* active);

/* Tests and tools: triangles per LDS tile of k_naive_mesh. */
int32_t pt_debug_naive_mesh_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_NAIVE_MESH_H */
