/*
 * pt_geom_bvh.h — primitive intersection through a 4-wide hierarchy over the geoms.
 *
 * Every fast path for cubes and spheres stops at LDS_GEOMS = 64 geoms (the LDS geom table, the
 * 64-bit candidate masks, k_head, k_tail).  Beyond that the flat loop of intersect_scene runs one
 * conservative box pre-test per geom per ray, with records from global memory: cost linear in the
 * geom count.  With this mode on, pt_init builds a hierarchy over the geoms' conservative world
 * boxes (host/geom_bvh.cpp; one 128-byte record of up to four children per node) and the bounce
 * kernels find the primitive winner by a per-lane, near-first, t-culled traversal of it
 * (intersect_prims_bvh, csrc/pt_geom_bvh_kernels.h).
 *
 * Semantics.  The primitive winner is the geom of smallest exact t > 0; among equal t the smallest
 * geom index wins.  That is what the flat loop's `t > 0 && t_min > t` in array order yields, and
 * the rule intersect_scene_q states for exact tests run out of index order.  The traversal only
 * decides WHICH exact tests run: a box test never decides a result, and the box tests are the flat
 * loop's own pre-test arithmetic, so every image, hit record and live count is bit-identical with
 * the mode on or off (the argument: csrc/pt_geom_bvh_kernels.h).  The mesh part of a scene is
 * untouched: the triangles' BVH is traversed afterwards with the primitive winner, as before.
 *
 * The mode is a speed hint, not a semantic switch: where it cannot apply pt_init succeeds, the flat
 * path runs and pt_get_geom_bvh reports active = 0.  It cannot apply when
 *   - the scene has fewer than min_geoms geoms,
 *   - a geom's conservative box is not finite (a degenerate transform),
 *   - the fused pipeline was asked for a kernel variant that has no geom-BVH instantiation (they
 *     exist for the default variant, its texture-free and its material-grouping forms),
 *   - the naive mesh mode is on,
 *   - pt_options.num_devices > 1 or shard_mode != PT_SHARD_NONE,
 *   - the traversal stack (3 x tree height + 1 entries per lane) does not fit in the block's LDS
 *     beside the mesh traversal's stack and the material-grouping exchange.
 * Fused pipeline: k_bounce takes no LDS geom table (also below 65 geoms when min_geoms was
 * lowered), k_head / k_tail are not used and mesh rays are not split off into k_bvh_bounce -- as is
 * already the case above 64 geoms.  Staged pipeline: k_intersect_gbvh runs in place of
 * k_intersect; pt_test_intersect honours the mode.  The denoiser's captures (k_gbuffer and the
 * through-capture) keep the flat loop: they give the same records, and a capture runs once per
 * camera.
 *
 * Off by default.  Recommended min_geoms: 65, the default threshold (LDS_GEOMS + 1, the first count
 * the LDS paths cannot serve).  tools/geom_bvh_probe.py (profiles/geom_bvh_probe.json, DESIGN §4
 * "Geom BVH") timed mode off against mode on at 800^2, depth 8: the hierarchy wins at every count
 * measured, from 72 geoms (fused 1.25x, staged 1.04x) to 4000 (fused 10x, staged 4.3x).  Below 65
 * geoms nothing was measured; there the mode would replace the LDS fast paths, not the flat loop.
 */
#ifndef PT_GEOM_BVH_H
#define PT_GEOM_BVH_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Process-global, read by the NEXT pt_init, sticky until changed.  enabled != 0: on for scenes of
 * at least min_geoms geoms; min_geoms <= 0: the default, LDS_GEOMS + 1 = 65.  The initial value
 * comes from the environment variable PT_GEOM_BVH, read once at the first use of either call or
 * of pt_init: unset or 0 = off, 1 = on with the default threshold, N > 1 = on with min_geoms = N.
 * Never fails; needs no device. */
int32_t pt_set_geom_bvh(int32_t enabled, int32_t min_geoms);

/* *next_enabled, *next_min: what the next pt_init will use (next_min is the resolved threshold).
 * *active: 1 only if the live context really launches the geom-BVH kernels (0 without a context).
 * Any pointer may be NULL.  Needs no device. */
int32_t pt_get_geom_bvh(int32_t* next_enabled, int32_t* next_min, int32_t* active);

/* Tests and tools: the live context's tree -- node records, height in node levels, stack entries
 * per lane.  Zeros when the mode is not active.  Any pointer may be NULL. */
int32_t pt_debug_geom_bvh_info(int32_t* num_nodes, int32_t* height, int32_t* stack_entries);

#ifdef __cplusplus
}
#endif
#endif /* PT_GEOM_BVH_H */
