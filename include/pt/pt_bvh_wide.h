/*
 * pt_bvh_wide.h — an opt-in 8-wide quantised record layout for mesh trees that do not fit the L2.
 *
 * The two traversal kernels behind the split queue, k_bvh_bounce and k_bvh_tail_trav, walk the SAH
 * hierarchy over the reference's BVH leaves as 64-byte pairs or as 4-wide records (two levels per
 * 128-byte line).  On trees past an XCD's 4 MB L2 every miss moves a whole line, so the lever is
 * fewer lines per ray.  With this mode on, pt_init builds a third layout and those two kernels walk it:
 *
 *   DevWide8, 128 bytes, one line per node, up to eight children (csrc/pt_records.h):
 *     float origin[3]; uint8 exp[3]; uint8 count; uint8 qlo[3][8]; uint8 qhi[3][8];
 *     int32 ref[8]   (-1: no child, < num_records: a record, else leaf + num_records);
 *     uint32 cull[8] (the child's certified-cull constants, as the other layouts carry them).
 *   Child i's box decodes per axis to origin + float(q) * 2^(exp - 127).  The product is exact, so
 *   there is one rounding and no fused-multiply-add ambiguity.  The host picks q by floor / ceil,
 *   checks containment with that same float expression and bumps q (or raises exp) where rounding
 *   breaks it.  A record starts from a binary node's two children and replaces the inner child of
 *   largest surface area by its own two children until it holds eight or only leaves remain.
 *
 *   DevLeaf8, 192 bytes per leaf: the leaf's exact float box, its cull constants, its triangle count,
 *   then the nine float4 the other layouts' leaf records hold.  192 bytes start at 0 or 64 (mod 128)
 *   and touch exactly two lines; the 144-byte records of the other layouts touch up to three.
 *
 * Why it stays exact.  Any hierarchy above the reference's leaves is exact if its inner boxes contain
 * their leaves' boxes and the leaf is decided by the reference's exact box test.  A
 * decoded box that contains the true child box passes whenever the true box passes: extra visits,
 * never a missed leaf.  Its entry distance is no larger than the true one, so the certified cull
 * threshold computed from it is no larger: a cull can only be lost.  A quantised box cannot decide
 * a leaf, so the leaf record carries the exact box and the kernels run the exact decision and the
 * certified cull on it before they touch a triangle.  Ties go to the smaller triangle slot, so the
 * visiting order is free.  Images, hit records, live counts and segments_total are bit-identical
 * with the mode on or off.
 *
 * The mode is a speed hint, not a semantic switch: where it cannot apply pt_init succeeds, the tracer
 * runs as without it and pt_get_bvh_wide reports active = 0.  It applies only to one unsharded
 * device context on the fused pipeline with the split queue live, and a SAH tree of at least
 * min_refs refs (inner nodes + leaves).  It is inactive for
 *   - the staged pipeline, and kernel variants without the split (VAR_BVH_SPLIT and what it needs),
 *   - the naive mesh mode, an active geom BVH (pt/pt_geom_bvh.h), more than 64 geoms,
 *   - pt_options.num_devices > 1 or shard_mode != PT_SHARD_NONE,
 *   - trees below min_refs, PT_BVH_TREE=ref, a tree the pair layout cannot hold,
 *   - a box that cannot be encoded (a non-finite coordinate, no exponent that covers the extent),
 *   - a traversal that could need more than 96 stack entries (what the hand-over can save).
 * k_bounce's own traversals, k_intersect, the g-buffer kernels and the root test keep the pairs.
 * When the mode is active the 4-wide records are not uploaded.  Device memory: 128 B per record
 * (about a third of the leaf count with the largest-area collapse) plus 192 B per leaf, beside the
 * pairs and the 144-byte leaf records the other kernels keep.
 *
 * The traversal can push up to seven entries per record.  The host computes the exact need (the
 * maximum over root-to-node paths of the sum of children - 1, plus 1).  By default the LDS part of
 * the stack stays what the pairs would take and the rest goes to the spill rows
 * (PT_BVH_STACK_LDS overrides, as for the other layouts).
 *
 * Off by default, and as built NOT recommended at any size: tools/bvh_wide_probe.py
 * (profiles/bvh_wide_probe.json, DESIGN.md §4 "8-wide quantised records"; 800^2, depth 8, mode off = the
 * 4-wide records against mode on, interleaved) measured it slower on the trees past the L2 it was meant
 * for (262k triangles: 0.387 -> 0.534 ms / frame; 1.0M: 0.419 -> 0.601) and on the L2-resident ones (bunny
 * 0.374 -> 0.523, khaslana 0.304 -> 0.379).  The records hold 4.1 children on average with the
 * largest-area collapse, and every leaf costs its own two-line fetch before the exact box decision.
 * It is kept as a bit-exact base for the next layouts, behind the switch.
 */
#ifndef PT_BVH_WIDE_H
#define PT_BVH_WIDE_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Process-global, read by the NEXT pt_init, sticky until changed.  enabled != 0: on for trees of at
 * least min_refs refs; min_refs <= 0: the default, 65,536 (the size from which the hand-over already
 * changes its defaults).  The initial value comes from the environment variable PT_BVH_WIDE, read
 * once at the first use of either call or of pt_init: unset or 0 = off, 1 = on with the default
 * threshold, N > 1 = on with min_refs = N.  Never fails; needs no device. */
int32_t pt_set_bvh_wide(int32_t enabled, int32_t min_refs);

/* *next_enabled, *next_min: what the next pt_init will use (next_min is the resolved threshold).
 * *active: 1 only if the live context's traversal kernels really walk the 8-wide records (0 without a
 * context).  Any pointer may be NULL.  Needs no device. */
int32_t pt_get_bvh_wide(int32_t* next_enabled, int32_t* next_min, int32_t* active);

/* Tests and tools: the live context's layout -- records, height in record levels plus the leaf
 * level, stack entries a traversal can need, bytes per leaf record.  Zeros when the mode is not
 * active.  Any pointer may be NULL. */
int32_t pt_debug_bvh_wide_info(int32_t* num_records, int32_t* height, int32_t* stack_entries, int32_t* leaf_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PT_BVH_WIDE_H */
