/*
 * pt_trav_build.h — the SAH traversal hierarchy built on the device, bit-identical to the host's.
 *
 * Everything the traversal kernels walk (pairs, 4-wide records, 8-wide records) is derived from one
 * binary tree: the binned-SAH hierarchy over the reference's BVH leaves (host/trav_tree.h,
 * pth::build_sah_tree).  On the host that build is serial and, for a mesh of a million triangles,
 * the longest stage of pt_init.  With this mode on, pt_init builds the same tree on the device
 * (csrc/pt_trav_build.hip) and hands the host layout code the same records.
 *
 * Why the trees are the same bits.  Every reduction in the algorithm is order-free and exact: min /
 * max of floats and doubles, integer bin counts.  The device kernels use the host's expressions,
 * operation for operation and with contraction off: the centroid 0.5 * ((double)lo + (double)hi),
 * recomputed wherever it is needed; the bin min(31, (int)((cen - cl) / ext * 32)); the area
 * x*y + y*z + z*x in double; the cost l.area()*lc + r.area()*rc; the first strict minimum in the
 * order axis 0..2, split 0..30; index-order halving when every centroid is equal; and, where a split
 * would leave a child no room below max_height, the median split on the same axis ordered by
 * (centroid, leaf id).  The device decides the tree's SHAPE (split search, partitions, median
 * selection).  The boxes and cull sizes are then folded bottom-up and the nodes numbered by the
 * host's own code (pth::finish_sah_tree, O(n)): a parent's box is min / max over its two children
 * with ties to the left child, which decides the sign of a zero bound, and an order-free device
 * reduction cannot reproduce that.
 *
 * Known divergence.  After a median split the host's std::nth_element leaves an unspecified order
 * inside each half; the device keeps each half in its previous relative order.  The order inside a
 * segment is read only by the index-order halving, so the trees can differ only if a segment below
 * a median split has all centroids equal.
 *
 * The mode is a speed hint, not a semantic switch: images, hit records and segments_total do not
 * depend on it.  Where the device build cannot run (no device, an allocation fails) pt_init builds on
 * the host, succeeds, and pt_get_trav_build reports active = 0.  PT_BVH_TREE=ref, the naive mesh mode
 * and scenes without a mesh never build the tree at all.
 */
#ifndef PT_TRAV_BUILD_H
#define PT_TRAV_BUILD_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The device build's two sizes (tests name them): a segment of more than PT_TRAV_BUILD_SUBTREE leaves is
 * split level by level, cut into pieces of PT_TRAV_BUILD_PIECE leaves, one workgroup each; a segment
 * of at most PT_TRAV_BUILD_SUBTREE leaves is finished, with its whole subtree, in LDS by one launch. */
#define PT_TRAV_BUILD_PIECE 2048
#define PT_TRAV_BUILD_SUBTREE 1024

/* One inner node of the tree: two children, each an inner node (leaf = 0, ref = its index) or a
 * leaf (leaf = 1, ref = the leaf's id).  72 bytes. */
typedef struct pt_trav_child {
    float lo[3], hi[3];
    int32_t ref;
    int32_t leaf;
    float s;
} pt_trav_child;
typedef struct pt_trav_inner {
    pt_trav_child c[2];
} pt_trav_inner;

/* Process-global, read by the NEXT pt_init, sticky until changed.  on_device != 0: trees of at least
 * min_leaves leaves are built on the device; min_leaves <= 0: the default, 32,768 (the smallest power of two from which
 * tools/trav_build_probe.py measured the device build not slower; it has a floor of about 11 ms of
 * allocations, copies and launches: profiles/trav_build_probe.json).  The initial value
 * comes from the environment variable PT_TRAV_BUILD, read once at the first use of either call or of
 * pt_init: unset or 0 = host, 1 = device with the default threshold, N > 1 = device from N leaves.
 * Never fails; needs no device. */
int32_t pt_set_trav_build(int32_t on_device, int32_t min_leaves);

/* *next_on_device, *next_min: what the next pt_init will use (next_min is the resolved threshold).
 * *active: 1 only if the live context's hierarchy really came from the device build (0 without a
 * context, for a tree below the threshold, or after a fall-back to the host).  Any pointer may be
 * NULL.  Needs no device. */
int32_t pt_get_trav_build(int32_t* next_on_device, int32_t* next_min, int32_t* active);

/* The tree over caller data: n leaf boxes (leaf_lo / leaf_hi: 3 floats each) and cull sizes leaf_s,
 * numbered breadth-first over the top bfs_levels levels and in preorder below, at most max_height
 * levels high (raised to 1 + ceil(log2 n)).  where = 0: the host build; where = 1: the device build
 * on the current HIP device (PT_E_NODEVICE without one).  out: capacity cap >= n - 1 nodes;
 * *num_inner and *height receive the counts.  PT_E_INVALID where the host function returns false:
 * n < 2, a non-finite coordinate, lo > hi (and for a NULL pointer or a short `out`). */
int32_t pt_trav_build(const float* leaf_lo, const float* leaf_hi, const float* leaf_s, int32_t n, int32_t bfs_levels,
                      int32_t max_height, int32_t where, pt_trav_inner* out, int32_t cap, int32_t* num_inner,
                      int32_t* height);

/* The message of the last pt_trav_build failure on this thread's process (never NULL). */
const char* pt_trav_build_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_TRAV_BUILD_H */
