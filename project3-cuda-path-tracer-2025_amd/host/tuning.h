// tuning.h — the runtime's tuning and test knobs, and the one place that reads them.
#pragma once

#include <cstddef>
#include <cstdint>

namespace pth {

// Tuning and test knobs (tools, A/B runs, tests).  Every one is read from the environment in ONE
// place, read_tuning(), when pt_init builds a context -- never on a hot call -- and none changes a
// result (the tests run each one against the oracle).  INTEGRATION.md §4 lists them.
struct Tuning {
    size_t bounce_lds_pad = 0, bvh_lds_pad = 0;   // PT_BOUNCE_LDS_PAD / PT_BVH_LDS_PAD: unused LDS (occupancy A/B)
    bool sections_skip_camera = false;              // PT_SECTIONS_SKIP_CAMERA: camera bounce out of the counters
    bool tail_off = false;                          // PT_TAIL=0: no k_tail launch
    bool tail_any_batch = false;                    // PT_TAIL_BATCH=1: k_tail for multi-frame passes too
    int tail_from = 0;                              // PT_TAIL_FROM: k_tail's first bounce (0: depth / 2)
    bool head_fuse = true;                          // PT_HEAD_FUSE=0: bounces 0 and 1 as two k_bounce launches
    int64_t auto_paths = 0;                         // PT_AUTO_PATHS: auto pass size in paths (0: AUTO_BATCH_PATHS)
    bool f1_graph = false;                          // PT_F1_GRAPH=1: single-frame passes through a graph
    bool multi_f1_direct = false;                   // PT_MULTI_F1_DIRECT=1: shards' single frames launched directly
    int bvh_tail_lanes = -1;                        // PT_BVH_TAIL_LANES (0..56; 0: no hand-over; -1: by tree size)
    int bvh_tail_chunks = 0;                        // PT_BVH_TAIL_CHUNKS: capped hand-over buffers (tests)
    int tail_refill = 16;                           // PT_BVH_TAIL_REFILL (1..64 idle lanes)
    int tail_trav_blocks = 224;                     // PT_BVH_TAIL_TRAV_BLOCKS per segment
    int tail_shade_blocks = 512;                    // PT_BVH_TAIL_SHADE_BLOCKS per segment (0: one per chunk)
    bool combine_force_staged = false;              // PT_COMBINE_FORCE_STAGED=1: peer shards via packed tiles
    bool bvh_tree_ref = false;                      // PT_BVH_TREE=ref: the reference's hierarchy, no SAH tree
    bool bvh_tree_info = false;                     // PT_BVH_TREE_INFO: print the traversal tree's shape
    int bvh_max_height = -1;                        // PT_BVH_MAX_HEIGHT: SAH tree height bound (0: none; -1: the
                                                    // height whose LDS stack still admits BVH_WAVES blocks per CU)
    int bvh_quad = 1;                               // PT_BVH_QUAD: the traversal kernels on 4-wide records (1) or on
                                                    // the pairs (0) (A/B: 262k -7.6 %, 1.0M -8.7 %, bunny -5.0 %,
                                                    // khaslana -1.9 %; profiles/r06_ab_four_wide.json)
    int bvh_stack_lds = 0;                          // PT_BVH_STACK_LDS: traversal stack entries kept in LDS by the split
                                                    // kernels, deeper ones spilled to a row per queue slot (0: all)
    int bvh_bfs_levels = 12;                        // PT_BVH_BFS_LEVELS: SAH pairs numbered breadth-first over
                                                    // this many levels, each subtree below in preorder
                                                    // (A/B: 262k -1.0 %, 1.0M -1.4 %, bunny +-0 vs all
                                                    // breadth-first; profiles/r06_ab_pair_numbering.json)
    int grid = -1;                                  // PT_GRID: 0 no candidate table, 1 also for small scenes
    bool speculate = true;                          // PT_SPECULATE=0: initial state of pt_set_speculation
    int band_copy = -1;                             // PT_BAND_COPY: several devices' host copy split over the
                                                    // shards (1), one copy from the first device (0), or
                                                    // split only when every shard has a device of its own (-1)
};
// the library's own: not among the symbols libptamd.so exports
__attribute__((visibility("hidden"))) Tuning read_tuning();

}  // namespace pth
