// tuning.cpp — read_tuning(): every PT_* tuning knob, from the environment, clamped to its range.
#include "tuning.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace pth {

Tuning read_tuning() {
    auto num = [](const char* name, long dflt) {
        const char* e = getenv(name);
        return e && *e ? atol(e) : dflt;
    };
    Tuning t;
    t.bounce_lds_pad = (size_t)std::max(0L, num("PT_BOUNCE_LDS_PAD", 0));
    t.bvh_lds_pad = (size_t)std::max(0L, num("PT_BVH_LDS_PAD", 0));
    t.sections_skip_camera = getenv("PT_SECTIONS_SKIP_CAMERA") != nullptr;
    t.tail_off = num("PT_TAIL", 1) == 0;
    t.tail_any_batch = num("PT_TAIL_BATCH", 0) != 0;
    t.tail_from = (int)num("PT_TAIL_FROM", 0);
    t.head_fuse = num("PT_HEAD_FUSE", 1) != 0;
    t.auto_paths = num("PT_AUTO_PATHS", 0);
    t.f1_graph = num("PT_F1_GRAPH", 0) != 0;
    t.multi_f1_direct = num("PT_MULTI_F1_DIRECT", 0) != 0;
    t.bvh_tail_lanes = (int)std::min(56L, std::max(-1L, num("PT_BVH_TAIL_LANES", -1)));
    t.bvh_tail_chunks = (int)std::max(0L, num("PT_BVH_TAIL_CHUNKS", 0));
    t.tail_refill = (int)std::max(1L, std::min(64L, num("PT_BVH_TAIL_REFILL", 16)));
    t.tail_trav_blocks = (int)std::max(1L, num("PT_BVH_TAIL_TRAV_BLOCKS", 224));
    t.tail_shade_blocks = (int)std::max(0L, num("PT_BVH_TAIL_SHADE_BLOCKS", 512));
    t.combine_force_staged = num("PT_COMBINE_FORCE_STAGED", 0) != 0;
    const char* tree = getenv("PT_BVH_TREE");
    t.bvh_tree_ref = tree && strcmp(tree, "ref") == 0;
    t.bvh_tree_info = getenv("PT_BVH_TREE_INFO") != nullptr;
    t.bvh_bfs_levels = (int)std::max(0L, num("PT_BVH_BFS_LEVELS", 12));
    t.bvh_max_height = (int)std::max(-1L, num("PT_BVH_MAX_HEIGHT", -1));
    t.bvh_quad = num("PT_BVH_QUAD", 1) != 0 ? 1 : 0;
    t.bvh_stack_lds = (int)std::max(0L, num("PT_BVH_STACK_LDS", 0));
    t.grid = (int)num("PT_GRID", -1);
    t.speculate = num("PT_SPECULATE", 1) != 0;
    t.band_copy = (int)std::max(-1L, std::min(1L, num("PT_BAND_COPY", -1)));
    return t;
}

}  // namespace pth
