// scene_layout.h — the byte images of the device scene buffers, built on the host.
//
// pt_init has two halves: this one turns a pt_scene_view into the records the kernels read
// (csrc/pt_records.h) and the scalars that go with them, touching neither HIP nor any global state;
// the runtime (csrc/pt_runtime.hip, init_one) allocates a device buffer for each vector filled here
// and uploads it.  Every exactness argument of the BVH fast path rests on this code and it indexes
// caller-supplied trees, so it is plain C++: linked into the library and, under the sanitizers,
// into host/ingest_check.cpp.
#pragma once

#include <string>
#include <vector>

#include "pt/pathtrace_abi.h"
#include "pt_records.h"

namespace pth {

// What the layout depends on besides the scene: pt_options fields, the PT_* tuning knobs
// (the runtime reads the environment, this code never does) and the SAH
// height bound the runtime resolves from its kernels' LDS budget.  The defaults are pt_init's.
struct LayoutParams {
    bool bvh = true;                    // pt_options.bvh
    int variant = ptd::VAR_DEFAULT;     // pt_options.variant
    bool naive = false;                 // NAIVE_MESH_LOADING mode (pt/pt_naive_mesh.h)
    bool bvh_tree_ref = false;          // PT_BVH_TREE=ref: the reference's hierarchy, no SAH tree
    bool bvh_tree_info = false;         // PT_BVH_TREE_INFO: print the traversal tree's shape (stderr)
    int bvh_bfs_levels = 12;            // PT_BVH_BFS_LEVELS
    int bvh_quad = 1;                   // PT_BVH_QUAD
    int grid = -1;                      // PT_GRID: 0 no candidate table, 1 also for small scenes
    int sah_max_height = 21;            // SAH tree height bound, resolved (1 << 30: none)
};

struct SceneLayout {
    std::vector<ptd::DevGeom> geoms;
    std::vector<ptd::DevCull> culls;        // padded to a multiple of CULL_GROUP
    std::vector<ptd::DevMaterial> mats;     // at least one
    bool no_tex = true;                     // no material samples a texture or bump map
    // the pre-test's candidate table (empty: flat pre-test) and its cells' origin and scale
    std::vector<unsigned long long> grid;
    float grid_lo[3] = {0.f, 0.f, 0.f}, grid_inv[3] = {0.f, 0.f, 0.f};
    // BVH (has_bvh: the reference would traverse it); everything below is empty / 0 without one
    bool has_bvh = false;
    int variant = 0;                        // params.variant, minus VAR_BVH_FAST | VAR_BVH_SPLIT for a
                                            // tree the near-first traversals cannot walk
    std::vector<ptd::DevNode> nodes;
    std::vector<float4> node_aux;
    std::vector<ptd::DevTriHot> hot;
    std::vector<ptd::DevTriCold> cold;      // also filled in the naive mesh mode
    std::vector<ptd::DevPair> pairs;        // VAR_BVH_FAST layout (empty: tree not representable)
    std::vector<float4> quads;              // its 4-wide form (8 float4 per record; empty: not built)
    std::vector<ptd::DevTriHot> hot4;
    std::vector<float4> leaf9;
    std::vector<ptd::DevTriHot> naive_hot;  // naive mesh mode: positions in triangle order
    int stack_depth = 0;                    // LDS stack entries per lane, all traversals
    int pair_depth = 0;                     // entries the pair traversal needs: height of its hierarchy + 1
    int quad_stack = 0;                     // stack entries the 4-wide traversal can need
    int root_ref = 0, pair_count = 0, ref_shift = 16;
    float4 root_lo{}, root_hi{};            // root box (hi.w: root cull size)
    double cull_extent = 1.0;
};

// PT_OK and a filled `out`, or an error code with its message in `err` (`out` is then unspecified).
int32_t build_scene_layout(const pt_scene_view& s, const LayoutParams& p, SceneLayout& out, std::string& err);

}  // namespace pth
