// geom_bvh.h — the 4-wide hierarchy over the geoms' conservative world boxes (include/pt/pt_geom_bvh.h).
//
// Plain C++ beside scene_layout.cpp: no HIP, no environment, no global state.  Input: the DevGeom
// records whose box_lo / box_hi fill_geom_boxes has just computed.  Output: one DevGeomNode (a
// 128-byte line, csrc/pt_records.h) per node, node 0 the root, and the scalars the runtime sizes the
// traversal stack with.  Deterministic: the same boxes give the same bytes.
#pragma once

#include <vector>

#include "pt_records.h"

namespace pth {

struct GeomBvh {
    std::vector<ptd::DevGeomNode> nodes;   // empty: no tree was built
    int height = 0;                        // node levels on the longest root-to-leaf path
    int stack_entries = 0;                 // 3 * height + 1: what intersect_prims_bvh can push, asserted
                                           // by the builder's own walk over the tree
};

// Is every bound of every box finite and below the degenerate-transform sentinel (1e17)?  The
// traversal's monotonicity argument needs box * (1 / d) to stay finite for the clamped 1 / d.
bool geom_boxes_finite(const std::vector<ptd::DevGeom>& geoms);

// Builds the tree over geoms[0 .. n); n == 0 or a box that is not finite leaves `out` empty.
void build_geom_bvh(const std::vector<ptd::DevGeom>& geoms, GeomBvh& out);

}  // namespace pth
