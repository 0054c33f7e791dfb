// geom_bvh.cpp — see geom_bvh.h.
//
//   1. a binary tree over the geoms by the surface-area heuristic, one geom per leaf: for every axis
//      the set is ordered by (box centre, index) and every split position is priced
//      area(left) * n_left + area(right) * n_right in double precision; the cheapest wins, the first
//      one found on a tie.  A set whose centres all coincide (duplicated geoms) is cut at the median
//      of its indices.  Both sides of every cut are non-empty, so the recursion ends.
//   2. the collapse to four children: a node starts from its two binary children and, while it has
//      fewer than four, replaces its inner child of largest area by that child's own two.
//   3. records in breadth-first order, node 0 the root.  A slot's box is the float min / max union
//      of the boxes below it: it contains every one of them exactly, with no rounding.
#include "geom_bvh.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>

namespace pth {

using ptd::DevGeom;
using ptd::DevGeomNode;

namespace {

struct Bin {              // a node of the binary tree
    int left = -1, right = -1;
    int geom = -1;        // >= 0: a leaf
    float lo[3], hi[3];
    double area = 0.0;
};

double box_area(const float* lo, const float* hi) {
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return 2.0 * (x * y + y * z + z * x);
}

struct Builder {
    const std::vector<DevGeom>& g;
    std::vector<Bin> bin;

    double centre(int i, int a) const { return 0.5 * ((double)g[i].box_lo[a] + (double)g[i].box_hi[a]); }

    int leaf(int i) {
        Bin b;
        b.geom = i;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = g[i].box_lo[a];
            b.hi[a] = g[i].box_hi[a];
        }
        b.area = box_area(b.lo, b.hi);
        bin.push_back(b);
        return (int)bin.size() - 1;
    }

    // idx[0 .. n): the set; returns its binary node
    int build(int* idx, int n) {
        if (n == 1) return leaf(idx[0]);
        bool spread = false;
        for (int a = 0; a < 3 && !spread; ++a)
            for (int k = 1; k < n && !spread; ++k) spread = centre(idx[k], a) != centre(idx[0], a);
        int cut = n / 2;
        std::vector<int> best(idx, idx + n);
        std::sort(best.begin(), best.end());   // coincident centres: the median of the indices
        if (spread) {
            double best_cost = std::numeric_limits<double>::infinity();
            std::vector<int> ord(n);
            std::vector<double> right_area(n);
            for (int a = 0; a < 3; ++a) {
                std::copy(idx, idx + n, ord.begin());
                std::sort(ord.begin(), ord.end(), [&](int x, int y) {
                    const double cx = centre(x, a), cy = centre(y, a);
                    return cx < cy || (cx == cy && x < y);
                });
                float lo[3], hi[3];
                auto reset = [&]() {
                    for (int r = 0; r < 3; ++r) {
                        lo[r] = std::numeric_limits<float>::infinity();
                        hi[r] = -std::numeric_limits<float>::infinity();
                    }
                };
                auto grow = [&](int i) {
                    for (int r = 0; r < 3; ++r) {
                        lo[r] = std::min(lo[r], g[i].box_lo[r]);
                        hi[r] = std::max(hi[r], g[i].box_hi[r]);
                    }
                };
                reset();
                for (int k = n - 1; k >= 1; --k) {   // right_area[k]: the box of ord[k .. n)
                    grow(ord[k]);
                    right_area[k] = box_area(lo, hi);
                }
                reset();
                for (int k = 1; k < n; ++k) {        // left = ord[0 .. k)
                    grow(ord[k - 1]);
                    const double cost = box_area(lo, hi) * k + right_area[k] * (n - k);
                    if (cost < best_cost) {
                        best_cost = cost;
                        cut = k;
                        best = ord;
                    }
                }
            }
        }
        std::copy(best.begin(), best.end(), idx);
        const int l = build(idx, cut), r = build(idx + cut, n - cut);
        Bin b;
        b.left = l;
        b.right = r;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = std::min(bin[l].lo[a], bin[r].lo[a]);
            b.hi[a] = std::max(bin[l].hi[a], bin[r].hi[a]);
        }
        b.area = box_area(b.lo, b.hi);
        bin.push_back(b);
        return (int)bin.size() - 1;
    }
};

// the most entries intersect_prims_bvh can have on its stack while it works below node k: it pushes
// every child but the one it goes on with, and the deepest subtree may be the one it goes on with
int walk_need(const std::vector<DevGeomNode>& nodes, int k, int level, int& height) {
    height = std::max(height, level);
    int children = 0, below = 0;
    for (int c = 0; c < 4; ++c) {
        if (nodes[k].lo[0][c] > nodes[k].hi[0][c]) continue;   // empty slot
        ++children;
        if (nodes[k].ref[c] >= 0) below = std::max(below, walk_need(nodes, nodes[k].ref[c], level + 1, height));
    }
    return std::max(0, children - 1) + below;
}

}  // namespace

bool geom_boxes_finite(const std::vector<DevGeom>& geoms) {
    for (const DevGeom& d : geoms)
        for (int a = 0; a < 3; ++a)
            if (!(std::fabs(d.box_lo[a]) < 1e17f) || !(std::fabs(d.box_hi[a]) < 1e17f)) return false;
    return true;
}

void build_geom_bvh(const std::vector<DevGeom>& geoms, GeomBvh& out) {
    out = GeomBvh();
    const int n = (int)geoms.size();
    if (n == 0 || !geom_boxes_finite(geoms)) return;
    Builder b{geoms, {}};
    b.bin.reserve(2 * (size_t)n);
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    const int root = b.build(idx.data(), n);
    const std::vector<Bin>& bin = b.bin;

    // breadth-first: todo[k] is the binary node that record k expands
    std::vector<int> todo{root};
    for (size_t k = 0; k < todo.size(); ++k) {
        int kids[4], nk = 0;
        const Bin& top = bin[todo[k]];
        if (top.geom >= 0) {
            kids[nk++] = todo[k];           // a one-geom scene: the root holds its only leaf
        } else {
            kids[nk++] = top.left;
            kids[nk++] = top.right;
            while (nk < 4) {
                int big = -1;
                for (int c = 0; c < nk; ++c)
                    if (bin[kids[c]].geom < 0 && (big < 0 || bin[kids[c]].area > bin[kids[big]].area)) big = c;
                if (big < 0) break;
                const int l = bin[kids[big]].left, r = bin[kids[big]].right;
                for (int c = nk; c > big + 1; --c) kids[c] = kids[c - 1];   // its two children take its place
                kids[big] = l;
                kids[big + 1] = r;
                ++nk;
            }
        }
        DevGeomNode rec;
        for (int c = 0; c < 4; ++c) {
            for (int a = 0; a < 3; ++a) {   // empty slot: an inverted box
                rec.lo[a][c] = c < nk ? bin[kids[c]].lo[a] : std::numeric_limits<float>::infinity();
                rec.hi[a][c] = c < nk ? bin[kids[c]].hi[a] : -std::numeric_limits<float>::infinity();
            }
            rec.spare[c] = 0.0f;
            if (c >= nk) {
                rec.ref[c] = INT32_MIN;
            } else if (bin[kids[c]].geom >= 0) {
                rec.ref[c] = ~bin[kids[c]].geom;
            } else {
                rec.ref[c] = (int32_t)(todo.size());
                todo.push_back(kids[c]);
            }
        }
        out.nodes.push_back(rec);
    }
    int height = 0;
    const int need = std::max(1, walk_need(out.nodes, 0, 1, height));   // 1: the root's own entry
    out.height = height;
    out.stack_entries = 3 * height + 1;
    assert(need <= out.stack_entries);
    if (need > out.stack_entries) out = GeomBvh();   // (unreachable: each level adds at most 3)
}

}  // namespace pth
