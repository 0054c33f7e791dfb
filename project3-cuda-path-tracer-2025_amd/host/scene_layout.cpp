// scene_layout.cpp — pt_scene_view -> the device buffers' byte images (see scene_layout.h).
//
// One step per record family, in the order pt_init has always run them (the error checks fire in
// that order): geoms and their cull boxes, cull rows, materials, BVH nodes and their aux records,
// hot and cold triangles, the pair layout with its 4-wide and leaf records, the naive-mesh records,
// the candidate table.  Compiled with -ffp-contract=off like every host file: each expression
// rounds where it is written.
#include "scene_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "trav_tree.h"

namespace pth {
using namespace ptd;
namespace {

int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

bool is_leaf_node(const pt_bvh_node& nd) { return nd.triCount > 0 && nd.start >= 0; }

// max DFS stack the reference traversal can reach on this tree (no culling)
int bvh_max_stack(const pt_bvh_node* nodes, int n) {
    if (n <= 0) return 0;
    std::vector<int> st;
    st.push_back(0);
    size_t mx = 1;
    std::vector<char> seen(n, 0);
    while (!st.empty()) {
        int i = st.back();
        st.pop_back();
        if (i < 0 || i >= n || seen[i]) continue;
        seen[i] = 1;
        const pt_bvh_node& nd = nodes[i];
        if (is_leaf_node(nd)) continue;
        if (nd.left >= 0) st.push_back(nd.left);
        if (nd.right >= 0) st.push_back(nd.right);
        mx = std::max(mx, st.size());
    }
    return (int)mx;
}

// levels of the tree below node 0 (root = 1); -1 for a malformed tree (a child out of range or
// reached twice).  The near-first traversals (VAR_BVH_FAST) push at most one entry per level.
int bvh_height(const pt_bvh_node* nodes, int n) {
    if (n <= 0) return 0;
    std::vector<std::pair<int, int>> st{{0, 1}};
    std::vector<char> seen(n, 0);
    int h = 0;
    while (!st.empty()) {
        const int i = st.back().first, d = st.back().second;
        st.pop_back();
        if (i < 0 || i >= n || seen[i]) return -1;
        seen[i] = 1;
        h = std::max(h, d);
        const pt_bvh_node& nd = nodes[i];
        if (is_leaf_node(nd)) continue;
        if (nd.left >= 0) st.push_back({nd.left, d + 1});
        if (nd.right >= 0) st.push_back({nd.right, d + 1});
    }
    return h;
}

// The pre-test's candidate table (SceneDev::grid, read by grid_superset): GRID_G^3 origin cells
// over the scene x 6 dominant-axis faces x GRID_B^2 bins of the two other direction ratios
// (d_i / |d_k| in [-1, 1]).  Entry bit g is set when SOME ray with its origin in the cell and its
// direction in the bin can reach geom g's conservative world box at a nonnegative distance --
// interval arithmetic in double along the dominant axis (the distance interval tau) and then on
// the other two axes (origin interval + ratio interval x tau interval), a superset of the real
// condition.  Every exact hit point lies in that box (the pre-test's premise, cull_geom), so a geom
// outside the entry cannot be hit.  The cells are grown by far more than the device's float
// cell computation can be off, the bins likewise for its rcp-based ratio, the boxes by 1e-6 of
// the scene.  The two ratio axes are bounded independently, so an entry is the AND of one mask
// per bin of each: with PT_GRID_SEP the table holds those 2 GRID_B masks per (cell, face) and the
// device ANDs them (the same entries in 2 / GRID_B of the words).  Returns false (no table) for
// scenes whose geom boxes are not finite.
bool build_candidate_table(const std::vector<DevCull>& culls, int ng, const pt_vec3& cam,
                           std::vector<unsigned long long>& table, float lo_out[3], float inv_out[3]) {
    double lo[3] = {cam.x, cam.y, cam.z}, hi[3] = {cam.x, cam.y, cam.z};
    for (int g = 0; g < ng; ++g)
        for (int a = 0; a < 3; ++a) {
            if (!(std::fabs(culls[g].lo[a]) < 1e17f && std::fabs(culls[g].hi[a]) < 1e17f)) return false;
            lo[a] = std::min(lo[a], (double)culls[g].lo[a]);
            hi[a] = std::max(hi[a], (double)culls[g].hi[a]);
        }
    double ext = 1.0;
    for (int a = 0; a < 3; ++a) ext = std::max({ext, std::fabs(lo[a]), std::fabs(hi[a])});
    double cs[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] -= 1e-3 * ext;
        hi[a] += 1e-3 * ext;
        lo_out[a] = (float)lo[a];
        lo[a] = lo_out[a];                                  // the device's origin of the cells
        inv_out[a] = (float)(GRID_G / (hi[a] - lo[a]));
        cs[a] = 1.0 / (double)inv_out[a];                   // the device's cell size
    }
    const double cm = 1e-6 * ext, bin_eps = 1e-5;
    const int G = GRID_G, B = GRID_B;
    table.assign((size_t)G * G * G * 6 * (PT_GRID_SEP ? 2 * B : B * B), 0ull);
    std::vector<double> ta(ng), tb(ng);
    std::vector<unsigned long long> mi(B), mj(B);
    for (int cz = 0; cz < G; ++cz)
        for (int cy = 0; cy < G; ++cy)
            for (int cx = 0; cx < G; ++cx) {
                const int c[3] = {cx, cy, cz};
                double cl[3], ch[3];
                for (int a = 0; a < 3; ++a) {
                    cl[a] = lo[a] + c[a] * cs[a] - (1e-4 * cs[a] + cm);
                    ch[a] = lo[a] + (c[a] + 1) * cs[a] + (1e-4 * cs[a] + cm);
                }
                const int cell = (cz * G + cy) * G + cx;
                for (int face = 0; face < 6; ++face) {
                    const int k = face / 2, i = (k + 1) % 3, j = (k + 2) % 3;
                    const double s = (face & 1) ? 1.0 : -1.0;
                    unsigned long long mk_ = 0;
                    for (int g = 0; g < ng; ++g) {   // distance along axis k to reach the box's k-slab
                        const double bl = culls[g].lo[k] - cm, bh = culls[g].hi[k] + cm;
                        double a0 = s > 0 ? bl - ch[k] : cl[k] - bh, a1 = s > 0 ? bh - cl[k] : ch[k] - bl;
                        a0 = std::max(a0, -cm);
                        ta[g] = a0;
                        tb[g] = a1;
                        if (a1 >= a0) mk_ |= 1ull << g;
                    }
                    for (int axis = 0; axis < 2; ++axis) {
                        const int a = axis == 0 ? i : j;
                        std::vector<unsigned long long>& m = axis == 0 ? mi : mj;
                        for (int b = 0; b < B; ++b) {
                            const double r0 = (b == 0 ? -1.0 : -1.0 + 2.0 * b / B) - bin_eps;
                            const double r1 = (b == B - 1 ? 1.0 : -1.0 + 2.0 * (b + 1) / B) + bin_eps;
                            unsigned long long bits = 0;
                            for (int g = 0; g < ng; ++g) {
                                if (!((mk_ >> g) & 1)) continue;
                                const double p[4] = {r0 * ta[g], r0 * tb[g], r1 * ta[g], r1 * tb[g]};
                                const double pl = std::min({p[0], p[1], p[2], p[3]});
                                const double ph = std::max({p[0], p[1], p[2], p[3]});
                                if (cl[a] + pl <= (double)culls[g].hi[a] + cm && ch[a] + ph >= (double)culls[g].lo[a] - cm)
                                    bits |= 1ull << g;
                            }
                            m[b] = bits;
                        }
                    }
                    if (PT_GRID_SEP) {   // the device ANDs the two bins' masks
                        unsigned long long* row = &table[((size_t)cell * 6 + face) * 2 * B];
                        for (int b = 0; b < B; ++b) {
                            row[b] = mi[b];
                            row[B + b] = mj[b];
                        }
                        continue;
                    }
                    unsigned long long* row = &table[((size_t)cell * 6 + face) * B * B];
                    for (int bu = 0; bu < B; ++bu)
                        for (int bv = 0; bv < B; ++bv) row[bu * B + bv] = mi[bu] & mj[bv];
                }
            }
    return true;
}

// Every inner node's box contains both children's boxes and every leaf's box contains its
// triangles' vertices, with ordered (non-NaN) bounds -- true of every tree scene.cpp:428-441
// builds (each box is the min / max over its own triangles).  The reference then visits a leaf
// iff the leaf's own box passes, which is what a different hierarchy above the
// leaves and the certified t-culls need.  Called after the structural checks (children and
// triIndices in range).
bool bvh_boxes_nested(const pt_scene_view& s) {
    auto inside = [](const pt_vec3& lo, const pt_vec3& hi, const pt_vec3& a, const pt_vec3& b) {
        return lo.x <= a.x && lo.y <= a.y && lo.z <= a.z && b.x <= hi.x && b.y <= hi.y && b.z <= hi.z;
    };
    for (int i = 0; i < s.num_bvh_nodes; ++i) {
        const pt_bvh_node& nd = s.bvh_nodes[i];
        if (is_leaf_node(nd)) {
            for (int k = 0; k < nd.triCount; ++k) {
                const int64_t j = (int64_t)nd.start + k;
                if (j >= s.num_tri_indices) return false;
                const int ti = s.tri_indices[j];
                if (ti < 0 || ti >= s.num_triangles) return false;
                const pt_triangle& t = s.triangles[ti];
                for (const pt_vertex* v : {&t.v1, &t.v2, &t.v3})
                    if (!inside(nd.aabb.min, nd.aabb.max, v->position, v->position)) return false;
            }
            continue;
        }
        for (int c : {nd.left, nd.right}) {
            if (c < 0) continue;
            if (c >= s.num_bvh_nodes) return false;
            const pt_bvh_node& ch = s.bvh_nodes[c];
            if (!inside(nd.aabb.min, nd.aabb.max, ch.aabb.min, ch.aabb.max)) return false;
        }
    }
    return true;
}

// ---- geoms: the three affine matrices, the away axis, the conservative world box ----
void fill_geoms(const pt_scene_view& s, std::vector<DevGeom>& geoms) {
    geoms.resize(s.num_geoms);
    for (int i = 0; i < s.num_geoms; ++i) {
        const pt_geom& gg = s.geoms[i];
        DevGeom& d = geoms[i];
        memset(&d, 0, sizeof d);
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) {
                d.inv[c * 3 + r] = gg.inverseTransform.m[c][r];
                d.fwd[c * 3 + r] = gg.transform.m[c][r];
                d.itr[c * 3 + r] = gg.invTranspose.m[c][r];
            }
        d.type = gg.type;
        d.materialid = gg.materialid;
        // away_on_axis pre-test: the object axis of smallest world scale (a wall's thin axis,
        // the face a ray leaving it crosses); only when the inverse matrix is bounded so that
        // dot(u, u) < inf is guaranteed for |rd| components <= 1e3
        d.away_axis = -1;
        if (gg.type == PT_CUBE) {
            double big = 0.0;
            for (int c = 0; c < 4; ++c)
                for (int r = 0; r < 3; ++r) big = std::max(big, std::fabs((double)gg.inverseTransform.m[c][r]));
            if (big <= 1e12) {
                double best = 1e300;
                for (int a = 0; a < 3; ++a) {
                    const double len = std::sqrt((double)gg.transform.m[a][0] * gg.transform.m[a][0] +
                                                 (double)gg.transform.m[a][1] * gg.transform.m[a][1] +
                                                 (double)gg.transform.m[a][2] * gg.transform.m[a][2]);
                    if (len < best) {
                        best = len;
                        d.away_axis = a;
                    }
                }
            }
        }
    }
}

// conservative world boxes for cull_geom: the transformed unit cube (contains the radius-0.5
// sphere too), grown by a margin far above every rounding the exact test can make (1e-3 of
// the largest half extent + 1e-3 absolute; object-space pull-back is 1e-4 times the scale)
// and above the cull's own fma/rcp error for ray origins anywhere in the scene (1e-6 of the
// scene extent), then rounded outward.
void fill_geom_boxes(const pt_scene_view& s, std::vector<DevGeom>& geoms) {
    double extent = std::max({std::fabs((double)s.camera.position.x), std::fabs((double)s.camera.position.y),
                              std::fabs((double)s.camera.position.z), 1.0});
    std::vector<float> bc(3 * (size_t)s.num_geoms), bh(3 * (size_t)s.num_geoms);
    std::vector<char> fin(s.num_geoms);
    for (int i = 0; i < s.num_geoms; ++i) {
        DevGeom& d = geoms[i];
        float hmax = 0.f;
        for (int r = 0; r < 3; ++r) {
            bc[3 * i + r] = d.fwd[9 + r];
            bh[3 * i + r] = 0.5f * (std::fabs(d.fwd[r]) + std::fabs(d.fwd[3 + r]) + std::fabs(d.fwd[6 + r]));
            hmax = std::max(hmax, bh[3 * i + r]);
        }
        for (int r = 0; r < 3; ++r) bh[3 * i + r] += 1e-3f * hmax + 1e-3f * std::max(1.0f, hmax);
        fin[i] = std::isfinite(hmax) && std::isfinite(bc[3 * i]) && std::isfinite(bc[3 * i + 1]) &&
                 std::isfinite(bc[3 * i + 2]) && hmax < 1e17f;
        if (fin[i])
            for (int r = 0; r < 3; ++r)
                extent = std::max(extent, std::fabs((double)bc[3 * i + r]) + (double)bh[3 * i + r]);
    }
    for (int t = 0; t < s.num_triangles; ++t) {
        const pt_vertex* v[3] = {&s.triangles[t].v1, &s.triangles[t].v2, &s.triangles[t].v3};
        for (auto* x : v) {
            double m = std::max({std::fabs((double)x->position.x), std::fabs((double)x->position.y),
                                 std::fabs((double)x->position.z)});
            if (std::isfinite(m)) extent = std::max(extent, m);
        }
    }
    const float emargin = (float)std::min(1e-6 * extent, 1e17);
    for (int i = 0; i < s.num_geoms; ++i) {
        DevGeom& d = geoms[i];
        for (int r = 0; r < 3; ++r) {
            if (!fin[i]) {   // degenerate transform: a box that never culls
                d.box_lo[r] = -1e18f;
                d.box_hi[r] = 1e18f;
                continue;
            }
            const float h = bh[3 * i + r] + emargin;
            d.box_lo[r] = std::nextafter(bc[3 * i + r] - h, -INFINITY);
            d.box_hi[r] = std::nextafter(bc[3 * i + r] + h, INFINITY);
        }
    }
}

// ---- cull rows: padded to a multiple of CULL_GROUP records (cull_candidates reads that many at a
// time; pad bits are masked) ----
void fill_culls(const pt_scene_view& s, const std::vector<DevGeom>& geoms, std::vector<DevCull>& culls) {
    culls.resize((std::max(1, s.num_geoms) + CULL_GROUP - 1) / CULL_GROUP * CULL_GROUP);
    for (DevCull& c : culls) memset(&c, 0, sizeof c);
    for (int i = 0; i < s.num_geoms; ++i) {
        const DevGeom& d = geoms[i];
        DevCull& c = culls[i];
        memset(&c, 0, sizeof c);
        for (int r = 0; r < 3; ++r) {
            c.lo[r] = d.box_lo[r];
            c.hi[r] = d.box_hi[r];
        }
        const int a = d.away_axis;
        if (d.type == PT_CUBE && a >= 0 && a < 3) {
            for (int k = 0; k < 4; ++k) c.row[k] = d.inv[3 * k + a];
            c.has_row = 1;
        }
    }
}

// ---- materials; no_tex: no material samples a texture or bump map (the fused kernels'
// texture-free build, VAR_NO_TEX) ----
void fill_materials(const pt_scene_view& s, std::vector<DevMaterial>& mats, bool& no_tex) {
    mats.resize(std::max(1, s.num_materials));
    for (int i = 0; i < s.num_materials; ++i) {
        const pt_material& m = s.materials[i];
        DevMaterial& d = mats[i];
        memset(&d, 0, sizeof d);
        d.color[0] = m.color.x;
        d.color[1] = m.color.y;
        d.color[2] = m.color.z;
        d.emittance = m.emittance;
        d.hasReflective = m.hasReflective;
        d.hasRefractive = m.hasRefractive;
        d.roughness = m.roughness;
        d.metallic = m.metallic;
        d.ior = m.indexOfRefraction;
        d.hasTexture = m.hasTexture ? 1 : 0;
        d.textureID = m.textureID;
        d.hasBumpMap = m.hasBumpMap ? 1 : 0;
        d.bumpID = m.bumpID;
        d.bumpScale = m.bumpScale;
    }
    no_tex = true;
    for (int i = 0; i < s.num_materials; ++i)
        if (s.materials[i].hasTexture || s.materials[i].hasBumpMap) no_tex = false;
}

// ---- BVH nodes: the reference's array, children / leaf range in the w components ----
int32_t fill_nodes(const pt_scene_view& s, std::vector<DevNode>& nodes, std::string& err) {
    nodes.resize(s.num_bvh_nodes);
    for (int i = 0; i < s.num_bvh_nodes; ++i) {
        const pt_bvh_node& nd = s.bvh_nodes[i];
        bool leaf = is_leaf_node(nd);
        int a = leaf ? nd.start : nd.left;
        int b = leaf ? -(nd.triCount + 2) : (nd.right >= 0 ? nd.right : -1);
        if (leaf && (int64_t)nd.start + nd.triCount > s.num_tri_indices)
            return fail(err, PT_E_INVALID, "BVH leaf %d indexes past triIndices", i);
        if (!leaf && (nd.left >= s.num_bvh_nodes || nd.right >= s.num_bvh_nodes))
            return fail(err, PT_E_INVALID, "BVH node %d child out of range", i);
        float fa, fb;
        memcpy(&fa, &a, 4);
        memcpy(&fb, &b, 4);
        nodes[i].lo = make_float4(nd.aabb.min.x, nd.aabb.min.y, nd.aabb.min.z, fa);
        nodes[i].hi = make_float4(nd.aabb.max.x, nd.aabb.max.y, nd.aabb.max.z, fb);
    }
    return PT_OK;
}

// ---- node_aux: per-node culling bounds (from the largest triangle edge below the node) and the
// reference's DFS visit rank (push left, push right, pop); cull_extent: the scene's extent ----
void fill_node_aux(const pt_scene_view& s, const std::vector<DevGeom>& geoms, std::vector<float4>& node_aux,
                   double& cull_extent) {
    node_aux.assign(s.num_bvh_nodes, make_float4(0.f, 0.f, 0.f, 0.f));
    double extent = std::max({1.0, std::fabs((double)s.camera.position.x), std::fabs((double)s.camera.position.y),
                              std::fabs((double)s.camera.position.z)});
    for (int t = 0; t < s.num_triangles; ++t) {
        const pt_vertex* v[3] = {&s.triangles[t].v1, &s.triangles[t].v2, &s.triangles[t].v3};
        for (auto* x : v)
            extent = std::max({extent, std::fabs((double)x->position.x), std::fabs((double)x->position.y),
                               std::fabs((double)x->position.z)});
    }
    for (int i = 0; i < s.num_geoms; ++i)   // hit points on primitives are ray origins too
        for (int r = 0; r < 3; ++r)
            extent = std::max(extent, std::fabs((double)geoms[i].box_lo[r]) + std::fabs((double)geoms[i].box_hi[r]));
    cull_extent = extent;
    std::vector<double> smax(s.num_bvh_nodes, -1.0);
    // bottom-up max edge: children have larger indices than parents in the reference build,
    // but compute it by explicit post-order to accept any valid tree
    std::vector<int> order, st{0};
    std::vector<char> seen(s.num_bvh_nodes, 0);
    while (!st.empty()) {
        int n = st.back();
        st.pop_back();
        if (n < 0 || n >= s.num_bvh_nodes || seen[n]) continue;
        seen[n] = 1;
        order.push_back(n);
        const pt_bvh_node& nd = s.bvh_nodes[n];
        if (!is_leaf_node(nd)) {
            if (nd.left >= 0) st.push_back(nd.left);
            if (nd.right >= 0) st.push_back(nd.right);
        }
    }
    for (size_t k = order.size(); k-- > 0;) {
        const int n = order[k];
        const pt_bvh_node& nd = s.bvh_nodes[n];
        double m = 0.0;
        if (is_leaf_node(nd)) {
            for (int i = 0; i < nd.triCount; ++i) {
                const int ti = s.tri_indices[nd.start + i];
                if (ti < 0 || ti >= s.num_triangles) continue;   // rejected by fill_hot
                const pt_triangle& t = s.triangles[ti];
                const double e1 = std::hypot((double)t.v2.position.x - t.v1.position.x,
                                             (double)t.v2.position.y - t.v1.position.y,
                                             (double)t.v2.position.z - t.v1.position.z);
                const double e2 = std::hypot((double)t.v3.position.x - t.v1.position.x,
                                             (double)t.v3.position.y - t.v1.position.y,
                                             (double)t.v3.position.z - t.v1.position.z);
                m = std::max({m, e1, e2});
            }
        } else {
            if (nd.left >= 0) m = std::max(m, smax[nd.left]);
            if (nd.right >= 0) m = std::max(m, smax[nd.right]);
        }
        smax[n] = m;
        const double sx = m * 1.01 + 1e-30;
        const double c = 64.0 * std::ldexp(1.0, -24) * sx * sx / 1e-5;
        node_aux[n].x = (float)std::min(c * 1.01, 1e30);
        node_aux[n].y = (float)std::min(sx, 1e30);
        node_aux[n].w = (float)std::min(c * extent * 1.01, 1e30);
    }
    // reference visit rank
    int rank = 0;
    st.assign(1, 0);
    std::fill(seen.begin(), seen.end(), 0);
    while (!st.empty()) {
        int n = st.back();
        st.pop_back();
        if (n < 0 || n >= s.num_bvh_nodes) continue;
        int r = rank++;
        float fr;
        memcpy(&fr, &r, 4);
        node_aux[n].z = fr;
        const pt_bvh_node& nd = s.bvh_nodes[n];
        if (!is_leaf_node(nd) && !seen[n]) {
            seen[n] = 1;
            if (nd.left >= 0) st.push_back(nd.left);
            if (nd.right >= 0) st.push_back(nd.right);
        }
    }
}

// the three positions of triangle ti, tagged with the int `tag` (its triangle index)
DevTriHot hot_record(const pt_triangle& t, int tag) {
    float ftag;
    memcpy(&ftag, &tag, 4);
    DevTriHot h;
    h.a = make_float4(t.v1.position.x, t.v1.position.y, t.v1.position.z, t.v2.position.x);
    h.b = make_float4(t.v2.position.y, t.v2.position.z, t.v3.position.x, t.v3.position.y);
    h.c = make_float4(t.v3.position.z, ftag, 0.f, 0.f);
    return h;
}

// ---- hot triangles in leaf order (index k = node.start + i) ----
int32_t fill_hot(const pt_scene_view& s, std::vector<DevTriHot>& hot, std::string& err) {
    hot.resize(s.num_tri_indices);
    for (int k = 0; k < s.num_tri_indices; ++k) {
        int ti = s.tri_indices[k];
        if (ti < 0 || ti >= s.num_triangles) return fail(err, PT_E_INVALID, "triIndices[%d] out of range", k);
        hot[k] = hot_record(s.triangles[ti], ti);
    }
    return PT_OK;
}

// ---- cold triangle data by reference triangle index (vertex normals, uvs, tangents, material) ----
int32_t fill_cold(const pt_scene_view& s, std::vector<DevTriCold>& cold, std::string& err) {
    cold.resize(s.num_triangles);
    for (int i = 0; i < s.num_triangles; ++i) {
        const pt_triangle& t = s.triangles[i];
        DevTriCold& c = cold[i];
        memset(&c, 0, sizeof c);
        const pt_vertex* v[3] = {&t.v1, &t.v2, &t.v3};
        float* ns[3] = {c.n0, c.n1, c.n2};
        float* uvs[3] = {c.uv0, c.uv1, c.uv2};
        for (int k = 0; k < 3; ++k) {
            ns[k][0] = v[k]->normal.x;
            ns[k][1] = v[k]->normal.y;
            ns[k][2] = v[k]->normal.z;
            uvs[k][0] = v[k]->uv.x;
            uvs[k][1] = v[k]->uv.y;
        }
        c.dpdu[0] = t.dpdu.x; c.dpdu[1] = t.dpdu.y; c.dpdu[2] = t.dpdu.z;
        c.dpdv[0] = t.dpdv.x; c.dpdv[1] = t.dpdv.y; c.dpdv[2] = t.dpdv.z;
        c.materialID = t.materialID;
        if (t.materialID < 0 || t.materialID >= std::max(1, s.num_materials))
            return fail(err, PT_E_INVALID, "triangle %d material %d out of range", i, t.materialID);
    }
    return PT_OK;
}

// The reference tree as the pair layout numbers it: walked in the reference's visit order (push
// left, push right, pop -> right subtree first), internal nodes (pairs) and leaves (4-slot
// triangle groups) numbered apart.  ok is false for any tree the layout cannot hold exactly: a
// missing child, a node reached twice, a leaf of more than 4 triangles.
struct RefTree {
    std::vector<int> id;           // per node: its pair or leaf number (-1: not reached)
    std::vector<char> is_leaf;
    std::vector<int> leaf_nodes;   // node of leaf k
    int P = 0, L = 0, height = 0;
    bool ok = true;
    int ref(int n) const { return is_leaf[n] ? P + id[n] : id[n]; }
};
RefTree number_reference_tree(const pt_scene_view& s) {
    const int nn = s.num_bvh_nodes;
    RefTree t;
    t.id.assign(nn, -1);
    t.is_leaf.assign(nn, 0);
    std::vector<std::pair<int, int>> st{{0, 1}};
    while (!st.empty() && t.ok) {
        const int n = st.back().first, d = st.back().second;
        st.pop_back();
        if (n < 0 || n >= nn || t.id[n] >= 0) { t.ok = false; break; }
        t.height = std::max(t.height, d);
        const pt_bvh_node& nd = s.bvh_nodes[n];
        if (is_leaf_node(nd)) {
            if (nd.triCount > 4) t.ok = false;
            t.is_leaf[n] = 1;
            t.id[n] = t.L++;
            t.leaf_nodes.push_back(n);
        } else {
            if (nd.left < 0 || nd.right < 0) { t.ok = false; break; }
            t.id[n] = t.P++;
            st.push_back({nd.left, d + 1});
            st.push_back({nd.right, d + 1});
        }
    }
    if (t.ok) {   // internal refs breadth-first: the top levels share a few cache lines
        std::vector<int> fifo{0};
        int k = 0;
        for (size_t h = 0; h < fifo.size(); ++h) {
            const int n = fifo[h];
            if (t.is_leaf[n]) continue;
            t.id[n] = k++;
            fifo.push_back(s.bvh_nodes[n].left);
            fifo.push_back(s.bvh_nodes[n].right);
        }
    }
    return t;
}

// cull_threshold_packed's constants for a child of cull size s (same c0 and E as SceneDev::cull_c0 /
// cull_E), evaluated in double and rounded up
struct CullPacker {
    float c0f, Ef;
    explicit CullPacker(double cull_extent)
        : c0f((float)(64.0 * std::ldexp(1.0, -24) / 1e-5 * 1.01 * (1.0 + 1e-5))), Ef((float)(cull_extent * (1.0 + 1e-5))) {}
    float operator()(float sf) const {
        auto up16 = [](double v) -> uint32_t {
            if (!(v >= 0.0)) v = HUGE_VAL;                  // NaN: never cull
            float f = (float)v;
            if ((double)f < v) f = std::nextafter(f, HUGE_VALF);
            uint32_t b;
            memcpy(&b, &f, 4);
            if (b & 0xffffu) b = (b & 0xffff0000u) + 0x10000u;   // up to 16 bits (inf stays inf)
            return b >> 16;
        };
        const double sd = sf, c = sd * sd * (double)c0f;
        const double A = c * sd * 1.002 + c * (double)Ef * (1.0 + 1e-6);
        const double d = 1.0 - (1.0 - 1e-6) / (1.0 + 2.0 * c + 2e-6);
        const uint32_t w = (up16(A) << 16) | up16(d);
        float f;
        memcpy(&f, &w, 4);
        return f;
    }
};

// The hierarchy above the reference's leaves (trav_tree.h): a binned-SAH tree over them, its
// inner boxes the unions of their leaves' boxes, unless a leaf box has a NaN / infinite bound (the
// containment argument needs ordered bounds), the union differs from the reference root box, or
// the tree would not fit the stack.  The traversal kernels keep one stack entry per tree level in
// LDS, so the height is bounded (LayoutParams::sah_max_height).
bool build_sah_hierarchy(const RefTree& rt, const LayoutParams& p, const SceneLayout& out, std::vector<TravInner>& tt,
                         int& th) {
    const int L = rt.L;
    std::vector<float> llo(3 * (size_t)L), lhi(3 * (size_t)L), ls(L);
    for (int k = 0; k < L; ++k) {
        const DevNode& nd = out.nodes[rt.leaf_nodes[k]];
        llo[3 * k] = nd.lo.x; llo[3 * k + 1] = nd.lo.y; llo[3 * k + 2] = nd.lo.z;
        lhi[3 * k] = nd.hi.x; lhi[3 * k + 1] = nd.hi.y; lhi[3 * k + 2] = nd.hi.z;
        ls[k] = out.node_aux[rt.leaf_nodes[k]].y;
    }
    bool sah = build_sah_tree(llo, lhi, ls, tt, th, p.bvh_bfs_levels, p.sah_max_height) && th + 1 <= MAXSTACK &&
               (int64_t)tt.size() + L < (1 << 24);
    if (sah) {   // the union of the leaves is the reference root box, bit for bit
        const TravChild& a = tt[0].c[0];
        const TravChild& b = tt[0].c[1];
        const float r[6] = {out.nodes[0].lo.x, out.nodes[0].lo.y, out.nodes[0].lo.z,
                            out.nodes[0].hi.x, out.nodes[0].hi.y, out.nodes[0].hi.z};
        for (int ax = 0; ax < 3; ++ax)
            sah = sah && std::min(a.lo[ax], b.lo[ax]) == r[ax] && std::max(a.hi[ax], b.hi[ax]) == r[3 + ax];
    }
    return sah;
}

// pairs over the SAH tree: pair i holds inner node i's two children
void fill_sah_pairs(const std::vector<TravInner>& tt, const CullPacker& pack_cull, std::vector<DevPair>& pairs) {
    const int P = (int)tt.size();
    pairs.resize(P);
    for (int i = 0; i < P; ++i) {
        DevPair& pr = pairs[i];
        float4* lo[2] = {&pr.l_lo, &pr.r_lo};
        float4* hi[2] = {&pr.l_hi, &pr.r_hi};
        for (int k = 0; k < 2; ++k) {
            const TravChild& c = tt[i].c[k];
            const int rf = c.leaf ? P + c.ref : c.ref;
            float frf;
            memcpy(&frf, &rf, 4);
            *lo[k] = make_float4(c.lo[0], c.lo[1], c.lo[2], frf);
            *hi[k] = make_float4(c.hi[0], c.hi[1], c.hi[2], pack_cull(c.s));
        }
    }
}

// pairs over the reference's own hierarchy (pairs already sized)
void fill_ref_pairs(const pt_scene_view& s, const RefTree& rt, const SceneLayout& out, const CullPacker& pack_cull,
                    std::vector<DevPair>& pairs) {
    for (int n = 0; n < s.num_bvh_nodes; ++n) {
        if (rt.id[n] < 0 || rt.is_leaf[n]) continue;
        const pt_bvh_node& nd = s.bvh_nodes[n];
        DevPair& pr = pairs[rt.id[n]];
        const int kids[2] = {nd.left, nd.right};
        float4* lo[2] = {&pr.l_lo, &pr.r_lo};
        float4* hi[2] = {&pr.l_hi, &pr.r_hi};
        for (int k = 0; k < 2; ++k) {
            const int c = kids[k];
            const int rf = rt.ref(c);
            float frf;
            memcpy(&frf, &rf, 4);
            *lo[k] = make_float4(out.nodes[c].lo.x, out.nodes[c].lo.y, out.nodes[c].lo.z, frf);
            *hi[k] = make_float4(out.nodes[c].hi.x, out.nodes[c].hi.y, out.nodes[c].hi.z, pack_cull(out.node_aux[c].y));
        }
    }
}

// The 4-wide form of the SAH hierarchy: record q holds the children of binary node n, an inner
// child replaced by its own two children (two levels per record, one 128-B line); quad 0 is the
// root's.  Inner refs breadth-first over the top levels, preorder below, as the pairs
// (PT_BVH_BFS_LEVELS / 2 levels).  Returns the stack entries its traversal can need (0: not built).
int fill_quads(const std::vector<TravInner>& tt, int bfs_levels, const CullPacker& pack_cull, std::vector<float4>& quads) {
    std::vector<QuadRecord> qr;
    int qneed = 0;
    build_quad_records(tt, std::max(0, bfs_levels / 2), qr, qneed);
    // the hand-over saves the stack depth in 7 bits (trav_saved_node): deeper worst cases (trees
    // far past the height bound) keep the pairs
    if (qneed + 1 > 96) qr.clear();
    const int Q = (int)qr.size();
    quads.assign(8 * (size_t)Q, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int q = 0; q < Q; ++q) {
        float4* R = &quads[8 * (size_t)q];
        float* f[8] = {&R[0].x, &R[1].x, &R[2].x, &R[3].x, &R[4].x, &R[5].x, &R[6].x, &R[7].x};
        for (int i = 0; i < 4; ++i) {
            int rf = -1;   // no child
            if (i < qr[q].n) {
                const TravChild& c = qr[q].c[i];
                for (int a = 0; a < 3; ++a) {
                    f[a][i] = c.lo[a];
                    f[3 + a][i] = c.hi[a];
                }
                rf = c.leaf ? Q + c.ref : c.ref;
                f[7][i] = pack_cull(c.s);
            }
            memcpy(&f[6][i], &rf, 4);
        }
    }
    return Q > 0 ? qneed + 1 : 0;
}

// ---- leaf records: hot4 (4 triangle slots per leaf, slot 0's c.z = count) and trav_step's leaf9:
// component k of the 4 slots in one float4, positions as v0 and the float edges v1 - v0, v2 - v0
// (tri_test's own first rounding) ----
void fill_leaf_records(const pt_scene_view& s, const RefTree& rt, const std::vector<DevTriHot>& hot,
                       std::vector<DevTriHot>& hot4, std::vector<float4>& leaf9) {
    const int L = rt.L;
    hot4.assign(4 * (size_t)L, DevTriHot{});
    for (int k = 0; k < L; ++k) {
        const pt_bvh_node& nd = s.bvh_nodes[rt.leaf_nodes[k]];
        for (int i = 0; i < nd.triCount; ++i) hot4[4 * (size_t)k + i] = hot[nd.start + i];
        const int cnt = nd.triCount;
        memcpy(&hot4[4 * (size_t)k].c.z, &cnt, 4);
    }
    leaf9.assign(9 * (size_t)L, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int k = 0; k < L; ++k)
        for (int i = 0; i < 4; ++i) {
            const DevTriHot& h = hot4[4 * (size_t)k + i];
            const float v0[3] = {h.a.x, h.a.y, h.a.z}, v1[3] = {h.a.w, h.b.x, h.b.y}, v2[3] = {h.b.z, h.b.w, h.c.x};
            float comp9[9];
            for (int a = 0; a < 3; ++a) {
                comp9[a] = v0[a];
                comp9[3 + a] = v1[a] - v0[a];
                comp9[6 + a] = v2[a] - v0[a];
            }
            for (int m = 0; m < 9; ++m) (&leaf9[9 * (size_t)k + m].x)[i] = comp9[m];
        }
}

// ---- VAR_BVH_FAST pair layout (DevPair) with its 4-wide and leaf records.  Any tree it cannot
// hold exactly -- RefTree's cases, 2^24 refs or more (pack_ref's widest ref field), a deeper tree
// than the stack -- or whose boxes are not nested keeps the node-array traversal: pairs stay empty.
void build_pair_layout(const pt_scene_view& s, const LayoutParams& p, bool nested, SceneLayout& out) {
    const RefTree rt = number_reference_tree(s);
    int P = rt.P;
    const int L = rt.L;
    if (!(rt.ok && nested && (int64_t)P + L < (1 << 24) && rt.height + 1 <= MAXSTACK && !(out.variant & VAR_BVH_NODES)))
        return;
    const CullPacker pack_cull(out.cull_extent);
    // PT_BVH_TREE=ref (tools, A/B) keeps the reference's own hierarchy
    std::vector<TravInner> tt;
    int th = 0;
    const bool sah = !p.bvh_tree_ref && L >= 2 && build_sah_hierarchy(rt, p, out, tt, th);
    if (sah) {
        P = (int)tt.size();
        fill_sah_pairs(tt, pack_cull, out.pairs);
        out.stack_depth = std::max(out.stack_depth, th + 1);
        out.pair_depth = th + 1;
        if (p.bvh_quad > 0) {
            out.quad_stack = fill_quads(tt, p.bvh_bfs_levels, pack_cull, out.quads);
            out.stack_depth = std::max(out.stack_depth, out.quad_stack);
            out.pair_depth = std::max(out.pair_depth, out.quad_stack);   // the push bound covers both
            if (p.bvh_tree_info)
                fprintf(stderr, "pt_init: 4-wide records %d (pairs %d), stack %d entries\n", (int)(out.quads.size() / 8), P,
                        out.quad_stack);
        }
        if (p.bvh_tree_info)
            fprintf(stderr, "pt_init: SAH traversal tree over %d reference leaves, height %d (reference %d)\n", L, th,
                    rt.height);
    }
    out.pairs.resize(std::max(1, P));
    if (!sah) {
        fill_ref_pairs(s, rt, out, pack_cull, out.pairs);
        out.pair_depth = rt.height + 1;
    }
    fill_leaf_records(s, rt, out.hot, out.hot4, out.leaf9);
    out.root_ref = sah ? 0 : rt.ref(0);
    out.root_lo = make_float4(out.nodes[0].lo.x, out.nodes[0].lo.y, out.nodes[0].lo.z, 0.f);
    out.root_hi = make_float4(out.nodes[0].hi.x, out.nodes[0].hi.y, out.nodes[0].hi.z, out.node_aux[0].y);
    out.pair_count = P;
    // stack entries: as few ref bits as the P + L refs need, the rest for the cull T
    int rb = 2;
    while (((int64_t)1 << rb) < (int64_t)P + L) ++rb;
    out.ref_shift = 32 - rb;
}

// ---- the BVH buffers and the traversal stack's depth ----
int32_t build_bvh_layout(const pt_scene_view& s, const LayoutParams& p, SceneLayout& out, std::string& err) {
    if (int32_t rc = fill_nodes(s, out.nodes, err)) return rc;
    fill_node_aux(s, out.geoms, out.node_aux, out.cull_extent);
    if (int32_t rc = fill_hot(s, out.hot, err)) return rc;
    if (int32_t rc = fill_cold(s, out.cold, err)) return rc;
    // traversal stack (LDS, MAXSTACK entries per lane at most).  The reference-order DFS needs
    // bvh_max_stack entries -- more than 64 overflows the reference's own int stack[64]
    // (intersections.cu:167), so such a tree is refused rather than traversed differently.
    // The near-first traversals need up to height + 1; a tree too deep (or malformed) for
    // that keeps the reference-order traversal.  No push is ever dropped.
    const int ref_stack = bvh_max_stack(s.bvh_nodes, s.num_bvh_nodes);
    if (ref_stack > MAXSTACK)
        return fail(err, PT_E_UNSUPPORTED, "BVH needs a %d-entry traversal stack; the reference's holds %d "
                    "(intersections.cu:167)", ref_stack, MAXSTACK);
    const int tree_height = bvh_height(s.bvh_nodes, s.num_bvh_nodes);
    // the near-first traversals (pair layout, SAH hierarchy, certified t-culls) rely on the
    // boxes being nested as scene.cpp:428-441 builds them; a caller-supplied tree that is not
    // keeps the reference-order traversal, which assumes nothing
    const bool nested = bvh_boxes_nested(s);
    if (tree_height < 0 || tree_height + 1 > MAXSTACK || !nested) out.variant &= ~(VAR_BVH_FAST | VAR_BVH_SPLIT);
    out.stack_depth = std::max(2, ref_stack);
    if (out.variant & VAR_BVH_FAST) out.stack_depth = std::max(out.stack_depth, tree_height + 1);
    build_pair_layout(s, p, nested, out);
    return PT_OK;
}

}  // namespace

int32_t build_scene_layout(const pt_scene_view& s, const LayoutParams& p, SceneLayout& out, std::string& err) {
    out = SceneLayout();
    out.variant = p.variant;
    fill_geoms(s, out.geoms);
    fill_geom_boxes(s, out.geoms);
    fill_culls(s, out.geoms, out.culls);
    fill_materials(s, out.mats, out.no_tex);
    // BVH: only when the reference would traverse it (BVH_ACCELERATION and a non-empty tree)
    // (the naive mesh mode skips it whatever the options and the scene view say)
    out.has_bvh = !p.naive && p.bvh && s.num_bvh_nodes > 0 && s.num_triangles > 0;
    if (out.has_bvh)
        if (int32_t rc = build_bvh_layout(s, p, out, err)) return rc;
    // naive mesh mode: the three positions of every triangle in ARRAY order (k_naive_mesh forms the
    // edges tri_test() forms when it stages a tile), record k naming triangle k, and the cold data
    if (p.naive && s.num_triangles > 0) {
        out.naive_hot.resize(s.num_triangles);
        for (int k = 0; k < s.num_triangles; ++k) out.naive_hot[k] = hot_record(s.triangles[k], k);
        if (int32_t rc = fill_cold(s, out.cold, err)) return rc;
    }
    for (int i = 0; i < s.num_geoms; ++i)
        if (s.geoms[i].materialid < 0 || s.geoms[i].materialid >= std::max(1, s.num_materials))
            return fail(err, PT_E_INVALID, "geom %d material %d out of range", i, s.geoms[i].materialid);
    // the pre-test's candidate table, for scenes whose flat pre-test is long (A/B: PT_GRID=0 off,
    // PT_GRID=1 also for scenes under GRID_MIN_GEOMS)
    const int grid_min = p.grid == 1 ? 2 : GRID_MIN_GEOMS;
    if (p.grid != 0 && s.num_geoms >= grid_min && s.num_geoms <= LDS_GEOMS)   // (false: boxes not finite, no table)
        build_candidate_table(out.culls, s.num_geoms, s.camera.position, out.grid, out.grid_lo, out.grid_inv);
    return PT_OK;
}

}  // namespace pth
