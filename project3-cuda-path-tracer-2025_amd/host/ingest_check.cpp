// ingest_check.cpp — the host ingest behind the C-ABI, driven standalone for the sanitizer build
// (Makefile target `asan`: host/*.cpp with -fsanitize=address,undefined, no device code).
//
// The files a caller hands the library are untrusted: scene JSON (host/json_lite.h), OBJ meshes
// (host/scene.cpp's reader) and PNG textures (host/png_decode.cpp, a from-scratch inflate).  The
// reference's failure semantics are an exception for a scene it cannot read (scene.cpp:245-247,
// "Failed to load") and -1 for a texture it cannot decode (scene.cpp:372-375, shown as magenta);
// here: PT_E_INVALID with a message, and textureID -1.  Every input must end in one of those or
// in a loaded scene -- never in a sanitizer report.
//
//   ingest_check scene FILE.json...   pt_scene_load_ex (host BVH) + pt_scene_get_view + the device scene
//                                     layout pt_init builds from it (host/scene_layout.cpp, default
//                                     parameters) + the SAH traversal tree over its leaves under
//                                     other numberings and bounds; prints "scene rc=<rc> ..."
//   ingest_check layout FILE.json [key=value ...]
//                                     the layout under the given LayoutParams (keys: its fields): per
//                                     buffer "buf NAME COUNT DIGEST" (64-bit FNV-1a of its bytes), then
//                                     "scalar NAME VALUE..." (floats as bit patterns), then "rc=<rc> err=..."
//   ingest_check layout-mutate FILE.json KIND
//                                     the same over a copy of the scene's BVH arrays with one corruption
//                                     (mutate_bvh's kinds): a layout or an error, never a sanitizer report
//   ingest_check png FILE...          pt_texture_load (size query, then decode); "png rc=<rc> w h"
//   ingest_check savepng OUT W H      pt_save_png of a W x H test image with NaN / inf / negatives
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pt/pathtrace_abi.h"
#include "scene_layout.h"
#include "trav_tree.h"

static int check_scene(const char* path) {
    pt_scene_file* f = nullptr;
    const int rc = pt_scene_load_ex(path, -1, -1, -1, PT_SCENE_VIEWER_CAMERA, &f);
    if (rc != PT_OK) {
        std::printf("scene rc=%d err=%s\n", rc, pt_scene_last_error());
        return rc;
    }
    pt_scene_view v{};
    pt_scene_get_view(f, &v);
    int32_t iters = 0, depth = 0;
    char name[256];
    pt_scene_get_info(f, &iters, &depth, name, (int32_t)sizeof name);
    int bad_tex = 0;
    for (int i = 0; i < v.num_materials; ++i) {
        char mname[128];
        pt_scene_material_name(f, i, mname, (int32_t)sizeof mname);
        if ((v.materials[i].hasTexture && v.materials[i].textureID < 0) ||
            (v.materials[i].hasBumpMap && v.materials[i].bumpID < 0))
            ++bad_tex;
    }
    // the device scene layout pt_init builds (every buffer's byte image), default parameters
    pth::SceneLayout lay;
    std::string lay_err;
    const int lay_rc = pth::build_scene_layout(v, pth::LayoutParams(), lay, lay_err);
    // its leaves' boxes and cull sizes: the SAH hierarchy over them under other numberings and bounds
    std::vector<float> lo, hi, s;
    for (int i = 0; i < v.num_bvh_nodes && lay_rc == PT_OK && lay.has_bvh; ++i) {
        const pt_bvh_node& nd = v.bvh_nodes[i];
        if (!(nd.triCount > 0 && nd.start >= 0)) continue;
        const float l[3] = {lay.nodes[i].lo.x, lay.nodes[i].lo.y, lay.nodes[i].lo.z};
        const float h[3] = {lay.nodes[i].hi.x, lay.nodes[i].hi.y, lay.nodes[i].hi.z};
        for (int a = 0; a < 3; ++a) {
            lo.push_back(l[a]);
            hi.push_back(h[a]);
        }
        s.push_back(lay.node_aux[i].y);
    }
    std::vector<pth::TravInner> tree;
    int height = 0;
    const bool sah = pth::build_sah_tree(lo, hi, s, tree, height);
    // the same tree under every numbering (breadth-first top levels, preorder below): walk both
    // from the root and compare every child's box, cull size and leaf id
    int orders_equal = sah ? 1 : -1;
    for (int levels : {0, 1, 4, 8}) {
        if (!sah || s.size() > 20000) break;   // (the 262k / 1.0M stand-ins: too slow under ASan)
        std::vector<pth::TravInner> t2;
        int h2 = 0;
        if (!pth::build_sah_tree(lo, hi, s, t2, h2, levels) || h2 != height || t2.size() != tree.size()) {
            orders_equal = 0;
            break;
        }
        std::vector<std::pair<int, int>> st{{0, 0}};
        size_t seen = 0;
        while (!st.empty() && orders_equal) {
            const auto [a, b] = st.back();
            st.pop_back();
            ++seen;
            for (int c = 0; c < 2; ++c) {
                const pth::TravChild &x = tree[a].c[c], &y = t2[b].c[c];
                bool same = x.leaf == y.leaf && x.s == y.s && (!x.leaf || x.ref == y.ref);
                for (int k = 0; k < 3; ++k) same = same && x.lo[k] == y.lo[k] && x.hi[k] == y.hi[k];
                if (!same) orders_equal = 0;
                else if (!x.leaf) st.push_back({x.ref, y.ref});
            }
        }
        if (seen != tree.size()) orders_equal = 0;
    }
    if (sah && s.size() > 20000) orders_equal = -2;   // not checked
    // the tightest height bound (1 + ceil(log2 leaves)): every leaf still in the tree exactly once
    int tight = -1, tight_leaves = 0;
    if (sah) {
        std::vector<pth::TravInner> t3;
        int h3 = 0;
        if (pth::build_sah_tree(lo, hi, s, t3, h3, 1 << 30, 1)) {
            tight = h3;
            std::vector<int> seen(s.size(), 0);
            for (const pth::TravInner& t : t3)
                for (const pth::TravChild& c : t.c)
                    if (c.leaf && c.ref >= 0 && c.ref < (int)s.size()) seen[c.ref]++;
            for (int x : seen) tight_leaves += x == 1;
        }
    }
    // the 4-wide records: every leaf in exactly one record, every record but the root referenced
    // exactly once and after its parent... 2..4 children, each child's box the tree's own
    int quads = -1, quad_ok = -1, quad_need = -1;
    if (sah) {
        std::vector<pth::QuadRecord> qr;
        pth::build_quad_records(tree, 6, qr, quad_need);
        quads = (int)qr.size();
        quad_ok = 1;
        std::vector<int> leaf_seen(s.size(), 0), rec_seen(qr.size(), 0);
        for (const pth::QuadRecord& r : qr) {
            if (r.n < 2 || r.n > 4) quad_ok = 0;
            for (int i = 0; i < r.n; ++i) {
                const pth::TravChild& c = r.c[i];
                if (c.leaf) {
                    if (c.ref < 0 || c.ref >= (int)s.size()) quad_ok = 0;
                    else leaf_seen[c.ref]++;
                } else if (c.ref <= 0 || c.ref >= (int)qr.size()) {
                    quad_ok = 0;
                } else {
                    rec_seen[c.ref]++;
                }
                for (int a = 0; a < 3; ++a)
                    if (!(c.lo[a] <= c.hi[a])) quad_ok = 0;
            }
        }
        for (int x : leaf_seen) quad_ok &= x == 1;
        for (size_t q = 1; q < rec_seen.size(); ++q) quad_ok &= rec_seen[q] == 1;
        if (!rec_seen.empty()) quad_ok &= rec_seen[0] == 0;
    }
    std::printf("scene rc=0 geoms=%d materials=%d triangles=%d nodes=%d depth=%d textures=%d bad_tex=%d sah=%d "
                "sah_orders_equal=%d sah_tight=%d leaves=%zu tight_leaves=%d quads=%d quad_ok=%d quad_stack=%d "
                "layout=%d layout_pairs=%zu layout_quads=%zu layout_stack=%d\n",
                v.num_geoms, v.num_materials, v.num_triangles, v.num_bvh_nodes, depth, v.num_textures, bad_tex,
                sah ? height : -1, orders_equal, tight, s.size(), tight_leaves, quads, quad_ok, quad_need, lay_rc,
                lay.pairs.size(), lay.quads.size() / 8, lay.stack_depth);
    pt_scene_free(f);
    return 0;
}

// One corruption of a caller-supplied BVH (copies of the scene's node and index arrays).
static bool mutate_bvh(const std::string& kind, const pt_scene_view& v, std::vector<pt_bvh_node>& nodes,
                       std::vector<int32_t>& idx) {
    auto is_leaf = [](const pt_bvh_node& nd) { return nd.triCount > 0 && nd.start >= 0; };
    int inner = -1, inner2 = -1, leaf = -1, leaf5 = -1;   // first inner node, first inner node below the root, first leaf,
    for (int i = (int)nodes.size(); i-- > 0;) {           // first leaf with 5 indices from its start on
        if (is_leaf(nodes[i])) {
            leaf = i;
            if ((int64_t)nodes[i].start + 5 <= (int64_t)idx.size()) leaf5 = i;
        } else {
            inner = i;
            if (i > 0) inner2 = i;
        }
    }
    if (inner < 0 || inner2 < 0 || leaf < 0 || leaf5 < 0 || idx.empty()) return false;
    if (kind == "unnested") {   // an inner box shrunk: it no longer contains its children's
        pt_bvh_node& nd = nodes[inner];
        nd.aabb.max.x = nd.aabb.min.x + 0.25f * (nd.aabb.max.x - nd.aabb.min.x);
    } else if (kind == "same_child") {
        nodes[inner].right = nodes[inner].left;
    } else if (kind == "child_root") {
        nodes[inner2].right = 0;
    } else if (kind == "child_past_end") {
        nodes[inner].right = (int32_t)nodes.size();
    } else if (kind == "leaf5") {
        nodes[leaf5].triCount = 5;
    } else if (kind == "tri_index_end") {
        idx[0] = v.num_triangles;
    } else if (kind == "leaf_past_end") {
        nodes[leaf].start = (int32_t)idx.size() - nodes[leaf].triCount + 1;
    } else if (kind == "nan_box") {
        nodes[leaf].aabb.min.y = std::numeric_limits<float>::quiet_NaN();
    } else {
        return false;
    }
    return true;
}

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t x = 14695981039346656037ull;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) {
        x ^= b[i];
        x *= 1099511628211ull;
    }
    return x;
}
template <class T>
static void print_buf(const char* name, const std::vector<T>& v) {
    std::printf("buf %s %zu %016llx\n", name, v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}
static unsigned fbits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

static bool parse_param(const std::string& kv, pth::LayoutParams& p) {
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return false;
    const std::string k = kv.substr(0, eq);
    const int x = std::atoi(kv.c_str() + eq + 1);
    if (k == "bvh") p.bvh = x != 0;
    else if (k == "variant") p.variant = x;
    else if (k == "naive") p.naive = x != 0;
    else if (k == "bvh_tree_ref") p.bvh_tree_ref = x != 0;
    else if (k == "bvh_tree_info") p.bvh_tree_info = x != 0;
    else if (k == "bvh_bfs_levels") p.bvh_bfs_levels = x;
    else if (k == "bvh_quad") p.bvh_quad = x;
    else if (k == "grid") p.grid = x;
    else if (k == "sah_max_height") p.sah_max_height = x;
    else return false;
    return true;
}

static int print_layout(const pt_scene_view& v, const pth::LayoutParams& p) {
    pth::SceneLayout l;
    std::string err;
    const int rc = pth::build_scene_layout(v, p, l, err);
    if (rc == PT_OK) {
        print_buf("geoms", l.geoms);
        print_buf("culls", l.culls);
        print_buf("mats", l.mats);
        print_buf("grid", l.grid);
        print_buf("nodes", l.nodes);
        print_buf("node_aux", l.node_aux);
        print_buf("hot", l.hot);
        print_buf("cold", l.cold);
        print_buf("pairs", l.pairs);
        print_buf("quads", l.quads);
        print_buf("hot4", l.hot4);
        print_buf("leaf9", l.leaf9);
        print_buf("naive_hot", l.naive_hot);
        unsigned long long ce;
        std::memcpy(&ce, &l.cull_extent, 8);
        std::printf("scalar stack_depth %d\nscalar pair_depth %d\nscalar quad_stack %d\nscalar root_ref %d\n"
                    "scalar ref_shift %d\nscalar pair_count %d\nscalar num_quads %d\nscalar no_tex %d\nscalar has_bvh %d\n"
                    "scalar variant %d\n",
                    l.stack_depth, l.pair_depth, l.quad_stack, l.root_ref, l.ref_shift, l.pair_count,
                    (int)(l.quads.size() / 8), (int)l.no_tex, (int)l.has_bvh, l.variant);
        std::printf("scalar root_lo %08x %08x %08x %08x\nscalar root_hi %08x %08x %08x %08x\n", fbits(l.root_lo.x),
                    fbits(l.root_lo.y), fbits(l.root_lo.z), fbits(l.root_lo.w), fbits(l.root_hi.x), fbits(l.root_hi.y),
                    fbits(l.root_hi.z), fbits(l.root_hi.w));
        std::printf("scalar cull_extent %016llx\n", ce);
        std::printf("scalar grid_lo %08x %08x %08x\nscalar grid_inv %08x %08x %08x\n", fbits(l.grid_lo[0]),
                    fbits(l.grid_lo[1]), fbits(l.grid_lo[2]), fbits(l.grid_inv[0]), fbits(l.grid_inv[1]), fbits(l.grid_inv[2]));
    }
    std::printf("rc=%d err=%s\n", rc, err.c_str());
    return rc;
}

// `layout FILE.json [key=value ...]` (kind null) / `layout-mutate FILE.json KIND`
static int check_layout(const char* path, const char* kind, int nkv, char** kv) {
    pth::LayoutParams p;
    for (int i = 0; i < nkv; ++i)
        if (!parse_param(kv[i], p)) {
            std::fprintf(stderr, "unknown layout parameter %s\n", kv[i]);
            return 2;
        }
    pt_scene_file* f = nullptr;
    const int rc = pt_scene_load_ex(path, -1, -1, -1, PT_SCENE_VIEWER_CAMERA, &f);
    if (rc != PT_OK) {
        std::printf("rc=%d err=%s\n", rc, pt_scene_last_error());
        return 1;
    }
    pt_scene_view v{};
    pt_scene_get_view(f, &v);
    std::vector<pt_bvh_node> nodes(v.bvh_nodes, v.bvh_nodes + v.num_bvh_nodes);
    std::vector<int32_t> idx(v.tri_indices, v.tri_indices + v.num_tri_indices);
    int ret = 0;
    if (kind) {
        if (!mutate_bvh(kind, v, nodes, idx)) {
            std::fprintf(stderr, "cannot apply mutation %s\n", kind);
            ret = 2;
        }
        v.bvh_nodes = nodes.data();
        v.tri_indices = idx.data();
    }
    if (ret == 0) print_layout(v, p);
    pt_scene_free(f);
    return ret;
}

static int check_png(const char* path) {
    int32_t w = 0, h = 0;
    int rc = pt_texture_load(path, &w, &h, nullptr, 0);
    if (rc == PT_OK) {
        std::vector<uint8_t> px((size_t)w * h * 4);
        rc = pt_texture_load(path, &w, &h, px.data(), (int64_t)px.size());
    }
    if (rc != PT_OK) std::printf("png rc=%d err=%s\n", rc, pt_scene_last_error());
    else std::printf("png rc=0 %d %d\n", w, h);
    return rc;
}

static int save_png(const char* out, int w, int h) {
    std::vector<float> img((size_t)w * h * 3);
    for (size_t i = 0; i < img.size(); ++i) img[i] = (float)((i * 37) % 300) / 7.0f - 3.0f;
    if (!img.empty()) img[0] = std::numeric_limits<float>::quiet_NaN();
    if (img.size() > 1) img[1] = std::numeric_limits<float>::infinity();
    if (img.size() > 2) img[2] = -std::numeric_limits<float>::infinity();
    const int rc = pt_save_png(img.data(), w, h, 3, out);
    std::printf("savepng rc=%d\n", rc);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s scene|png FILE... | savepng OUT W H | layout FILE [key=value ...] | "
                             "layout-mutate FILE KIND\n", argv[0]);
        return 2;
    }
    const std::string mode = argv[1];
    if (mode == "savepng" && argc == 5) return save_png(argv[2], std::atoi(argv[3]), std::atoi(argv[4])) == 0 ? 0 : 1;
    if (mode == "layout") return check_layout(argv[2], nullptr, argc - 3, argv + 3);
    if (mode == "layout-mutate" && argc == 4) return check_layout(argv[2], argv[3], 0, nullptr);
    for (int i = 2; i < argc; ++i) {
        std::printf("%s: ", argv[i]);
        if (mode == "scene") check_scene(argv[i]);
        else if (mode == "png") check_png(argv[i]);
        else return 2;
        std::fflush(stdout);
    }
    return 0;
}
