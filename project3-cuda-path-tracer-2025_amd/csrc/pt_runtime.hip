// pt_runtime.hip — the wavefront path tracer on MI355X: kernels, device buffers, frame loop
// and the C-ABI of include/pt/pathtrace_abi.h.
//
// The one translation unit with device code.  The kernels are in pt_*_kernels.h, the host runtime
// in rt_*.h (one file per concern, each saying what it owns and may call), included below in
// dependency order; this file keeps run_pass, pt_init / pt_free and the trace, image and stats
// entry points.
//
// Two pipelines render bit-identical images (the same per-path functions, pt_kernels.h):
//
//  FUSED (default): one kernel per bounce.  Bounce 0 generates the camera ray in registers;
//    every bounce intersects, shades, adds terminated paths into the image (the reference's
//    finalGather, done at termination — one add per pixel per frame either way) and compacts
//    survivors with a wave ballot + LDS block scan + one atomic per block into one of NSEG
//    output segments (segment = blockIdx % 8, i.e. one per XCD group) — no host round trip,
//    no per-bounce readback of the live count.
//
//  STAGED: one kernel per reference stage — camera, intersect, [material sort], shade,
//    compaction — each a separately testable HIP kernel.  Its compaction is a STABLE
//    partition in three order-independent launches — per-tile alive counts, one single-
//    workgroup scan of the tile counts, scatter (wave ballot/mbcnt within a tile) — the drop-in
//    for thrust::stable_partition(PathAlive) (pathtrace.cu:750-757).
//
// A frame is captured once into a hipGraph and replayed; the iteration number lives in
// device memory (k_frame_begin advances it), so the replay needs no parameter updates.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>   // types only: librccl.so is opened at run time (PT_COMBINE_RCCL)

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "pt/pathtrace_abi.h"
#include "pt/pt_denoise.h"
#include "pt/pt_naive_mesh.h"
#include "pt_kernels.h"
#include "pt_denoise_kernels.h"
#include "pt_naive_mesh_kernels.h"
#include "scene_layout.h"
#include "band_layout.h"
#include "tuning.h"
#include "worker.h"

using namespace ptd;

// =============================================================================================
// kernels (global scope, after the using-directive above)
// =============================================================================================
#include "pt_pass_kernels.h"
#include "pt_staged_kernels.h"

// =============================================================================================
// host runtime
// =============================================================================================
namespace {

#include "rt_core.h"
#include "rt_multi.h"
#include "rt_pass.h"
#include "rt_spec.h"
#include "rt_buffers.h"

CamDev to_camdev(const pt_camera& c) {
    CamDev d;
    d.resx = c.resolution.x;
    d.resy = c.resolution.y;
    d.position = f3{c.position.x, c.position.y, c.position.z};
    d.view = f3{c.view.x, c.view.y, c.view.z};
    d.up = f3{c.up.x, c.up.y, c.up.z};
    d.right = f3{c.right.x, c.right.y, c.right.z};
    d.plx = c.pixelLength.x;
    d.ply = c.pixelLength.y;
    d.aperture = c.aperture;
    d.focalDist = c.focalDist;
    return d;
}

// one pass: frames iter .. iter + batch - 1
int run_pass(int iter, int batch) {
    RC(ensure_frames(batch));
    // a single-frame pass (the API's pathtrace(), one call per frame) is launched directly: its six
    // kernels run back to back either way, and a graph launch costs the host ~10 us more before
    // its first kernel starts (tools/api_trace.py; PT_F1_GRAPH=1 keeps the graph, A/B)
    // Shards of a multi-device context replay their single-frame pass as a graph too: there the
    // host walks the shards one after another, and one graph launch per shard costs the host less
    // than six kernel launches (tools/multi_probe.py enqueue_us_per_shard)
    if (gp->opts.use_graph && (batch > 1 || gp->tune.f1_graph || (gp->multi && !gp->tune.multi_f1_direct))) {
        if (!gp->graph_exec[batch]) RC(build_graph(batch));
        // the graph's k_frame_begin advances the device iteration by one: preset iter - 1 (stream-
        // ordered) unless the last pass left it there -- main.cpp's pathtrace(pbo, 0, ++iteration)
        // calls then launch the graph alone
        if (gp->dev_iter != iter - 1) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&gp->d_ctl->iter, iter - 1, 1, gp->stream));
        HIPCHK(hipGraphLaunch(gp->graph_exec[batch], gp->stream));
    } else {
        RC(enqueue_pass(iter, batch));
    }
    gp->dev_iter = iter;
    gp->last_iter = iter + batch - 1;
    gp->frames_done += batch;
    return PT_OK;
}
int run_frame(int iter) { return run_pass(iter, 1); }

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
// NAIVE_MESH_LOADING (pt/pt_naive_mesh.h): what the next pt_init uses; -1 until first asked, then
// PT_NAIVE_MESH from the environment or what pt_set_naive_mesh stored
static int g_naive_next = -1;
static bool naive_next() {
    if (g_naive_next < 0) {
        const char* e = getenv("PT_NAIVE_MESH");
        g_naive_next = (e && strtol(e, nullptr, 10) == 1) ? 1 : 0;
    }
    return g_naive_next != 0;
}

extern "C" {

int32_t pt_abi_version(void) { return PT_ABI_VERSION; }

int32_t pt_set_naive_mesh(int32_t enabled) {
    g_naive_next = enabled ? 1 : 0;
    return PT_OK;
}
int32_t pt_get_naive_mesh(int32_t* next_init, int32_t* active) {
    if (next_init) *next_init = naive_next() ? 1 : 0;
    if (active) *active = (g_primary.inited && g_primary.naive) ? 1 : 0;
    return PT_OK;
}
int32_t pt_debug_naive_mesh_tile(void) { return NAIVE_TILE; }
const char* pt_last_error(void) { return g_err.c_str(); }

void pt_default_options(pt_options* o) {
    memset(o, 0, sizeof(*o));
    o->stream_compaction = 1;
    o->material_sort = 0;
    o->bvh = 1;
    o->arg_order = 0;
    // the naive mesh mode runs on the staged pipeline: with it on, that is the default, and a
    // PT_PIPELINE_FUSED reaching pt_init is the caller's own choice (refused there)
    o->pipeline = naive_next() ? PT_PIPELINE_STAGED : PT_PIPELINE_FUSED;
    o->use_graph = 1;
    o->device = 0;
    o->shard_mode = PT_SHARD_NONE;
    o->shard_rank = 0;
    o->shard_count = 1;
    o->shard_rows = 8;
    o->block_size = BLOCK;
    // fastest in the in-process A/B (tools/ab_variants.py); every variant is bit-identical
    o->variant = VAR_DEFAULT;
    o->frames_per_pass = 0;        // auto
    // several GPUs behind one pathtrace(): the drop-in and pt_render reach it through the environment
    o->num_devices = 0;
    for (int k = 0; k < PT_MAX_DEVICES; ++k) o->device_ids[k] = k;
    if (const char* e = getenv("PT_DEVICES")) {
        if (strchr(e, ',')) {
            int n = 0;
            for (const char* c = e; *c && n < PT_MAX_DEVICES;) {
                char* end = nullptr;
                const long v = strtol(c, &end, 10);
                if (end == c) break;
                o->device_ids[n++] = (int32_t)v;
                c = *end == ',' ? end + 1 : end;
                if (*end != ',') break;
            }
            o->num_devices = n;
        } else {
            o->num_devices = (int32_t)std::min<long>(PT_MAX_DEVICES, std::max<long>(0, strtol(e, nullptr, 10)));
        }
    }
    o->combine = PT_COMBINE_PEER;
    if (const char* e = getenv("PT_COMBINE")) o->combine = strcmp(e, "rccl") == 0 ? PT_COMBINE_RCCL : PT_COMBINE_PEER;
}

int32_t pt_init_data_container(int32_t* traced_depth) {
    gp->traced_depth = traced_depth;
    return PT_OK;
}

int32_t pt_free(void) {
    gp = &g_primary;
    if (M.n > 1) {
        multi_release();
        for (int k = M.n - 1; k >= 1; --k) {
            if (!M.shard[k]) continue;
            {   // whatever a shard allocated, also when its init_one failed part-way (inited false):
                // free_all releases only the buffers and stream that exist
                ShardScope sc(M.shard[k]);
                free_all();
            }
            delete M.shard[k];
        }
    }
    M = Multi();
    for (auto& h : g_copy_helpers) h.join();
    free_all();   // also resets g_primary's sizes (alloc_frames, capacity, ...) after a failed init
    return PT_OK;
}

// frames per pass when pt_options.frames_per_pass == 0: enough paths in flight to fill the
// chip in the late, mostly-terminated bounces (~84M paths at bounce 0), at most MAXF
int auto_batch(int local_pixels) {
    const int64_t target = gp->tune.auto_paths > 0 ? gp->tune.auto_paths : AUTO_BATCH_PATHS;
    int f = 1;
    while (f * 2 <= MAXF && (int64_t)local_pixels * f * 2 <= target) f *= 2;
    return f;
}

// one context (gp): the whole pathtraceInit for one device, or for shard k of a multi-device
// context; `share` contexts live on this device (auto F divides its free memory among them)
static int32_t init_one(const pt_scene_view* s, pt_options o, int share) {
    if (o.block_size != BLOCK) return fail(PT_E_UNSUPPORTED, "block_size must be %d", BLOCK);
    const int W = s->camera.resolution.x, H = s->camera.resolution.y;
    if (W <= 0 || H <= 0) return fail(PT_E_INVALID, "bad resolution %dx%d", W, H);
    if (s->trace_depth > MAXB) return fail(PT_E_UNSUPPORTED, "trace depth %d > %d", s->trace_depth, MAXB);
    if (s->num_geoms < 0 || s->num_materials < 0 || s->num_triangles < 0 || s->num_bvh_nodes < 0)
        return fail(PT_E_INVALID, "negative counts");
    if (s->num_materials > MAXMAT) return fail(PT_E_UNSUPPORTED, "more than %d materials", MAXMAT);
    // NAIVE_MESH_LOADING (pt/pt_naive_mesh.h): staged pipeline, one unsharded context
    const bool naive = naive_next();
    if (naive && o.pipeline == PT_PIPELINE_FUSED)
        return fail(PT_E_UNSUPPORTED, "naive mesh mode runs on the staged pipeline: pipeline = PT_PIPELINE_FUSED is not "
                    "supported (take pt_default_options after pt_set_naive_mesh(1), or set PT_PIPELINE_STAGED)");
    if (naive && o.shard_mode != PT_SHARD_NONE)
        return fail(PT_E_UNSUPPORTED, "naive mesh mode: one unsharded device context only (shard_mode must be PT_SHARD_NONE)");
    if (naive && s->num_triangles > 0 && !s->triangles) return fail(PT_E_INVALID, "triangles is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_E_NODEVICE, "no HIP device visible");
    if (o.device < 0 || o.device >= ndev) return fail(PT_E_INVALID, "device %d out of range", o.device);
    HIPCHK(hipSetDevice(o.device));
    gp->opts = o;
    gp->device = o.device;
    gp->tune = read_tuning();
    HIPCHK(hipStreamCreateWithFlags(&gp->stream, hipStreamNonBlocking));
    gp->width = W;
    gp->height = H;
    gp->pixels_total = W * H;
    // shard
    ShardDev sh{};
    sh.mode = o.shard_mode == PT_SHARD_PIXELS && o.shard_count > 1 ? 1 : 0;
    sh.rank = o.shard_rank;
    sh.count = std::max(1, o.shard_count);
    sh.rows = std::max(1, o.shard_rows);
    if (sh.mode == 1) {
        if (o.shard_rank < 0 || o.shard_rank >= o.shard_count) return fail(PT_E_INVALID, "bad shard rank");
        int rows = 0;
        for (int y = 0; y < H; ++y) rows += ((y / sh.rows) % sh.count) == sh.rank;
        sh.local_pixels = rows * W;
    } else {
        sh.local_pixels = gp->pixels_total;
    }
    gp->local_pixels = sh.local_pixels;
    if (o.frames_per_pass < 0 || o.frames_per_pass > MAXF)
        return fail(PT_E_INVALID, "frames_per_pass must be 0 (auto) .. %d", MAXF);

    // ---- scene -> the device buffers' byte images (host/scene_layout.cpp) ----
    pth::LayoutParams lp;
    lp.bvh = o.bvh != 0;
    lp.variant = o.variant;
    lp.naive = naive;
    lp.bvh_tree_ref = gp->tune.bvh_tree_ref;
    lp.bvh_tree_info = gp->tune.bvh_tree_info;
    lp.bvh_bfs_levels = gp->tune.bvh_bfs_levels;
    lp.bvh_quad = gp->tune.bvh_quad;
    lp.grid = gp->tune.grid;
    // the traversal kernels keep one stack entry per tree level in LDS (BLOCK x 4 B each): a tree of
    // height h needs (h + 1) KB per block, so the SAH tree's height is bounded to what still lets
    // BVH_WAVES blocks share a CU's 160 KB (21 levels; the 262k / 1.0M stand-ins' SAH trees are
    // 24 / 26 high unbounded: 6 / 5 blocks)
    lp.sah_max_height = gp->tune.bvh_max_height > 0 ? gp->tune.bvh_max_height
                        : gp->tune.bvh_max_height == 0
                            ? (1 << 30)
                            : (int)(163840 / ((size_t)BVH_WAVES * BLOCK * sizeof(int))) - 1;
    pth::SceneLayout L;
    {
        std::string err;
        const int32_t rc = pth::build_scene_layout(*s, lp, L, err);
        if (rc != PT_OK) return fail(rc, "%s", err.c_str());
    }
    o.variant = L.variant;   // minus the near-first traversals, for a tree they cannot walk
    gp->opts.variant = o.variant;
    gp->no_tex = L.no_tex;
    gp->naive = naive;
    gp->has_bvh = L.has_bvh;
    gp->stack_depth = L.stack_depth;
    gp->pair_depth = L.pair_depth;
    if (gp->has_bvh) gp->bvh_lds = (size_t)gp->stack_depth * BLOCK * sizeof(int);
    // VAR_BVH_SPLIT needs the pair layout, the fast traversal and an LDS geom table
    gp->split = gp->has_bvh && !L.pairs.empty() && o.pipeline == PT_PIPELINE_FUSED && (o.variant & VAR_BVH_SPLIT) &&
              (o.variant & VAR_BVH_FAST) && (o.variant & (VAR_CAND_QUEUE | VAR_WAVE_REDIST)) &&
              s->num_geoms <= LDS_GEOMS;
    // MATERIAL_SORTING on the fused pipeline: the block-local regrouping by material (VAR_MAT_GROUP;
    // keys are the material ids, at most MG_KEYS - 1 of them), for the kernel variants built with it
    if (o.material_sort && o.pipeline == PT_PIPELINE_FUSED && s->num_materials <= MG_KEYS - 1 &&
        variant_compiled(effective_variant(true, o.variant | VAR_MAT_GROUP)) &&
        variant_compiled(effective_variant(false, o.variant | VAR_MAT_GROUP))) {
        o.variant |= VAR_MAT_GROUP;
        gp->opts.variant = o.variant;
    }
    if (o.pipeline == PT_PIPELINE_FUSED) {
        for (int first = 0; first < 2; ++first) {
            const int v = effective_variant(first != 0, o.variant);
            if (!variant_compiled(v))
                return fail(PT_E_UNSUPPORTED, "variant %d (effective %d for the %s bounce) is not compiled in", o.variant,
                            v, first ? "camera" : "later");
        }
    }
    gp->num_tex = (s->num_textures > 0 && s->textures) ? s->num_textures : 0;
    gp->sc.num_mats = s->num_materials;
    // frames per pass: as asked, or auto (~84M paths), halved while the per-pass buffers would
    // take more than half of the device memory free now.  Buffers are allocated when a pass of
    // that size is first traced or prepared (ensure_frames), not here.
    if (o.frames_per_pass > 0) {
        gp->batch = o.frames_per_pass;
    } else {
        gp->batch = auto_batch(gp->local_pixels);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (gp->batch > 1 && pass_bytes(gp->batch, o.pipeline == PT_PIPELINE_STAGED) > free_b / (2 * (size_t)share))
                gp->batch /= 2;
    }
    if ((int64_t)gp->local_pixels * gp->batch > (1 << 28)) return fail(PT_E_UNSUPPORTED, "wavefront too large");

    // ---- one device buffer per vector the layout filled ----
    auto to_device = [](auto** d, const auto& h) {
        RC(dalloc(d, h.size()));
        return upload(*d, h.data(), h.size());
    };
    RC(to_device(&gp->d_geoms, L.geoms));
    RC(to_device(&gp->d_cull, L.culls));
    RC(to_device(&gp->d_mats, L.mats));
    RC(to_device(&gp->d_grid, L.grid));
    RC(to_device(&gp->d_nodes, L.nodes));
    RC(to_device(&gp->d_node_aux, L.node_aux));
    RC(to_device(&gp->d_hot, L.hot));
    RC(to_device(&gp->d_cold, L.cold));
    RC(to_device(&gp->d_pairs, L.pairs));
    RC(to_device(&gp->d_hot4, L.hot4));
    RC(to_device(&gp->d_leaf9, L.leaf9));
    RC(to_device(&gp->d_quads, L.quads));
    RC(to_device(&gp->d_naive_hot, L.naive_hot));
    // textures (pathtrace.cu:169-201): RGBA8 texels of every texture in one buffer
    int num_tex = 0;
    if (s->num_textures > 0 && s->textures) {
        std::vector<int4> info(s->num_textures);
        size_t total = 0;
        for (int i = 0; i < s->num_textures; ++i) {
            const pt_texture& t = s->textures[i];
            if (t.width <= 0 || t.height <= 0 || !t.data || t.channels != 4)
                return fail(PT_E_INVALID, "texture %d: need RGBA8 data (channels 4)", i);
            info[i] = make_int4((int)total, t.width, t.height, 0);
            total += (size_t)t.width * t.height;
        }
        if (total > (size_t)INT32_MAX) return fail(PT_E_UNSUPPORTED, "texture data too large");
        RC(dalloc(&gp->d_texels, total));
        RC(dalloc(&gp->d_texinfo, info.size()));
        for (int i = 0; i < s->num_textures; ++i) {
            const pt_texture& t = s->textures[i];
            HIPCHK(smemcpy(gp->d_texels + info[i].x, t.data, (size_t)t.width * t.height * 4, hipMemcpyHostToDevice));
        }
        RC(upload(gp->d_texinfo, info.data(), info.size()));
        num_tex = s->num_textures;
    }
    RC(dalloc(&gp->d_image, (size_t)gp->pixels_total * 3));
    HIPCHK(smemset(gp->d_image, 0, sizeof(float) * 3 * (size_t)gp->pixels_total));
    RC(dalloc(&gp->d_ctl, 1));
    RC(ctl_reset());
    gp->key_bits = 1;
    while ((1 << gp->key_bits) < std::max(2, s->num_materials)) gp->key_bits++;

    SceneDev& sc = gp->sc;
    sc.geoms = gp->d_geoms;
    sc.cull = gp->d_cull;
    sc.mats = gp->d_mats;
    sc.nodes = gp->d_nodes;
    sc.node_aux = gp->d_node_aux;
    sc.hot = gp->d_hot;
    sc.cold = gp->d_cold;
    sc.num_geoms = s->num_geoms;
    sc.num_mats = s->num_materials;
    sc.num_nodes = gp->has_bvh ? s->num_bvh_nodes : 0;
    sc.num_tris = s->num_triangles;
    sc.trace_depth = s->trace_depth;
    sc.arg_order = o.arg_order;
    sc.use_bvh = gp->has_bvh ? 1 : 0;
    sc.stack_depth = gp->stack_depth;
    // the pair traversal pushes at most one entry per level of its hierarchy (never more than the
    // stack_depth the other traversals size their stacks for); k_bvh_bounce's LDS stack is sized
    // by it
    sc.pair_stack_depth = gp->pair_depth > 0 ? std::min(gp->pair_depth, gp->stack_depth) : gp->stack_depth;
    // the split kernels' LDS stack: all of it, or its first bvh_stack_lds entries and a spill row per
    // queue slot for the rest
    sc.stack_lds = gp->split && gp->tune.bvh_stack_lds > 0 ? std::min(gp->tune.bvh_stack_lds, sc.pair_stack_depth)
                                                           : sc.pair_stack_depth;
    sc.spill_stride = sc.pair_stack_depth - sc.stack_lds;
    sc.spill = nullptr;   // allocated with the traversal queue (ensure_frames)
    sc.cam = to_camdev(s->camera);
    sc.shard = sh;
    sc.contrib = gp->d_contrib;
    sc.texels = gp->d_texels;
    sc.texinfo = gp->d_texinfo;
    sc.num_textures = num_tex;
    sc.pairs = gp->d_pairs;
    sc.hot4 = gp->d_hot4;
    sc.leaf9 = gp->d_leaf9;
    sc.num_pairs = L.pair_count;
    sc.quads = gp->split ? gp->d_quads : nullptr;   // the 4-wide records serve the traversal kernels only
    sc.num_quads = (int)(L.quads.size() / 8);
    sc.root_ref = L.root_ref;
    sc.ref_shift = L.ref_shift;
    sc.root_lo = L.root_lo;
    sc.root_hi = L.root_hi;
    // node_aux's c = 64 2^-24 sx^2 / 1e-5, stored x 1.01, and cE = c x extent x 1.01: the same
    // bounds from s = sx on the device, rounded up
    sc.cull_c0 = (float)(64.0 * std::ldexp(1.0, -24) / 1e-5 * 1.01 * (1.0 + 1e-5));
    sc.cull_E = (float)(L.cull_extent * (1.0 + 1e-5));
    sc.grid = gp->d_grid;
    sc.grid_all = s->num_geoms >= 64 ? ~0ull : ((1ull << s->num_geoms) - 1);
    for (int a = 0; a < 3; ++a) {
        sc.grid_lo[a] = L.grid_lo[a];
        sc.grid_inv[a] = L.grid_inv[a];
    }
    RC(ensure_frames(1));            // one frame's wavefront now; larger passes grow it on first use
    gp->inited = true;
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int32_t pt_init(const pt_scene_view* s, const pt_options* opts_in) {
    if (!s) return fail(PT_E_INVALID, "scene is NULL");
    pt_free();
    pt_options o;
    if (opts_in) o = *opts_in;
    else pt_default_options(&o);
    if (o.num_devices < 0 || o.num_devices > PT_MAX_DEVICES)
        return fail(PT_E_INVALID, "num_devices must be 0 .. %d", PT_MAX_DEVICES);
    if (naive_next() && o.num_devices > 1)
        return fail(PT_E_UNSUPPORTED, "naive mesh mode: one device context only (pt_options.num_devices > 1)");
    if (o.num_devices <= 1) {
        const int rc = init_one(s, o, 1);
        if (rc != PT_OK) free_all();   // whatever was allocated before the failure
        return rc;
    }
    const int n = o.num_devices;
    if (o.shard_mode != PT_SHARD_NONE)
        return fail(PT_E_INVALID, "num_devices > 1 splits the frame itself; shard_mode must be PT_SHARD_NONE");
    if (o.combine != PT_COMBINE_PEER && o.combine != PT_COMBINE_RCCL) return fail(PT_E_INVALID, "bad combine");
    const int H = s->camera.resolution.y, rows = std::max(1, o.shard_rows);
    if (H > 0 && (H + rows - 1) / rows < n)
        return fail(PT_E_INVALID, "%d shards but only %d row bands of %d rows", n, (H + rows - 1) / rows, rows);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_E_NODEVICE, "no HIP device visible");
    for (int k = 0; k < n; ++k)
        if (o.device_ids[k] < 0 || o.device_ids[k] >= ndev)
            return fail(PT_E_INVALID, "device_ids[%d] = %d out of range (%d devices)", k, o.device_ids[k], ndev);
    M.n = n;
    M.combine = o.combine;
    int rc = PT_OK;
    for (int k = 0; k < n && rc == PT_OK; ++k) {
        M.shard[k] = k == 0 ? &g_primary : new State();
        pt_options ok = o;
        ok.num_devices = 1;
        ok.device = o.device_ids[k];
        ok.shard_mode = PT_SHARD_PIXELS;
        ok.shard_rank = k;
        ok.shard_count = n;
        ok.shard_rows = rows;
        int share = 0;
        for (int j = 0; j < n; ++j) share += o.device_ids[j] == o.device_ids[k];
        ShardScope sc(M.shard[k]);
        rc = init_one(s, ok, share);
        gp->multi = true;
    }
    if (rc == PT_OK) rc = multi_setup();
    if (rc != PT_OK) {
        const std::string err = g_err;
        pt_free();
        g_err = err;
        return rc;
    }
    HIPCHK(hipSetDevice(g_primary.device));
    return PT_OK;
}

int32_t pt_set_camera(const pt_camera* c) {
    RC(need_init());
    if (!c || c->resolution.x != gp->width || c->resolution.y != gp->height)
        return fail(PT_E_INVALID, "camera resolution must match pt_init");
    const CamDev nc = to_camdev(*c);
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        if (memcmp(&nc, &gp->sc.cam, sizeof nc) != 0) {
            RC(spec_cancel());                          // traced with the old camera
            HIPCHK(hipStreamSynchronize(gp->stream));   // a replayed pass may still hold the graph
            gp->sc.cam = nc;
            gp->gbuf_valid = false;   // the feature planes show the old camera's first hits
            release_graph();   // kernel arguments changed
        }
    }
    return PT_OK;
}

int32_t pt_set_trace_depth(int32_t depth) {
    RC(need_init());
    if (depth < 0 || depth > MAXB) return fail(PT_E_UNSUPPORTED, "trace depth %d not in 0 .. %d", depth, MAXB);
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        if (gp->sc.trace_depth != depth) {
            RC(spec_cancel());
            HIPCHK(hipStreamSynchronize(gp->stream));
            gp->sc.trace_depth = depth;
            release_graph();   // the bounce count is baked into the captured passes
        }
    }
    return PT_OK;
}

int32_t pt_debug_spec_counts(int64_t* launched, int64_t* adopted) {
    RC(need_init());
    int64_t l = 0, a = 0;
    for (int k = 0; k < nshards(); ++k) {
        l += shard_ctx(k)->spec_launched;
        a += shard_ctx(k)->spec_adopted;
    }
    if (launched) *launched = l;
    if (adopted) *adopted = a;
    return PT_OK;
}

int32_t pt_set_speculation(int32_t enabled) {
    RC(need_init());
    State* p = &g_primary;
    if (!enabled) RC(spec_cancel_all());
    p->tune.speculate = enabled != 0;
    return PT_OK;
}

int32_t pt_trace(pt_uchar4* pbo, int32_t frame, int32_t iteration, float* host_image) {
    (void)frame;   // unused by the reference too (pathtrace.cu:639)
    RC(need_init());
    if (iteration <= 0) return fail(PT_E_INVALID, "iteration is 1-based (main.cpp:458), got %d", iteration);
    // speculate only for callers that copy the image out (main.cpp's pathtrace() always does): a
    // call without the copy has nothing for the next frame to overlap with.  Several devices: every
    // shard speculates its own pixels; the call for N + 1 takes each shard's frame over, then
    // combines as usual (the host copy reads the combined image, so it waits for the combine)
    const bool spec = spec_enabled() && (host_image != nullptr || gp->spec_iter == iteration);
    const bool single = M.n <= 1;
    const bool bands_on = !single && M.band_copy && host_image;
    bool adopted = false;
    const int sum_idx = gp->spec_sum_idx;   // the taken-over frame's image, before the next launch flips it
    BandCopy bands[PT_MAX_DEVICES];
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        if (spec && gp->spec_iter == iteration) {
            adopted = true;
            const float* sum = gp->d_spec_sum[gp->spec_sum_idx];
            RC(spec_adopt(host_image != nullptr && single));   // traced already, during the previous call's copy
            // several devices: this shard's bands of the finished sum (the speculative stream has it)
            if (bands_on) RC(band_prepare(bands[k], host_image, sum, gp->spec_stream));
        } else {
            RC(spec_cancel());
            RC(run_frame(iteration));
            if (bands_on) RC(band_prepare(bands[k], host_image, gp->d_image, gp->stream));
        }
        if (g_primary.traced_depth) RC(frame_depth_enqueue());   // read after the one sync below
    }
    RC(multi_combine());
    if (pbo) {
        hipLaunchKernelGGL(k_to_pbo, dim3(nblocks(gp->pixels_total)), dim3(BLOCK), 0, gp->stream, gp->d_image, pbo,
                           gp->pixels_total, iteration);
        HIPCHK(hipGetLastError());
    }
    // the next frame, on the second stream, while this one's image is copied out (queued before
    // the copy: a copy into pageable memory may hold the host until it is done)
    if (spec && host_image && iteration < INT32_MAX) RC(spec_launch(iteration + 1));
    if (bands_on) {
        // every shard's row bands from its own device, side by side (shard 0's on this thread)
        for (int k = 1; k < nshards(); ++k) g_copy_helpers[k].post(bands[k]);
        hipError_t e = bands[0].run();
        for (int k = 1; k < nshards(); ++k) {
            const hipError_t ek = g_copy_helpers[k].wait();
            if (e == hipSuccess) e = ek;
        }
        HIPCHK(hipSetDevice(g_primary.device));
        HIPCHK(e);
    } else if (host_image) {
        // the caller's pageable memory, as cudaMemcpy(state.image) (pathtrace.cu:783).  It is not
        // page-locked: a registration would outlive a caller that frees the buffer and gets a new
        // one at the same address, and on MI355X the pageable copy runs at the pinned rate anyway
        // (tools/copy_probe.py: 7.68 MB in 0.145 ms either way)
        const size_t bytes = sizeof(float) * 3 * (size_t)gp->pixels_total;
        if (adopted && single)   // the speculated frame's finished sum, on the copy stream (it waited for it)
            HIPCHK(hipMemcpyAsync(host_image, gp->d_spec_sum[sum_idx], bytes, hipMemcpyDeviceToHost, gp->copy_stream));
        else
            HIPCHK(hipMemcpyAsync(host_image, gp->d_image, bytes, hipMemcpyDeviceToHost, gp->stream));
    }
    // one wait: the first device's stream waited for every shard's frame (multi_combine), and each
    // shard queued its counter copy before that
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (adopted && single && host_image) HIPCHK(hipStreamSynchronize(gp->copy_stream));
    if (gp->traced_depth) {
        // GuiDataContainer::TracedDepth = the bounces the frame ran (pathtrace.cu:759-770); with
        // shards, the frame ran as long as its longest shard
        int depth = 0;
        for (int k = 0; k < nshards(); ++k) {
            ShardScope sc(shard_ctx(k));
            depth = std::max(depth, frame_depth_read());
        }
        *gp->traced_depth = depth;
    }
    return PT_OK;
}

int32_t pt_trace_frames(int32_t first_iteration, int32_t count) {
    RC(need_init());
    RC(spec_cancel_all());
    if (first_iteration <= 0 || count < 0) return fail(PT_E_INVALID, "bad iteration range");
    // passes of gp->batch frames (bit-identical to frame-by-frame: k_combine keeps the order);
    // every shard's passes are queued before the combine, so the devices trace concurrently
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        for (int i = 0; i < count;) {
            const int f = pass_frames(count - i);
            RC(run_pass(first_iteration + i, f));
            i += f;
        }
    }
    return count > 0 ? multi_combine() : PT_OK;
}

int32_t pt_prepare_frames(int32_t count) {
    RC(need_init());
    RC(spec_cancel_all());
    if (count < 0) return fail(PT_E_INVALID, "bad count");
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        RC(ensure_frames(count > 0 ? pass_frames(count) : 1));   // the largest pass of the run comes first
        if (!gp->opts.use_graph) continue;
        // the pass sizes pt_trace_frames(., count) will replay
        for (int i = 0; i < count;) {
            const int f = pass_frames(count - i);
            if (!gp->graph_exec[f]) RC(build_graph(f));
            i += f;
        }
    }
    return PT_OK;
}

int32_t pt_synchronize(void) {
    RC(need_init());
    HIPCHK(g_spec_launcher.wait());
    for (int k = 0; k < nshards(); ++k) {   // speculated frames (their streams stay valid)
        State* s = shard_ctx(k);
        if (!s->spec_stream) continue;
        ShardScope sc(s);
        HIPCHK(hipStreamSynchronize(s->spec_stream));
    }
    for (int k = nshards() - 1; k >= 0; --k) {
        ShardScope sc(shard_ctx(k));
        HIPCHK(hipStreamSynchronize(gp->stream));
    }
    return PT_OK;
}

int32_t pt_get_image(float* host_out, int64_t n_floats) {
    RC(need_init());
    if (!host_out || n_floats < (int64_t)gp->pixels_total * 3) return fail(PT_E_INVALID, "image buffer too small");
    HIPCHK(hipStreamSynchronize(gp->stream));
    HIPCHK(smemcpy(host_out, gp->d_image, sizeof(float) * 3 * (size_t)gp->pixels_total, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t pt_get_image_device(void** device_ptr, int64_t* n_floats) {
    RC(need_init());
    // the caller may write through the pointer before the next pt_trace: a speculated next frame
    // summed from the image as it is now would then overwrite that write, so it is dropped here
    RC(spec_cancel_all());
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (device_ptr) *device_ptr = gp->d_image;
    if (n_floats) *n_floats = (int64_t)gp->pixels_total * 3;
    return PT_OK;
}

int32_t pt_set_image(const float* host_in, int64_t n_floats) {
    RC(need_init());
    RC(spec_cancel_all());   // its image + plane was formed from the image being replaced
    if (!host_in || n_floats != (int64_t)gp->pixels_total * 3) return fail(PT_E_INVALID, "image size mismatch");
    for (int k = 0; k < nshards(); ++k) {   // each shard keeps accumulating into its own pixels of it
        ShardScope sc(shard_ctx(k));
        HIPCHK(hipStreamSynchronize(gp->stream));
        HIPCHK(smemcpy(gp->d_image, host_in, sizeof(float) * (size_t)n_floats, hipMemcpyHostToDevice));
    }
    return PT_OK;
}

// device buffers for callers without the HIP headers (the headless viewer's PBO, ctypes)
int32_t pt_device_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return fail(PT_E_INVALID, "pt_device_alloc: bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_E_NODEVICE, "no HIP device visible");
    HIPCHK(hipMalloc(out, (size_t)bytes));
    return PT_OK;
}

int32_t pt_device_free(void* p) {
    if (p) HIPCHK(hipFree(p));
    return PT_OK;
}

int32_t pt_device_read(void* host_dst, const void* device_src, int64_t bytes) {
    if (!host_dst || !device_src || bytes < 0) return fail(PT_E_INVALID, "pt_device_read: bad argument");
    if (gp->stream) HIPCHK(hipStreamSynchronize(gp->stream));
    HIPCHK(smemcpy(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

// the current context's counters
static int32_t frame_stats(pt_frame_stats* out) {
    HIPCHK(hipStreamSynchronize(gp->stream));
    FrameCtl ctl;
    HIPCHK(smemcpy(&ctl, gp->d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->iteration = ctl.iter;
    out->bounces = std::max(1, gp->sc.trace_depth);
    out->pixels = gp->local_pixels;
    for (int b = 0; b < out->bounces; ++b) {
        int64_t s = 0;
        if (gp->opts.pipeline == PT_PIPELINE_STAGED && !gp->opts.stream_compaction) {
            s = b == 0 ? ctl.cnt[0][0][0] : -1;   // no compaction: the live count is never formed
        } else {
            for (int k = 0; k < NSEG; ++k) s += ctl.cnt[b][k][0];
        }
        out->live[b] = s;
        if (s > 0) out->segments += s;
    }
    out->frames_total = (int64_t)ctl.frames;
    out->frames_per_pass = gp->batch;
    out->last_pass_frames = ctl.batch;
    for (int b = 0; b <= MAXB; ++b) {
        int64_t cur = 0;
        for (int k = 0; k < NSEG; ++k) cur += ctl.cnt[b][k][0];
        out->live_total[b] = (int64_t)ctl.tot[b] + (ctl.frames > 0 ? cur : 0);
        int64_t q = 0;
        for (int k = 0; k < NSEG; ++k) q += ctl.qcnt[b][k][0];
        out->queued_total[b] = (int64_t)ctl.qtot[b] + (ctl.frames > 0 ? q : 0);
        int64_t h = 0, hs = 0;
        for (int k = 0; k < NSEG; ++k) {
            h += ctl.qcnt[b][k][3];
            hs += ctl.qcnt[b][k][4];
        }
        out->handed_total[b] = (int64_t)ctl.htot[b] + (ctl.frames > 0 ? h : 0);
        out->handed_stack_total[b] = (int64_t)ctl.hstk[b] + (ctl.frames > 0 ? hs : 0);
        if (b < out->bounces) out->segments_total += out->live_total[b];
    }
    return PT_OK;
}

int32_t pt_get_frame_stats(pt_frame_stats* out) {
    RC(need_init());
    if (!out) return fail(PT_E_INVALID, "NULL");
    RC(frame_stats(out));
    for (int k = 1; k < nshards(); ++k) {   // shards: the counts of every shard's pixels
        pt_frame_stats s;
        {
            ShardScope sc(shard_ctx(k));
            RC(frame_stats(&s));
        }
        out->pixels += s.pixels;
        out->segments += s.segments;
        out->segments_total += s.segments_total;
        for (int b = 0; b < 64; ++b) out->live[b] += s.live[b];
        for (int b = 0; b <= MAXB; ++b) {
            out->live_total[b] += s.live_total[b];
            out->queued_total[b] += s.queued_total[b];
            out->handed_total[b] += s.handed_total[b];
            out->handed_stack_total[b] += s.handed_stack_total[b];
        }
    }
    return PT_OK;
}

int32_t pt_reset_stats(void) {
    RC(need_init());
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        HIPCHK(hipStreamSynchronize(gp->stream));
        RC(ctl_reset());
    }
    return PT_OK;
}

#include "rt_abi_denoise.h"
#include "rt_abi_test.h"

}  // extern "C"
