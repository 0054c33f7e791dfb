// rt_core.h — the base of the host runtime (a part of pt_runtime.hip's one translation unit,
// inside its anonymous namespace; every rt_*.h is).
//
// Owns: the error string and the RC / HIPCHK return macros, dalloc / dfree, the per-context State
// with the current-context pointer gp, the stream-ordered memset / memcpy, ctl_reset, need_init,
// and launch() with the per-dispatch profiling records.
// Calls: HIP only.  Every other rt_*.h builds on this file; it knows none of them.
using pth::Tuning;        // host/tuning.h: the knobs, read from the environment in read_tuning() alone
using pth::read_tuning;

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define RC(x)                      \
    do {                           \
        int rc_ = (x);             \
        if (rc_ != PT_OK) return rc_; \
    } while (0)
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(PT_E_HIP, "%s:%d: %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
int dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) return PT_OK;
    HIPCHK(hipMalloc((void**)p, n * sizeof(T)));
    return PT_OK;
}

template <class T>
void dfree(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

constexpr int MAXF = 256;                   // frames per pass, upper bound (slot: 8 bits of a queue entry)
// auto F: up to ~84M paths at bounce 0 -> 800x800: F = 128, 1600x1600: F = 32.  A/B (ms/frame):
// cornell 800^2 F = 8 0.0992, 16 0.0949 (0.0937), 32 0.0921; bunny 800^2 F = 8 0.685, 16 0.633;
// khaslana 1600^2 F = 2 2.52, 4 1.95 (1.93), 8 1.66 (earlier kernels: F = 1 0.214, 2 0.161,
// 4 0.137, 8 0.129).  Round 2 (tools/autof_ab.sh, target 21M / 42M / 84M paths): khaslana
// 1600^2 d12 1.38 / 1.27 / 1.23, bunny 0.397 / 0.388 / 0.391, cornell flat.  ~16 GB of path
// buffers + 5.2 GB traversal queue at 1600^2, F = 32 (of 288 GB).
constexpr int64_t AUTO_BATCH_PATHS = 84000000;

struct State {
    bool inited = false;
    Tuning tune;
    pt_options opts{};
    int device = 0;
    hipStream_t stream = nullptr;
    SceneDev sc{};
    int width = 0, height = 0, pixels_total = 0, local_pixels = 0;
    // per-pass buffers are sized lazily (ensure_frames): a caller that only ever traces single
    // frames (the drop-in pathtrace(), the viewer) holds one frame's worth, not a whole pass's
    int seg_stride = 0, capacity = 0;
    int alloc_frames = 0;            // frames per pass the path buffers / queue / planes hold now
    bool staged_alloc = false;       // hit / alive / permutation / tile buffers at `capacity`
    int num_tex = 0;
    bool has_bvh = false;
    int stack_depth = 0;
    int pair_depth = 0;              // entries the pair traversal needs: height of its hierarchy + 1
    size_t bvh_lds = 0;
    // device buffers
    DevGeom* d_geoms = nullptr;
    DevCull* d_cull = nullptr;
    DevMaterial* d_mats = nullptr;
    float4* d_node_aux = nullptr;
    DevNode* d_nodes = nullptr;
    DevTriHot* d_hot = nullptr;
    DevPair* d_pairs = nullptr;
    float4* d_quads = nullptr;       // the 4-wide layout (SceneDev::quads), trees past the L2
    DevTriHot* d_hot4 = nullptr;
    float4* d_leaf9 = nullptr;
    DevTriCold* d_cold = nullptr;
    bool naive = false;              // NAIVE_MESH_LOADING mode (pt/pt_naive_mesh.h): k_naive_mesh, no BVH
    DevTriHot* d_naive_hot = nullptr;    // its triangle-ordered positions (allocated in that mode only)
    float4* d_path[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    float4* d_hit_nt = nullptr;
    int* d_hit_mat = nullptr;
    float4* d_hit_uvd0 = nullptr;    // textured scenes only
    float4* d_hit_uvd1 = nullptr;
    uint32_t* d_texels = nullptr;
    int4* d_texinfo = nullptr;
    int* d_alive = nullptr;
    int* d_perm = nullptr;
    int* d_tile_hist = nullptr;
    int* d_tile_cnt = nullptr;
    int* d_tile_off = nullptr;
    float* d_image = nullptr;
    FrameCtl* d_ctl = nullptr;
    float* d_contrib = nullptr;      // passes of F > 1 frames: F planes of pixels_total float3
    unsigned long long* d_grid = nullptr;   // the pre-test's candidate table (scene_layout.cpp, build_candidate_table)
    int batch = 1;                   // frames per pass (pt_options.frames_per_pass, resolved)
    bool split = false;              // VAR_BVH_SPLIT active (fused, fast BVH on the pair layout)
    bool no_tex = false;             // no textured / bump-mapped material (VAR_NO_TEX kernels)
    QueueBuf queue{};                // its traversal queue (capacity: one pass's paths)
    TailBuf tail{};                  // the traversals k_bvh_bounce hands to k_bvh_tail_trav
    int tail_lanes = 0;              // bvh_tail_lanes()
    int tail_refill = 16, tail_trav_blocks = 224, tail_shade_blocks = 512;   // PT_BVH_TAIL_REFILL / _TRAV_BLOCKS / _SHADE_BLOCKS
    int tail_depth = 0;              // stack entries per handed-over traversal
    // one captured pass per pass size (1..MAXF frames)
    hipGraph_t graph[MAXF + 1] = {};
    hipGraphExec_t graph_exec[MAXF + 1] = {};
    int last_iter = 0;
    int dev_iter = 0;                // FrameCtl::iter after the passes queued so far (0 after a reset)
    int ctl_rows = 1;                // counter rows k_frame_begin folds / clears (max trace depth + 1)
    int frames_done = 0;
    int32_t* traced_depth = nullptr;
    int* h_cnt = nullptr;            // page-locked copy of the live counters (TracedDepth, frame_depth_*)
    // single-frame speculation (pt_trace, spec_*): frame N + 1 traced into a plane of its own on a
    // second stream while frame N's image crosses PCIe to the caller
    hipStream_t spec_stream = nullptr;
    hipEvent_t spec_ev_in = nullptr;      // gp->stream: what the speculative frame follows
    hipEvent_t spec_ev_done = nullptr;    // spec_stream: the speculative frame is finished
    FrameCtl* d_ctl_spec = nullptr;       // its own counters (d_ctl keeps the caller's frame)
    float* d_spec_plane = nullptr;        // its contributions, one float3 per pixel
    float* d_spec_sum[2] = {nullptr, nullptr};   // image + plane, formed at its end (alternating)
    int spec_sum_idx = 0;                 // the buffer the pending speculative frame writes
    hipStream_t copy_stream = nullptr;    // the host copy of a taken-over frame's image
    hipStream_t band_stream = nullptr;    // several devices: the host copy of this shard's row bands
    hipEvent_t band_ready = nullptr;      // ... what it follows (the shard's frame)
    hipGraph_t spec_graph = nullptr;      // its pass, captured once (released with the pass graphs)
    hipGraphExec_t spec_exec = nullptr;
    int spec_iter = 0;                    // iteration of the queued speculative frame (0: none)
    int64_t spec_launched = 0, spec_adopted = 0;   // speculated frames queued / taken over (pt_debug_spec_counts)
    int spec_dev_iter = 0;                // d_ctl_spec->iter after the speculative frames queued so far
    int key_bits = 1;
    bool multi = false;              // a shard context of a multi-device pt_init
    // denoiser (pt/pt_denoise.h): feature planes + colour ping-pong, allocated by the first capture
    float4* d_gbuf[3] = {nullptr, nullptr, nullptr};   // normal | t, position | hit, albedo | material
    float4* d_dn_color[2] = {nullptr, nullptr};
    bool gbuf_valid = false;         // captured with the current camera
    hipEvent_t dn_ev[PT_DENOISE_MAX_LEVELS + 3] = {};   // pt_debug_denoise_timing: capture 0-1, levels 2..
    float dn_capture_ms = 0.f, dn_ms = 0.f, dn_level_ms[PT_DENOISE_MAX_LEVELS] = {};
};
State g_primary;                 // the process's context (shard 0 of a multi-device context)
State* gp = &g_primary;          // the context the host runtime works on now (see ShardScope)

// Host <-> device copies and memsets of the runtime, ordered on the library's stream and
// completed before returning.  gp->stream is a non-blocking stream: the legacy null stream that
// plain hipMemset / hipMemcpy use does not order against it, so a memset of FrameCtl could land
// after a kernel enqueued behind it on gp->stream (pt_test_camera saw a zeroed path count).
hipError_t smemset(void* p, int v, size_t n) {
    hipError_t e = hipMemsetAsync(p, v, n, gp->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(gp->stream);
}
hipError_t smemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, n, kind, gp->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(gp->stream);
}

PathBuf pathbuf(int i) { return PathBuf{gp->d_path[i][0], gp->d_path[i][1], gp->d_path[i][2]}; }

// zero the frame control block (counters, totals, the device iteration)
int ctl_reset() {
    const hipError_t e = smemset(gp->d_ctl, 0, sizeof(FrameCtl));
    if (e != hipSuccess) return fail(PT_E_HIP, "FrameCtl reset: %s", hipGetErrorString(e));
    gp->dev_iter = 0;
    return PT_OK;
}

int need_init() { return gp->inited ? PT_OK : fail(PT_E_STATE, "pt_init has not been called"); }

// pt_profile_frames: every kernel of the frame is launched with hipExtLaunchKernel's start/stop
// events, which take their timestamps from that dispatch packet itself -- the kernel's own
// execution time, independent of how far ahead of the GPU the host is.
struct ProfRec {
    int kind;            // -1 frame begin, 0 camera, 1 intersect, 2 shade, 3 compact scatter,
                         // 4 material sort, 5 compact count+scan, 7 naive mesh loop, 100+b fused bounce b,
                         // 200+b its split BVH traversal kernel, 300+b k_tail from bounce b
    hipEvent_t start, stop;
};
// The per-dispatch events skip the system-scope fence a default event performs when it is
// recorded: that fence writes back and invalidates L2 around every profiled kernel, which made
// the eager replay's k_bounce launches ~18 % longer than the same launches in the timed graph
// replay (rocprofv3 kernel trace, cornell 800^2 F = 20: 0.221 vs 0.188 ms per launch).  The
// kernels run on one stream and are ordered by it; no host reads their results through these
// events.
constexpr unsigned PROF_EVENT_FLAGS = hipEventDisableSystemFence;
std::vector<ProfRec>* g_prof = nullptr;
std::vector<hipEvent_t> g_prof_pool;   // events created before the profiled run (no host-side
size_t g_prof_next = 0;                // event creation between the timed launches)

hipEvent_t prof_event() {
    if (g_prof_next < g_prof_pool.size()) return g_prof_pool[g_prof_next++];
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, PROF_EVENT_FLAGS);
    g_prof_pool.push_back(e);
    g_prof_next = g_prof_pool.size();
    return e;
}

template <class K, class... A>
void launch(int kind, K kernel, dim3 grid, dim3 block, uint32_t lds, A... args) {
    if (g_prof) {
        ProfRec r{kind, prof_event(), prof_event()};
        hipExtLaunchKernelGGL(kernel, grid, block, lds, gp->stream, r.start, r.stop, 0, args...);
        g_prof->push_back(r);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, gp->stream, args...);
    }
}
int nblocks(int n) { return (n + BLOCK - 1) / BLOCK; }

