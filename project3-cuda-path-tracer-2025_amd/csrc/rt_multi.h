// rt_multi.h — several devices behind one context: the shards, their combine, their host copies.
//
// Owns: the RCCL loader, Multi (M) with nshards / shard_ctx / ShardScope, multi_setup /
// multi_combine / multi_release, the band copies (BandCopy, their helper threads: instances of
// host/worker.h, band_prepare over host/band_layout.h) and frame_depth_*.
// Calls: rt_core.h and the combine kernels.  Nothing of rt_pass.h, rt_spec.h or rt_buffers.h.

// ---------------------------------------------------------------------------------------------
// Several GPUs behind one pathtrace() (pt_options.num_devices > 1; SURVEY §8b: the split is
// internal to the boundary).  Shard k is a whole context of its own (State: device, stream,
// scene copy, pass buffers, full-size image of which it writes only its pixels) tracing the
// interleaved row bands (y / rows) % N == k; pixels are independent (the RNG is keyed by pixel,
// iteration and depth), so the shards need no exchange while tracing.  After every call the
// first device's image receives every shard's pixels: a pull kernel over xGMI peer access (or a
// packed tile + hipMemcpyPeerAsync without it), or one RCCL group of send / recv.
// ---------------------------------------------------------------------------------------------
struct Rccl {   // librccl.so, opened at the first pt_init that asks for it (the library is ~570 MB)
    void* h = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;

int rccl_open() {
    if (g_rccl.h) return PT_OK;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(PT_E_UNSUPPORTED, "PT_COMBINE_RCCL: cannot load librccl.so: %s", dlerror());
    Rccl r;
    r.h = h;
#define PT_RCCL_SYM(f)                                                             \
    r.f = reinterpret_cast<decltype(r.f)>(dlsym(h, "nccl" #f));                    \
    if (!r.f) {                                                                    \
        dlclose(h);                                                                \
        return fail(PT_E_UNSUPPORTED, "PT_COMBINE_RCCL: librccl.so lacks nccl" #f); \
    }
    PT_RCCL_SYM(CommInitAll)
    PT_RCCL_SYM(CommDestroy)
    PT_RCCL_SYM(GroupStart)
    PT_RCCL_SYM(GroupEnd)
    PT_RCCL_SYM(Send)
    PT_RCCL_SYM(Recv)
    PT_RCCL_SYM(GetErrorString)
#undef PT_RCCL_SYM
    g_rccl = r;
    return PT_OK;
}
#define NCCLCHK(expr)                                                                                   \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess)                                                                          \
            return fail(PT_E_HIP, "%s:%d: %s: %s", __FILE__, __LINE__, #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

struct Multi {
    int n = 0;                                     // shard contexts (0: single-context mode)
    State* shard[PT_MAX_DEVICES] = {};             // shard[0] == &g_primary
    int combine = PT_COMBINE_PEER;
    hipEvent_t done[PT_MAX_DEVICES] = {};          // shard k's queued work (its stream, its device)
    hipEvent_t pulled = nullptr;                   // the first device finished reading the shards
    bool direct[PT_MAX_DEVICES] = {};              // PEER: the first device reads shard k's image itself
    float* tile[PT_MAX_DEVICES] = {};              // shard k's packed pixels on its device (RCCL, staged peer)
    float* recv[PT_MAX_DEVICES] = {};              // the same on the first device
    // RCCL: one communicator rank per distinct device, each with its own stream
    int ndist = 0;
    int dist_dev[PT_MAX_DEVICES] = {};
    int dist_of[PT_MAX_DEVICES] = {};              // shard k -> index of its device in dist_dev
    ncclComm_t comm[PT_MAX_DEVICES] = {};
    hipStream_t cstream[PT_MAX_DEVICES] = {};
    hipEvent_t cdone[PT_MAX_DEVICES] = {};
    bool band_copy = false;                        // the host copy split over the shards (pt_trace)
};
Multi M;

int nshards() { return M.n > 1 ? M.n : 1; }
State* shard_ctx(int k) { return M.n > 1 ? M.shard[k] : &g_primary; }

// the host runtime works on one shard (its context and its device) until the scope ends
struct ShardScope {
    State* prev;
    int prev_dev = 0;
    explicit ShardScope(State* s) : prev(gp) {
        (void)hipGetDevice(&prev_dev);
        gp = s;
        (void)hipSetDevice(s->device);
    }
    ~ShardScope() {
        gp = prev;
        (void)hipSetDevice(prev_dev);
    }
};

void multi_release() {
    if (M.n <= 1) return;
    int entry_dev = 0;
    (void)hipGetDevice(&entry_dev);
    for (int i = 0; i < M.ndist; ++i) {
        (void)hipSetDevice(M.dist_dev[i]);
        if (M.comm[i] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(M.comm[i]);
        if (M.cdone[i]) (void)hipEventDestroy(M.cdone[i]);
        if (M.cstream[i]) (void)hipStreamDestroy(M.cstream[i]);
    }
    for (int k = 0; k < M.n; ++k) {
        State* s = M.shard[k];
        if (!s) continue;
        (void)hipSetDevice(s->device);
        if (M.done[k]) (void)hipEventDestroy(M.done[k]);
        if (M.tile[k]) (void)hipFree(M.tile[k]);
    }
    (void)hipSetDevice(M.shard[0] ? M.shard[0]->device : 0);
    for (int k = 0; k < M.n; ++k)
        if (M.recv[k]) (void)hipFree(M.recv[k]);
    if (M.pulled) (void)hipEventDestroy(M.pulled);
    (void)hipSetDevice(entry_dev);
}

// events, peer access, tiles and (RCCL) communicators once every shard is initialised
int multi_setup() {
    State* p = M.shard[0];
    ShardScope entry(p);   // restores the caller's device and context last
    for (int k = 0; k < M.n; ++k) {
        ShardScope sc(M.shard[k]);
        HIPCHK(hipEventCreateWithFlags(&M.done[k], hipEventDisableTiming));
    }
    {
        ShardScope sc(p);
        HIPCHK(hipEventCreateWithFlags(&M.pulled, hipEventDisableTiming));
    }
    // tools / tests: PT_COMBINE_FORCE_STAGED=1 sends every PEER shard through its packed tile and a
    // hipMemcpyPeerAsync (the branch taken without peer access), also when the shards share a device
    const bool force_staged = p->tune.combine_force_staged;
    for (int k = 1; k < M.n; ++k) {
        State* s = M.shard[k];
        const size_t bytes = 3 * sizeof(float) * (size_t)std::max(1, s->local_pixels);
        bool direct = M.combine == PT_COMBINE_PEER && s->device == p->device && !force_staged;
        if (M.combine == PT_COMBINE_PEER && !direct && !force_staged) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, p->device, s->device) == hipSuccess && can) {
                ShardScope sc(p);
                const hipError_t e = hipDeviceEnablePeerAccess(s->device, 0);
                if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) direct = true;
                (void)hipGetLastError();
            }
        }
        M.direct[k] = direct;
        if (!direct) {   // packed tiles: RCCL, or peer copies without peer access
            {
                ShardScope sc(s);
                RC(dalloc(&M.tile[k], bytes / sizeof(float)));
            }
            ShardScope sc(p);
            RC(dalloc(&M.recv[k], bytes / sizeof(float)));
        }
    }
    // the host copy of single-frame calls split over the shards' own links: by default only when
    // every shard has a device of its own (shards sharing a device share its link, and the split
    // then only adds the helper hand-offs: tools/multi_probe.py on one GPU)
    {
        bool distinct = true;
        for (int a = 0; a < M.n; ++a)
            for (int b = a + 1; b < M.n; ++b) distinct = distinct && M.shard[a]->device != M.shard[b]->device;
        M.band_copy = p->tune.band_copy > 0 || (p->tune.band_copy < 0 && distinct);
    }
    if (M.combine != PT_COMBINE_RCCL) return PT_OK;
    RC(rccl_open());
    for (int k = 0; k < M.n; ++k) {
        int i = 0;
        while (i < M.ndist && M.dist_dev[i] != M.shard[k]->device) ++i;
        if (i == M.ndist) M.dist_dev[M.ndist++] = M.shard[k]->device;
        M.dist_of[k] = i;
    }
    NCCLCHK(g_rccl.CommInitAll(M.comm, M.ndist, M.dist_dev));
    for (int i = 0; i < M.ndist; ++i) {
        HIPCHK(hipSetDevice(M.dist_dev[i]));
        HIPCHK(hipStreamCreateWithFlags(&M.cstream[i], hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&M.cdone[i], hipEventDisableTiming));
    }
    HIPCHK(hipSetDevice(p->device));
    return PT_OK;
}

// k_gather_shards' shard layout (sources filled in by the caller)
GatherSrc gather_src(int W, int H) {
    GatherSrc g{};
    g.n = M.n;
    g.rows = std::max(1, M.shard[0]->sc.shard.rows);
    g.W = W;
    g.H = H;
    return g;
}

// every shard's pixels into the first device's image, ordered after the work queued so far on
// every shard's stream; the shards' next work waits until the first device has read them
int multi_combine() {
    if (M.n <= 1) return PT_OK;
    State* p = M.shard[0];
    ShardScope entry(p);   // restores the caller's device and context last
    const int W = p->width;
    for (int k = 1; k < M.n; ++k) {
        State* s = M.shard[k];
        ShardScope sc(s);
        if (!M.direct[k]) {
            hipLaunchKernelGGL(k_pack_tile, dim3(nblocks(s->local_pixels)), dim3(BLOCK), 0, s->stream, s->d_image,
                               s->sc.shard, W, M.tile[k]);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(M.done[k], s->stream));
    }
    if (M.combine == PT_COMBINE_RCCL) {
        const int d0 = M.dist_of[0];
        {   // the first device's receive buffers are free once its earlier unpacks ran
            ShardScope sc(p);
            HIPCHK(hipEventRecord(M.done[0], p->stream));
        }
        for (int k = 0; k < M.n; ++k) {
            HIPCHK(hipSetDevice(M.dist_dev[M.dist_of[k]]));
            HIPCHK(hipStreamWaitEvent(M.cstream[M.dist_of[k]], M.done[k], 0));
        }
        NCCLCHK(g_rccl.GroupStart());
        for (int k = 1; k < M.n; ++k) {
            const size_t cnt = 3 * (size_t)M.shard[k]->local_pixels;
            const int dk = M.dist_of[k];
            NCCLCHK(g_rccl.Send(M.tile[k], cnt, ncclFloat32, d0, M.comm[dk], M.cstream[dk]));
            NCCLCHK(g_rccl.Recv(M.recv[k], cnt, ncclFloat32, dk, M.comm[d0], M.cstream[d0]));
        }
        NCCLCHK(g_rccl.GroupEnd());
        for (int i = 0; i < M.ndist; ++i) {
            HIPCHK(hipSetDevice(M.dist_dev[i]));
            HIPCHK(hipEventRecord(M.cdone[i], M.cstream[i]));
        }
        for (int k = 1; k < M.n; ++k) {   // a tile is rewritten only after its send completed
            ShardScope sc(M.shard[k]);
            HIPCHK(hipStreamWaitEvent(M.shard[k]->stream, M.cdone[M.dist_of[k]], 0));
        }
        ShardScope sc(p);
        HIPCHK(hipStreamWaitEvent(p->stream, M.cdone[d0], 0));
        // every shard's own work too (its TracedDepth counter copy is queued before done[k]):
        // once the first device's stream has drained, so has every shard's frame
        for (int k = 1; k < M.n; ++k) HIPCHK(hipStreamWaitEvent(p->stream, M.done[k], 0));
        GatherSrc g = gather_src(W, p->height);
        for (int k = 1; k < M.n; ++k) {
            g.src[k] = M.recv[k];
            g.local[k] = 1;
        }
        hipLaunchKernelGGL(k_gather_shards, dim3(nblocks(p->pixels_total)), dim3(BLOCK), 0, p->stream, p->d_image, g);
        HIPCHK(hipGetLastError());
        return PT_OK;
    }
    ShardScope sc(p);
    GatherSrc g = gather_src(W, p->height);
    for (int k = 1; k < M.n; ++k) {
        State* s = M.shard[k];
        HIPCHK(hipStreamWaitEvent(p->stream, M.done[k], 0));
        if (M.direct[k]) {   // read in place over peer access
            g.src[k] = s->d_image;
            g.local[k] = 0;
        } else {             // packed tile, copied to the first device
            HIPCHK(hipMemcpyPeerAsync(M.recv[k], p->device, M.tile[k], s->device,
                                      3 * sizeof(float) * (size_t)s->local_pixels, p->stream));
            g.src[k] = M.recv[k];
            g.local[k] = 1;
        }
    }
    hipLaunchKernelGGL(k_gather_shards, dim3(nblocks(p->pixels_total)), dim3(BLOCK), 0, p->stream, p->d_image, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(M.pulled, p->stream));
    for (int k = 1; k < M.n; ++k) {   // a shard's image changes again only after it was read
        ShardScope s2(M.shard[k]);
        HIPCHK(hipStreamWaitEvent(M.shard[k]->stream, M.pulled, 0));
    }
    return PT_OK;
}

// ---- several devices: the host copy split over the shards' own links --------------------------
// main.cpp's pathtrace() copies the whole image to pageable host memory every call
// (pathtrace.cu:783).  From one device that copy crosses one PCIe link (~0.14 ms at 800^2, longer
// than the frame).  With several devices each shard copies its own row bands from its own device,
// so the devices' links run side by side.  A copy into pageable memory holds the thread that
// issues it until it is done, so shard k's copy is issued by helper thread k (shard 0's by the
// caller).  The helpers keep INTEGRATION.md's threading rules: a helper gets copied values only
// (its shard's device and band stream, the event the caller recorded after the shard's frame, the
// two image bases and the band geometry), calls nothing but those HIP copies, and the call waits
// for every helper before it returns.
struct BandCopy {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr;
    const char* src = nullptr;     // a full-size image on the shard's device (same layout as dst)
    char* dst = nullptr;           // the caller's host image
    pth::BandGeom g;               // the shard's bytes of the image (host/band_layout.h)
    hipError_t run() const {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, ready, 0);
        if (e == hipSuccess && g.height > 0)
            e = hipMemcpy2DAsync(dst + g.first, g.pitch, src + g.first, g.pitch, g.width, g.height, hipMemcpyDeviceToHost,
                                 stream);
        if (e == hipSuccess && g.tail_bytes > 0)
            e = hipMemcpyAsync(dst + g.tail_off, src + g.tail_off, g.tail_bytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        return e;
    }
};
// helper k copies shard k's bands; every job's result replaces the last one (pth::Worker, not sticky)
pth::Worker<BandCopy, hipError_t> g_copy_helpers[PT_MAX_DEVICES];

// the current shard's row bands of `src` (a full-size image on its device: its own pixels are
// final) into the host image, after the work queued so far on `after`
int band_prepare(BandCopy& b, float* host, const float* src, hipStream_t after) {
    if (!gp->band_stream) {
        HIPCHK(hipStreamCreateWithFlags(&gp->band_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&gp->band_ready, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(gp->band_ready, after));
    const ShardDev& sd = gp->sc.shard;
    b = BandCopy();
    b.device = gp->device;
    b.stream = gp->band_stream;
    b.ready = gp->band_ready;
    b.src = reinterpret_cast<const char*>(src);
    b.dst = reinterpret_cast<char*>(host);
    b.g = pth::band_geometry(gp->width, gp->height, sd.rows, sd.count, sd.rank);
    return PT_OK;
}

// GuiDataContainer::TracedDepth of the last single-frame pass of the current context: the loop
// stops after bounce k when no path is left alive, or at traceDepth (pathtrace.cu:759-770).
// Two halves so that no call waits twice: frame_depth_enqueue queues the copy of the frame's live
// counters into page-locked host memory on the context's stream (behind the frame, before the
// caller's one synchronisation), frame_depth_read reads them after it.
int frame_depth_enqueue() {
    if (!gp->opts.stream_compaction) return PT_OK;
    const size_t n = (size_t)std::max(1, gp->sc.trace_depth) * NSEG * CNT_PAD;
    if (!gp->h_cnt) HIPCHK(hipHostMalloc((void**)&gp->h_cnt, sizeof(int) * (size_t)(MAXB + 1) * NSEG * CNT_PAD));
    HIPCHK(hipMemcpyAsync(gp->h_cnt, &gp->d_ctl->cnt[0][0][0], n * sizeof(int), hipMemcpyDeviceToHost, gp->stream));
    return PT_OK;
}
int frame_depth_read() {
    int depth = std::max(1, gp->sc.trace_depth);
    if (!gp->opts.stream_compaction || !gp->h_cnt) return depth;
    for (int k = 1; k < depth; ++k) {
        int64_t live = 0;
        for (int q = 0; q < NSEG; ++q) live += gp->h_cnt[((size_t)k * NSEG + q) * CNT_PAD];
        if (live == 0) return k;
    }
    return depth;
}
