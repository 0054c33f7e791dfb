// rt_buffers.h — the per-pass device buffers: how large, when (re)allocated, how released.
//
// Owns: free_* / free_all, the *_stride_for / capacity_for / pass_bytes arithmetic, ensure_frames /
// ensure_staged / ensure_test_paths, upload and the path AoS <-> SoA helpers.
// Calls: rt_core.h, release_graph and spec_release of rt_spec.h (captured graphs hold the old
// pointers, so they go before the buffers do).

// staged-pipeline buffers (hits, alive flags, permutation, tile counts): the staged pipeline and
// the pt_test_* entry points use them; the fused pipeline never does
void free_staged_buffers() {
    dfree(gp->d_hit_nt);
    dfree(gp->d_hit_mat);
    dfree(gp->d_hit_uvd0);
    dfree(gp->d_hit_uvd1);
    dfree(gp->d_alive);
    dfree(gp->d_perm);
    dfree(gp->d_tile_hist);
    dfree(gp->d_tile_cnt);
    dfree(gp->d_tile_off);
    gp->staged_alloc = false;
}
void free_pass_buffers() {
    free_staged_buffers();
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) dfree(gp->d_path[i][k]);
    dfree(gp->queue.A);
    dfree(gp->queue.B);
    dfree(gp->queue.C);
    dfree(gp->queue.D);
    dfree(gp->tail.node);
    dfree(gp->tail.hit);
    dfree(gp->tail.stack);
    gp->tail.stride = gp->tail.cap = 0;
    dfree(gp->sc.spill);
    dfree(gp->d_contrib);
    gp->sc.contrib = nullptr;
    gp->alloc_frames = 0;
    gp->seg_stride = 0;
    gp->capacity = 0;
}

// output segment s receives the survivors of the chunks c = s (mod NSEG): of k_bounce's, and in
// split mode also of k_bvh_bounce's (its chunks of the queue) -- twice the room then
int seg_stride_for(int frames) {
    const int nb = nblocks(std::max(1, gp->local_pixels * frames));
    return ((nb + NSEG - 1) / NSEG) * BLOCK * (gp->split ? 2 : 1);
}
// entries per traversal-queue segment: the rays of its k_bounce blocks (blockIdx % NSEG)
int q_stride_for(int frames) {
    const int nb = nblocks(std::max(1, gp->local_pixels * frames));
    return ((nb + NSEG - 1) / NSEG) * BLOCK;
}
// k_bvh_bounce hands a wave's traversals to k_bvh_tail_trav once no more than this many of its lanes
// are still traversing (PT_BVH_TAIL_LANES, 0: never; at most 56).  By default 32, and 48 for trees
// of 65,536 refs or more (stack entries with refs wider than 16 bits): deeper traversals diverge
// more, so handing over earlier pays (A/B on the 4-wide records, profiles/r06_ab_tail_lanes_four_wide.json:
// bunny / khaslana best at 32, the 262k stand-in at 48, 3.5 % below 32)
int bvh_tail_lanes() {
    if (gp->tune.bvh_tail_lanes >= 0) return gp->tune.bvh_tail_lanes;
    return 32 - gp->sc.ref_shift > 16 ? 48 : 32;
}
// entries per tail segment: what k_bvh_bounce can hand over, `lanes` per wave of its blocks of one
// segment.  Tools: PT_BVH_TAIL_CHUNKS=c caps it at c blocks' worth; a lane that finds its segment
// full then finishes its ray itself (tail_put).  A cap measured slower at every size tried:
// bunny's passes hand over ~20 % of 128 frames' queued rays (DESIGN Appendix A).
int tail_stride(int frames, int lanes) {
    const int chunks = gp->tune.bvh_tail_chunks;
    const int nb = nblocks(std::max(1, gp->local_pixels * frames));
    const int s = ((nb + NSEG - 1) / NSEG) * (BLOCK / 64) * lanes;
    return chunks > 0 ? std::min(s, chunks * BLOCK) : s;
}
// paths a pass of `frames` frames needs room for, tile-padded (kernels may read a whole tile)
int capacity_for(int frames) {
    const int c = std::max(seg_stride_for(frames) * NSEG, gp->local_pixels * frames);
    return ((c + STILE - 1) / STILE) * STILE;
}
// device bytes of the per-pass buffers for `frames` frames (auto F is capped by free memory)
size_t pass_bytes(int frames, bool staged) {
    const size_t cap = (size_t)capacity_for(frames);
    size_t b = 2 * 3 * sizeof(float4) * cap;                                     // path ping-pong
    if (gp->split) b += (4 * sizeof(float4) + sizeof(int) * gp->sc.spill_stride) * (size_t)q_stride_for(frames) * NSEG;   // traversal queue (+ stack spill rows)
    if (gp->split && bvh_tail_lanes() > 0)   // handed-over traversals
        b += (sizeof(int2) + sizeof(float4) + sizeof(int) * std::max(1, gp->sc.stack_lds)) * NSEG *
             (size_t)tail_stride(frames, bvh_tail_lanes());
    if (frames > 1) b += 3 * sizeof(float) * (size_t)gp->pixels_total * frames;      // contribution planes
    if (staged) b += cap * (sizeof(float4) + 3 * sizeof(int) + (gp->num_tex ? 2 * sizeof(float4) : 0));
    return b;
}

// Path buffers, traversal queue and contribution planes for passes of up to `frames` frames.
// Grows only; captured pass graphs hold the old pointers, so they are released on growth.
int ensure_frames(int frames) {
    frames = std::max(1, frames);
    if (frames <= gp->alloc_frames) return PT_OK;
    const bool staged = gp->staged_alloc || gp->opts.pipeline == PT_PIPELINE_STAGED;
    // a captured pass may still be running (pt_trace_frames does not wait): drain the stream
    // before its graph and the buffers it reads go away
    HIPCHK(hipStreamSynchronize(gp->stream));
    release_graph();
    free_pass_buffers();
    gp->seg_stride = seg_stride_for(frames);
    gp->capacity = capacity_for(frames);
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) RC(dalloc(&gp->d_path[i][k], (size_t)gp->capacity));
    if (gp->split) {   // NSEG queue segments, each room for the queued rays of its k_bounce blocks
        gp->queue.stride = q_stride_for(frames);
        const size_t qn = (size_t)gp->queue.stride * NSEG;
        RC(dalloc(&gp->queue.A, qn));
        RC(dalloc(&gp->queue.B, qn));
        RC(dalloc(&gp->queue.C, qn));
        RC(dalloc(&gp->queue.D, qn));
        gp->tail_lanes = bvh_tail_lanes();
        gp->tail_refill = gp->tune.tail_refill;
        gp->tail_trav_blocks = gp->tune.tail_trav_blocks;
        gp->tail_shade_blocks = gp->tune.tail_shade_blocks;
        // stack entries past the LDS part: one row per queue slot (rare: deep stacks only)
        if (gp->sc.spill_stride > 0) RC(dalloc(&gp->sc.spill, qn * (size_t)gp->sc.spill_stride));
        if (gp->tail_lanes > 0) {   // a wave hands over at most tail_lanes rays
            gp->tail_depth = std::max(1, gp->sc.stack_lds);
            TailBuf& t = gp->tail;
            t.stride = tail_stride(frames, gp->tail_lanes);
            t.cap = t.stride * NSEG;
            t.depth = gp->tail_depth;
            RC(dalloc(&t.node, (size_t)t.cap));
            RC(dalloc(&t.hit, (size_t)t.cap));
            RC(dalloc(&t.stack, (size_t)t.cap * gp->tail_depth));
        }
    }
    if (frames > 1) RC(dalloc(&gp->d_contrib, (size_t)gp->pixels_total * 3 * frames));
    gp->sc.contrib = gp->d_contrib;
    gp->alloc_frames = frames;
    if (staged) {
        RC(dalloc(&gp->d_hit_nt, (size_t)gp->capacity));
        RC(dalloc(&gp->d_hit_mat, (size_t)gp->capacity));
        if (gp->num_tex) {
            RC(dalloc(&gp->d_hit_uvd0, (size_t)gp->capacity));
            RC(dalloc(&gp->d_hit_uvd1, (size_t)gp->capacity));
        }
        RC(dalloc(&gp->d_alive, (size_t)gp->capacity));
        RC(dalloc(&gp->d_perm, (size_t)gp->capacity));
        const int ntiles = (gp->capacity + CTILE_MIN - 1) / CTILE_MIN + 1;
        RC(dalloc(&gp->d_tile_hist, (size_t)ntiles * std::max(1, gp->sc.num_mats)));
        RC(dalloc(&gp->d_tile_cnt, (size_t)ntiles));
        RC(dalloc(&gp->d_tile_off, (size_t)ntiles));
        gp->staged_alloc = true;
    }
    return PT_OK;
}
// the staged buffers at the current capacity (the pt_test_* entry points under the fused pipeline)
int ensure_staged() {
    if (gp->staged_alloc) return PT_OK;
    const int f = std::max(1, gp->alloc_frames);
    gp->alloc_frames = 0;              // re-size everything with the staged buffers included
    gp->staged_alloc = true;
    return ensure_frames(f);
}
// a pt_test_* call on n paths: room for n (up to what a pass of gp->batch frames holds) + staged buffers
int ensure_test_paths(int64_t n) {
    const int64_t most = capacity_for(gp->batch);
    if (n < 0 || n > most) return fail(PT_E_INVALID, "n out of range (capacity %lld)", (long long)most);
    RC(ensure_staged());
    const int frames = (int)std::min<int64_t>(gp->batch, std::max<int64_t>(1, (n + gp->local_pixels - 1) / gp->local_pixels));
    RC(ensure_frames(frames));
    if (n > gp->capacity) return fail(PT_E_INVALID, "n out of range (capacity %d)", gp->capacity);
    return PT_OK;
}

void free_all() {
    spec_release();
    if (gp->band_stream) (void)hipStreamSynchronize(gp->band_stream), (void)hipStreamDestroy(gp->band_stream);
    if (gp->band_ready) (void)hipEventDestroy(gp->band_ready);
    gp->band_stream = nullptr;
    gp->band_ready = nullptr;
    release_graph();
    free_pass_buffers();
    for (float4*& p : gp->d_gbuf) dfree(p);
    for (float4*& p : gp->d_dn_color) dfree(p);
    for (hipEvent_t& e : gp->dn_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    void* ptrs[] = {gp->d_geoms, gp->d_cull, gp->d_mats, gp->d_nodes, gp->d_node_aux, gp->d_hot, gp->d_pairs, gp->d_quads, gp->d_hot4,
                    gp->d_leaf9, gp->d_cold, gp->d_naive_hot, gp->d_texels, gp->d_texinfo, gp->d_image, gp->d_ctl, gp->d_grid};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (gp->stream) (void)hipStreamDestroy(gp->stream);
    if (gp->h_cnt) (void)hipHostFree(gp->h_cnt);
    int32_t* td = gp->traced_depth;
    *gp = State();
    gp->traced_depth = td;
}

template <class T>
int upload(T* d, const T* h, size_t n) {
    if (n) HIPCHK(smemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}

// AoS (reference layout) <-> SoA wavefront
void paths_to_soa(const pt_path_segment* p, int64_t n, std::vector<float4>& A, std::vector<float4>& B,
                  std::vector<float4>& C) {
    A.resize(n);
    B.resize(n);
    C.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        int32_t pix = p[i].pixelIndex, rb = p[i].remainingBounces;
        float fp, fr;
        memcpy(&fp, &pix, 4);
        memcpy(&fr, &rb, 4);
        A[i] = make_float4(p[i].ray.origin.x, p[i].ray.origin.y, p[i].ray.origin.z, fp);
        B[i] = make_float4(p[i].ray.direction.x, p[i].ray.direction.y, p[i].ray.direction.z, fr);
        C[i] = make_float4(p[i].color.x, p[i].color.y, p[i].color.z, 0.f);
    }
}
void soa_to_paths(const std::vector<float4>& A, const std::vector<float4>& B, const std::vector<float4>& C,
                  int64_t n, pt_path_segment* p) {
    for (int64_t i = 0; i < n; ++i) {
        p[i].ray.origin = pt_vec3{A[i].x, A[i].y, A[i].z};
        p[i].ray.direction = pt_vec3{B[i].x, B[i].y, B[i].z};
        p[i].color = pt_vec3{C[i].x, C[i].y, C[i].z};
        memcpy(&p[i].pixelIndex, &A[i].w, 4);
        memcpy(&p[i].remainingBounces, &B[i].w, 4);
    }
}

// n paths to / from slots at .. at + n - 1 of path buffer `buf`
int upload_paths(int buf, const pt_path_segment* paths, int64_t n, int64_t at = 0) {
    if (n <= 0) return PT_OK;
    std::vector<float4> A, B, C;
    paths_to_soa(paths, n, A, B, C);
    HIPCHK(smemcpy(gp->d_path[buf][0] + at, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(smemcpy(gp->d_path[buf][1] + at, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(smemcpy(gp->d_path[buf][2] + at, C.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    return PT_OK;
}
int download_paths(int buf, int64_t n, pt_path_segment* out, int64_t at = 0) {
    if (n <= 0) return PT_OK;
    std::vector<float4> A(n), B(n), C(n);
    HIPCHK(smemcpy(A.data(), gp->d_path[buf][0] + at, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(smemcpy(B.data(), gp->d_path[buf][1] + at, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(smemcpy(C.data(), gp->d_path[buf][2] + at, n * sizeof(float4), hipMemcpyDeviceToHost));
    soa_to_paths(A, B, C, n, out);
    return PT_OK;
}
int set_count(int slot, int value) {
    HIPCHK(smemcpy(&gp->d_ctl->cnt[slot][0][0], &value, sizeof(int), hipMemcpyHostToDevice));
    return PT_OK;
}

