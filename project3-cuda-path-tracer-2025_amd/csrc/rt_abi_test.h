// rt_abi_test.h — the test, debug and profiling entry points (inside pt_runtime.hip's extern "C"
// block).  Owns: pt_test_*, pt_debug_section_counters, pt_profile_frames.  Calls: every rt_*.h.
// The entry points that use the path buffers (camera, intersect, shade, compact, bounce, sort,
// pt_profile_frames) first drop a speculated frame (need_single); the pt_test_* among them leave
// FrameCtl reset.  The others only read the context or run a kernel on buffers of their own.

// ---------------------------------------------------------------------------------------------
// test entry points
// ---------------------------------------------------------------------------------------------
int32_t pt_test_camera(int32_t iteration, pt_path_segment* out, int64_t n) {
    RC(need_init());
    RC(need_single("pt_test_camera"));
    if (!out || n < gp->local_pixels) return fail(PT_E_INVALID, "output too small");
    RC(ensure_frames(1));
    RC(ctl_reset());
    hipLaunchKernelGGL(k_frame_begin, dim3(1), dim3(256), 0, gp->stream, gp->d_ctl, iteration, gp->local_pixels, 1,
                       gp->ctl_rows, 0);
    hipLaunchKernelGGL(k_camera, dim3(nblocks(gp->local_pixels)), dim3(BLOCK), 0, gp->stream, gp->sc, pathbuf(0), gp->d_ctl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(gp->stream));
    release_graph();
    RC(download_paths(0, gp->local_pixels, out));
    RC(ctl_reset());
    return PT_OK;
}

int32_t pt_test_intersect(const pt_path_segment* paths, int64_t n, pt_shadeable_isect* isects) {
    RC(need_init());
    RC(need_single("pt_test_intersect"));
    RC(ensure_test_paths(n));
    if (n == 0) return PT_OK;
    RC(upload_paths(0, paths, n));
    RC(set_count(0, (int)n));
    // uv / dpdu / dpdv are kept by the production pipelines only for textured scenes (nothing else
    // reads them); this entry point returns the reference's whole record, so mesh scenes without
    // textures get temporary attribute buffers, released on every return path
    struct TmpAttr {
        float4* p[2] = {nullptr, nullptr};
        ~TmpAttr() {
            for (float4* x : p)
                if (x) (void)hipFree(x);
        }
    } tmp;
    float4 *uvd0 = gp->d_hit_uvd0, *uvd1 = gp->d_hit_uvd1;
    const bool naive_tris = gp->naive && gp->sc.num_tris > 0;
    if (!uvd0 && (gp->has_bvh || naive_tris)) {
        RC(dalloc(&tmp.p[0], (size_t)n));
        RC(dalloc(&tmp.p[1], (size_t)n));
        uvd0 = tmp.p[0];
        uvd1 = tmp.p[1];
    }
    HitBuf hits{gp->d_hit_nt, gp->d_hit_mat, uvd0, uvd1};
    if (gp->has_bvh && (gp->opts.variant & VAR_BVH_FAST))
        hipLaunchKernelGGL((k_intersect<true, true>), dim3(nblocks((int)n)), dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc,
                           pathbuf(0), hits, staged_count(0));
    else if (gp->has_bvh)
        hipLaunchKernelGGL((k_intersect<true, false>), dim3(nblocks((int)n)), dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc,
                           pathbuf(0), hits, staged_count(0));
    else
        hipLaunchKernelGGL((k_intersect<false, false>), dim3(nblocks((int)n)), dim3(BLOCK), 0, gp->stream, gp->sc,
                           pathbuf(0), hits, staged_count(0));
    if (naive_tris)   // as the staged pipeline runs it
        hipLaunchKernelGGL(k_naive_mesh, dim3(nblocks((int)n)), dim3(BLOCK), 0, gp->stream, gp->sc,
                           (const DevTriHot*)gp->d_naive_hot, gp->sc.num_tris, pathbuf(0), hits.nt, hits.mat, hits.uvd0,
                           hits.uvd1, staged_count(0));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(gp->stream));
    std::vector<float4> nt(n);
    std::vector<int> mat(n);
    HIPCHK(smemcpy(nt.data(), gp->d_hit_nt, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(smemcpy(mat.data(), gp->d_hit_mat, n * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float4> a0, a1;
    if (uvd0) {
        a0.resize(n);
        a1.resize(n);
        HIPCHK(smemcpy(a0.data(), uvd0, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(smemcpy(a1.data(), uvd1, n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i) {
        memset(&isects[i], 0, sizeof(pt_shadeable_isect));
        isects[i].t = nt[i].w;
        isects[i].surfaceNormal = pt_vec3{nt[i].x, nt[i].y, nt[i].z};
        isects[i].materialId = mat[i];
        if (uvd0 && nt[i].w > 0.0f) {   // uv / dpdu / dpdv as the reference writes them (zero for primitives)
            isects[i].uv = pt_vec2{a0[i].x, a0[i].y};
            isects[i].dpdu = pt_vec3{a0[i].z, a0[i].w, a1[i].x};
            isects[i].dpdv = pt_vec3{a1[i].y, a1[i].z, a1[i].w};
        }
    }
    release_graph();
    RC(ctl_reset());
    return PT_OK;
}

int32_t pt_test_shade(int32_t iteration, const pt_shadeable_isect* isects, pt_path_segment* paths, int64_t n) {
    RC(need_init());
    RC(need_single("pt_test_shade"));
    RC(ensure_test_paths(n));
    if (n == 0) return PT_OK;
    RC(upload_paths(0, paths, n));
    RC(set_count(0, (int)n));
    std::vector<float4> nt(n);
    std::vector<int> mat(n);
    for (int64_t i = 0; i < n; ++i) {
        nt[i] = make_float4(isects[i].surfaceNormal.x, isects[i].surfaceNormal.y, isects[i].surfaceNormal.z,
                            isects[i].t);
        mat[i] = isects[i].materialId;
        if (isects[i].t > 0.0f && (mat[i] < 0 || mat[i] >= std::max(1, gp->sc.num_mats)))
            return fail(PT_E_INVALID, "materialId %d out of range", mat[i]);
    }
    HIPCHK(smemcpy(gp->d_hit_nt, nt.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(smemcpy(gp->d_hit_mat, mat.data(), n * sizeof(int), hipMemcpyHostToDevice));
    if (gp->d_hit_uvd0) {
        std::vector<float4> a0(n), a1(n);
        for (int64_t i = 0; i < n; ++i) {
            const pt_shadeable_isect& x = isects[i];
            a0[i] = make_float4(x.uv.x, x.uv.y, x.dpdu.x, x.dpdu.y);
            a1[i] = make_float4(x.dpdu.z, x.dpdv.x, x.dpdv.y, x.dpdv.z);
        }
        HIPCHK(smemcpy(gp->d_hit_uvd0, a0.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(smemcpy(gp->d_hit_uvd1, a1.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    }
    HitBuf hits{gp->d_hit_nt, gp->d_hit_mat, gp->d_hit_uvd0, gp->d_hit_uvd1};
    hipLaunchKernelGGL(k_shade, dim3(nblocks((int)n)), dim3(BLOCK), 0, gp->stream, gp->sc, pathbuf(0), hits,
                       (const int*)nullptr, staged_count(0), (const FrameCtl*)gp->d_ctl, iteration, (float*)nullptr,
                       (int*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(gp->stream));
    release_graph();
    RC(download_paths(0, n, paths));
    RC(ctl_reset());
    return PT_OK;
}

int32_t pt_test_compact(const pt_path_segment* paths, int64_t n, pt_path_segment* out, int64_t* alive_out) {
    RC(need_init());
    RC(need_single("pt_test_compact"));
    RC(ensure_test_paths(n));
    RC(upload_paths(0, paths, n));
    std::vector<int> al(std::max<int64_t>(1, n));
    for (int64_t i = 0; i < n; ++i) al[i] = paths[i].remainingBounces > 0;   // PathAlive
    if (n) HIPCHK(smemcpy(gp->d_alive, al.data(), n * sizeof(int), hipMemcpyHostToDevice));
    RC(ctl_reset());
    RC(set_count(0, (int)n));
    if (n > 0) {   // the pipeline's launch sequence
        launch_compact<CITEMS>(pathbuf(0), pathbuf(1), staged_count(0), &gp->d_ctl->cnt[1][0][0], (int)n);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(gp->stream));
    int na = 0;
    HIPCHK(smemcpy(&na, &gp->d_ctl->cnt[1][0][0], sizeof(int), hipMemcpyDeviceToHost));
    if (alive_out) *alive_out = na;
    release_graph();
    RC(download_paths(1, na, out));
    RC(ctl_reset());
    return PT_OK;
}

// One production bounce of the fused pipeline on caller-supplied paths: the n paths laid into the
// input buffer of `bounce` as the previous bounce's kernels would have left them (seg_counts[s] of
// them in segment s, in order; NULL: all in segment 0), a single-frame pass of `iteration` in
// frame slot 0, then launch_bounce exactly as enqueue_pass_body calls it.  Terminated paths are
// gathered into the accumulated image; the survivors of every output segment come back segment
// after segment (their order inside a segment is the kernels' business), seg_out[s] of them from
// segment s.  The path buffers are sized for min(frames per pass, NSEG) frames first: with NSEG
// frames a segment holds a whole frame's paths, so any split of n over the segments fits.
int32_t pt_test_bounce(int32_t iteration, int32_t bounce, const pt_path_segment* paths, int64_t n,
                       const int32_t* seg_counts, pt_path_segment* out_paths, int64_t out_capacity, int64_t* n_out,
                       int32_t* seg_out) {
    RC(need_init());
    RC(need_single("pt_test_bounce"));
    if (gp->opts.pipeline != PT_PIPELINE_FUSED || gp->naive)
        return fail(PT_E_INVALID, "pt_test_bounce: the fused pipeline only (this context runs the staged one)");
    if (iteration <= 0) return fail(PT_E_INVALID, "iteration is 1-based, got %d", iteration);
    if (bounce < 1 || bounce >= MAXB)
        return fail(PT_E_INVALID, "pt_test_bounce: bounce must be 1 .. %d, got %d", MAXB - 1, bounce);
    if (n < 0 || n > gp->local_pixels)
        return fail(PT_E_INVALID, "pt_test_bounce: n = %lld, one frame's wavefront holds %d paths", (long long)n,
                    gp->local_pixels);
    if ((n > 0 && !paths) || !n_out || (out_capacity > 0 && !out_paths) || out_capacity < 0)
        return fail(PT_E_INVALID, "pt_test_bounce: null argument");
    RC(ensure_test_paths(n));
    RC(ensure_frames(std::min(gp->batch, NSEG)));
    const int stride = gp->seg_stride;
    int cnt[NSEG] = {};
    int64_t total = 0;
    for (int s = 0; s < NSEG; ++s) {
        cnt[s] = seg_counts ? seg_counts[s] : (s == 0 ? (int)n : 0);
        if (cnt[s] < 0 || cnt[s] > stride)
            return fail(PT_E_INVALID, "pt_test_bounce: %d paths in segment %d, a segment holds %d", cnt[s], s, stride);
        total += cnt[s];
    }
    if (total != n) return fail(PT_E_INVALID, "pt_test_bounce: the segment counts add up to %lld, n = %lld",
                                (long long)total, (long long)n);
    HIPCHK(hipStreamSynchronize(gp->stream));
    RC(ctl_reset());   // every counter zero: this bounce's queue, the next bounce's segments
    const int ib = bounce & 1, ob = (bounce + 1) & 1;
    int64_t at = 0;
    for (int s = 0; s < NSEG; ++s) {
        RC(upload_paths(ib, paths + at, cnt[s], (int64_t)s * stride));
        HIPCHK(smemcpy(&gp->d_ctl->cnt[bounce][s][0], &cnt[s], sizeof(int), hipMemcpyHostToDevice));
        at += cnt[s];
    }
    const int head[3] = {iteration, 1, 0};   // FrameCtl::iter, batch, plane
    HIPCHK(smemcpy(&gp->d_ctl->iter, head, sizeof head, hipMemcpyHostToDevice));
    if (n > 0) {
        launch_bounce(false, gp->has_bvh, gp->opts.variant & ~VAR_BVH_NODES, dim3(nblocks((int)n)), pathbuf(ib),
                      pathbuf(ob), bounce);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(gp->stream));
    int got[NSEG] = {};
    total = 0;
    for (int s = 0; s < NSEG; ++s) {
        HIPCHK(smemcpy(&got[s], &gp->d_ctl->cnt[bounce + 1][s][0], sizeof(int), hipMemcpyDeviceToHost));
        total += got[s];
    }
    release_graph();
    for (int s = 0; s < NSEG; ++s)
        if (got[s] < 0 || got[s] > stride) {
            RC(ctl_reset());
            return fail(PT_E_HIP, "pt_test_bounce: output segment %d counts %d paths, it holds %d", s, got[s], stride);
        }
    *n_out = total;
    if (total > out_capacity) {
        RC(ctl_reset());
        return fail(PT_E_INVALID, "pt_test_bounce: %lld survivors, room for %lld", (long long)total,
                    (long long)out_capacity);
    }
    at = 0;
    for (int s = 0; s < NSEG; ++s) {
        RC(download_paths(ob, got[s], out_paths + at, (int64_t)s * stride));
        if (seg_out) seg_out[s] = got[s];
        at += got[s];
    }
    RC(ctl_reset());
    return PT_OK;
}

// the kernel variant pt_test_bounce (and every later bounce of a frame) launches: launch_bounce's own
// effective_variant of the context's options; *split: k_bvh_bounce runs behind the traversal queue
int32_t pt_test_bounce_variant(int32_t* variant, int32_t* split) {
    RC(need_init());
    if (!variant || !split) return fail(PT_E_INVALID, "pt_test_bounce_variant: null argument");
    if (gp->opts.pipeline != PT_PIPELINE_FUSED || gp->naive)
        return fail(PT_E_INVALID, "pt_test_bounce_variant: the fused pipeline only (this context runs the staged one)");
    *variant = effective_variant(false, gp->opts.variant & ~VAR_BVH_NODES);
    *split = (gp->has_bvh && (*variant & VAR_BVH_SPLIT)) ? 1 : 0;
    return PT_OK;
}

// the candidate table's geometry (grid_superset): cell = (o - lo) * inv per axis, `cells` cells per
// axis and `bins` direction bins per ratio; cells = 0: this context's scene has no table
int32_t pt_test_grid_info(float lo[3], float inv[3], int32_t* cells, int32_t* bins) {
    RC(need_init());
    if (!lo || !inv || !cells || !bins) return fail(PT_E_INVALID, "pt_test_grid_info: null argument");
    for (int a = 0; a < 3; ++a) {
        lo[a] = gp->sc.grid_lo[a];
        inv[a] = gp->sc.grid_inv[a];
    }
    *cells = gp->sc.grid ? GRID_G : 0;
    *bins = GRID_B;
    return PT_OK;
}

int32_t pt_test_sort(const pt_shadeable_isect* isects, int64_t n, int32_t* perm) {
    RC(need_init());
    RC(need_single("pt_test_sort"));
    RC(ensure_test_paths(n));
    if (n == 0) return PT_OK;
    const int nk = std::max(1, gp->sc.num_mats);
    std::vector<int> mat(n);
    for (int64_t i = 0; i < n; ++i) {
        mat[i] = isects[i].materialId;
        if (mat[i] < 0 || mat[i] >= nk) return fail(PT_E_INVALID, "materialId %d out of range", mat[i]);
    }
    HIPCHK(smemcpy(gp->d_hit_mat, mat.data(), n * sizeof(int), hipMemcpyHostToDevice));
    RC(set_count(0, (int)n));
    const int ntiles = (int)((n + STILE - 1) / STILE);
    hipLaunchKernelGGL(k_sort_hist, dim3(ntiles), dim3(BLOCK), 0, gp->stream, gp->d_hit_mat, staged_count(0), nk,
                       gp->d_tile_hist);
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(SCAN_THREADS), 0, gp->stream, gp->d_tile_hist, staged_count(0), nk);
    hipLaunchKernelGGL(k_sort_scatter, dim3(ntiles), dim3(BLOCK), 0, gp->stream, gp->d_hit_mat, staged_count(0), nk,
                       gp->key_bits, gp->d_tile_hist, gp->d_perm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(gp->stream));
    HIPCHK(smemcpy(perm, gp->d_perm, n * sizeof(int), hipMemcpyDeviceToHost));
    release_graph();
    RC(ctl_reset());
    return PT_OK;
}

int32_t pt_test_rng(const int32_t* iid, int64_t m, int32_t n, float* out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_E_NODEVICE, "no HIP device visible");
    if (m <= 0 || n <= 0) return PT_OK;
    int* d_iid = nullptr;
    float* d_out = nullptr;
    HIPCHK(hipMalloc(&d_iid, sizeof(int) * 3 * m));
    HIPCHK(hipMalloc(&d_out, sizeof(float) * m * n));
    HIPCHK(smemcpy(d_iid, iid, sizeof(int) * 3 * m, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rng, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, d_iid, (int)m, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(smemcpy(out, d_out, sizeof(float) * m * n, hipMemcpyDeviceToHost));
    (void)hipFree(d_iid);
    (void)hipFree(d_out);
    return PT_OK;
}

int32_t pt_test_pbo(const float* image, int64_t n, int32_t iteration, pt_uchar4* pbo) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_E_NODEVICE, "no HIP device visible");
    if (n <= 0) return PT_OK;
    float* d_img = nullptr;
    pt_uchar4* d_pbo = nullptr;
    HIPCHK(hipMalloc(&d_img, sizeof(float) * 3 * n));
    HIPCHK(hipMalloc(&d_pbo, sizeof(pt_uchar4) * n));
    HIPCHK(smemcpy(d_img, image, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_to_pbo, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0, d_img, d_pbo, (int)n,
                       iteration);
    HIPCHK(hipGetLastError());
    HIPCHK(smemcpy(pbo, d_pbo, sizeof(pt_uchar4) * n, hipMemcpyDeviceToHost));
    (void)hipFree(d_img);
    (void)hipFree(d_pbo);
    return PT_OK;
}

int32_t pt_debug_section_counters(uint64_t* out, int32_t n, int32_t reset) {
    RC(need_init());
    if (!out || n < 0 || n > SEC_SLOTS) return fail(PT_E_INVALID, "bad arguments");
    HIPCHK(hipStreamSynchronize(gp->stream));
    unsigned long long tmp[SEC_SLOTS];
    HIPCHK(hipMemcpyFromSymbolAsync(tmp, HIP_SYMBOL(g_sections), sizeof tmp, 0, hipMemcpyDeviceToHost, gp->stream));
    HIPCHK(hipStreamSynchronize(gp->stream));
    for (int i = 0; i < n; ++i) out[i] = tmp[i];
    if (reset) {
        memset(tmp, 0, sizeof tmp);
        HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_sections), tmp, sizeof tmp, 0, hipMemcpyHostToDevice, gp->stream));
        HIPCHK(hipStreamSynchronize(gp->stream));
    }
    return PT_OK;
}

int32_t pt_profile_frames(int32_t first_iteration, int32_t count, pt_kernel_times* out) {
    RC(need_init());
    RC(need_single("pt_profile_frames"));
    if (!out || count <= 0) return fail(PT_E_INVALID, "bad arguments");
    memset(out, 0, sizeof(*out));
    RC(ensure_frames(pass_frames(count)));
    // the same passes as pt_trace_frames, launched eagerly with per-dispatch start/stop events,
    // no host synchronisation until the end; stream-level events around the whole run
    std::vector<ProfRec> rec;
    std::vector<size_t> pass_start;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    {   // every kernel of every pass gets a start and a stop event, created up front
        const int passes = (count + gp->batch - 1) / gp->batch;
        const size_t need = 2 * (size_t)passes * (size_t)(4 * std::max(1, gp->sc.trace_depth) + 8);
        while (g_prof_pool.size() < need) {
            hipEvent_t e = nullptr;
            HIPCHK(hipEventCreateWithFlags(&e, PROF_EVENT_FLAGS));
            g_prof_pool.push_back(e);
        }
        g_prof_next = 0;
    }
    HIPCHK(hipEventRecord(e0, gp->stream));
    g_prof = &rec;
    int rc = PT_OK;
    for (int i = 0; i < count && rc == PT_OK;) {
        const int f = pass_frames(count - i);
        pass_start.push_back(rec.size());
        rc = enqueue_pass(first_iteration + i, f);
        gp->dev_iter = first_iteration + i;
        gp->frames_done += f;
        gp->last_iter = first_iteration + i + f - 1;
        i += f;
    }
    g_prof = nullptr;
    (void)hipEventRecord(e1, gp->stream);
    hipError_t se = hipStreamSynchronize(gp->stream);
    const int passes = (int)pass_start.size();
    double bounce_ms[MAXB] = {0}, bvh_ms[MAXB] = {0};
    double compact_ms = 0, isect_ms = 0, shade_ms = 0, cam_ms = 0, sort_ms = 0, scan_ms = 0, comb_ms = 0, tail_ms = 0;
    int tail_from = 0;
    float frame_ms = 0;
    if (rc == PT_OK && se == hipSuccess) {
        (void)hipEventElapsedTime(&frame_ms, e0, e1);
        for (int f = 0; f < passes; ++f) {
            size_t a = pass_start[f], b = (f + 1 < passes) ? pass_start[f + 1] : rec.size();
            int bi = 0, ni = 0;
            for (size_t i = a; i < b; ++i) {
                float ms = 0;
                (void)hipEventElapsedTime(&ms, rec[i].start, rec[i].stop);
                int k = rec[i].kind;
                if (k >= 400) { bounce_ms[k - 400] += ms; bvh_ms[k - 400] += ms; }   // k_bvh_tail_trav / _shade
                else if (k >= 300) { tail_ms += ms; tail_from = k - 300; }
                else if (k >= 200) { bounce_ms[k - 200] += ms; bvh_ms[k - 200] += ms; }
                else if (k >= 100) bounce_ms[k - 100] += ms;
                else if (k == 0) cam_ms += ms;
                else if (k == 1) isect_ms += ms;
                else if (k == 2) shade_ms += ms;
                else if (k == 3) { compact_ms += ms; if (bi < MAXB) bounce_ms[bi++] += ms; }
                else if (k == 5) scan_ms += ms;
                else if (k == 4) sort_ms += ms;
                else if (k == 6) comb_ms += ms;
                else if (k == 7) { isect_ms += ms; if (ni < MAXB) bvh_ms[ni++] += ms; }   // k_naive_mesh of bounce ni
            }
        }
    }
    for (auto e : g_prof_pool) (void)hipEventDestroy(e);
    g_prof_pool.clear();
    g_prof_next = 0;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    RC(rc);
    HIPCHK(se);
    out->frames = count;
    out->passes = passes;
    out->frame_ms = frame_ms / count;
    for (int b = 0; b < MAXB; ++b) {
        out->bounce_ms[b] = (float)(bounce_ms[b] / passes);
        out->bvh_ms[b] = (float)(bvh_ms[b] / passes);
    }
    out->combine_ms = (float)(comb_ms / count);
    out->compact_ms = (float)(compact_ms / count);
    out->intersect_ms = (float)(isect_ms / count);
    out->shade_ms = (float)(shade_ms / count);
    out->camera_ms = (float)(cam_ms / count);
    out->sort_ms = (float)(sort_ms / count);
    out->compact_scan_ms = (float)(scan_ms / count);
    out->tail_ms = (float)(tail_ms / passes);
    out->tail_from = tail_from;
    return PT_OK;
}
