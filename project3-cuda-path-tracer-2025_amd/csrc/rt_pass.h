// rt_pass.h — one pass of the frame loop: which kernels it launches, and its captured graph.
//
// Owns: the table of fused kernel variants and the dispatch from a run-time variant to its
// template instance (launch_bounce), effective_variant / head_fused / tail_from, the staged
// compaction's launch sequence, enqueue_pass (a pass's kernels on gp->stream), build_graph /
// release_pass_graphs, pass_frames.
// Calls: rt_core.h and the kernels.  It reads the buffers rt_buffers.h sizes but calls nothing
// of it: run_pass, which needs both, is in pt_runtime.hip.

// ---- the fused kernel variants ------------------------------------------------------------------
// Every VAR_* combination the fused kernels are built for, ONCE: the switch of launch_bounce_v
// and variant_compiled are both generated from these two lists, so a variant cannot be launchable
// without being admitted or the other way round (pt_init refuses every other value instead of
// running a different kernel than asked for).  X: full builds only; P: also in a PT_VAR_PROBE
// build (tools: register-pressure probes compile only the default variants).
//   154 / 186: the defaults (186: + VAR_BVH_SPLIT); 158 / 190: + section counters; 54: split +
//   section counters; 30: redist + pair counters; 666 / 698: 154 / 186 + material grouping, and
//   530 / 562 their camera bounces; 3: candidate queue + one compaction atomic per wave (every
//   build has carried it, until now as the switch's fall-through).
#define PT_FUSED_VARIANTS(X, P) \
    X(0) X(1) X(2) X(6) X(10) X(18) X(26) X(22) X(50) X(58) X(54) X(30) P(154) P(186) X(190) X(158) X(666) X(530) X(698) \
    X(562) P(3)
// ... and those also built without texture fetches (VAR_NO_TEX: no textured / bump-mapped
// material): the default variants with their section-counter and material-grouping forms
#define PT_FUSED_VARIANTS_NO_TEX(X, P) P(18) P(22) P(50) P(54) P(154) P(158) P(186) P(190) X(530) X(562) X(666) X(698)
#ifdef PT_VAR_PROBE
#define PT_VARIANT_SKIP(v)
#define PT_EACH_VARIANT(F) PT_FUSED_VARIANTS(PT_VARIANT_SKIP, F)
#define PT_EACH_VARIANT_NO_TEX(F) PT_FUSED_VARIANTS_NO_TEX(PT_VARIANT_SKIP, F)
#else
#define PT_EACH_VARIANT(F) PT_FUSED_VARIANTS(F, F)
#define PT_EACH_VARIANT_NO_TEX(F) PT_FUSED_VARIANTS_NO_TEX(F, F)
#endif

// Is this effective variant one of the table's?  3 is: it was instantiated all along and init_one
// let it through by a special case.  Listing it changes no decision: init_one admitted it before,
// effective_variant's VAR_NO_TEX probe asks about the second list only, and the material-group
// probe only about values with VAR_MAT_GROUP (512) set.
// A PT_VAR_PROBE build (tools only) does change: the list used to ignore the define, so such a
// build admitted variants it had not instantiated and ran them as variant 3's kernel; now pt_init
// refuses them there too (a textured scene's camera bounce, variant 18, for one).
bool variant_compiled(int v) {
    switch (v) {
#define PT_LISTED(n) case n:
#define PT_LISTED_NO_TEX(n) case VAR_NO_TEX + n:
        PT_EACH_VARIANT(PT_LISTED)
        PT_EACH_VARIANT_NO_TEX(PT_LISTED_NO_TEX)
#undef PT_LISTED
#undef PT_LISTED_NO_TEX
            return true;
        default: return false;
    }
}

// f(std::true_type / std::false_type): a run-time flag chosen once as a template argument, so
// that a launch whose kernel differs by that flag alone is written once
template <class F>
void with_flag(bool on, F&& f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// bytes of the block's LDS geom table (lds_geom_f4 on the device)
size_t geom_table_lds() {
    return (sizeof(DevGeomHot) + (gp->sc.grid ? sizeof(DevCull) : 0)) * (size_t)gp->sc.num_geoms;
}

// device-side counter of the input of bounce b in the staged pipeline
const int* staged_count(int b) { return &gp->d_ctl->cnt[b][0][0]; }

template <bool FIRST, bool HAS_BVH, int VAR>
void launch_bounce_t(dim3 grid, PathBuf in, PathBuf out, int b) {
    constexpr bool SPLIT = HAS_BVH && (VAR & VAR_BVH_SPLIT);
    const bool lds = (VAR & (VAR_CAND_QUEUE | VAR_WAVE_REDIST)) && gp->sc.num_geoms <= LDS_GEOMS;
    const size_t geom_lds = lds ? geom_table_lds() : 0;
    // the exchange's region: block_intersect's BlockLds, or one WaveLds per wave (wave_intersect)
    const size_t redist_lds = (VAR & VAR_WAVE_REDIST) && lds
                                  ? ((VAR & VAR_BLOCK_REDIST) ? sizeof(BlockLds) : sizeof(WaveLds) * (BLOCK / 64))
                                  : 0;
    const size_t stack_lds = HAS_BVH && !SPLIT ? gp->bvh_lds : 0;
    // VAR_MAT_GROUP's exchange reuses the exact-test exchange's region (it runs after it)
    const size_t xchg_lds = (VAR & VAR_MAT_GROUP) ? std::max(redist_lds, mat_group_lds(HAS_BVH, false)) : redist_lds;
    // tools: unused LDS added to k_bounce / the traversal kernel (occupancy A/B)
    const size_t bounce_pad = gp->tune.bounce_lds_pad;
    launch(100 + b, k_bounce<FIRST, HAS_BVH, VAR>, grid, dim3(BLOCK), geom_lds + stack_lds + xchg_lds + bounce_pad, gp->sc,
           in, out, gp->d_ctl, gp->d_image, b, gp->seg_stride, gp->queue);
    const size_t lds_pad = gp->tune.bvh_lds_pad;
    if (SPLIT) {
        const size_t stack_bytes = (size_t)gp->sc.stack_lds * BLOCK * sizeof(int);
        // the handed-over stacks were sized for the pair tree of the allocation (ensure_frames)
        if (gp->tail_lanes > 0 && gp->sc.stack_lds > gp->tail_depth) gp->tail_lanes = 0;
        const bool quads = gp->sc.quads != nullptr;   // the 4-wide layout (trees past the L2)
        with_flag(quads, [&](auto quad) {
            launch(200 + b, k_bvh_bounce<VAR, quad.value>, grid, dim3(BLOCK), stack_bytes + lds_pad, gp->sc, gp->queue,
                   gp->tail, gp->tail_lanes, out, gp->d_ctl, gp->d_image, b, gp->seg_stride);
        });
        if (gp->tail_lanes > 0) {   // the handed-over rays: refilling waves, then their shading
            with_flag(quads, [&](auto quad) {
                launch(400 + b, k_bvh_tail_trav<VAR, quad.value>, dim3(NSEG * gp->tail_trav_blocks), dim3(BLOCK),
                       stack_bytes, gp->sc, gp->queue, gp->tail, gp->d_ctl, b, gp->tail_refill);
            });
            const int per_seg = gp->tail_shade_blocks > 0 ? std::min(gp->tail_shade_blocks, nblocks(gp->tail.stride))
                                                          : nblocks(gp->tail.stride);
            launch(400 + b, k_bvh_tail_shade<VAR>, dim3(NSEG * per_seg), dim3(BLOCK), 0, gp->sc,
                   gp->queue, gp->tail, out, gp->d_ctl, gp->d_image, b, gp->seg_stride);
        }
    }
}
template <bool FIRST, bool HAS_BVH>
void launch_bounce_v(int var, dim3 grid, PathBuf in, PathBuf out, int b) {
    switch (var) {
#define PT_CASE(v) case v: launch_bounce_t<FIRST, HAS_BVH, v>(grid, in, out, b); break;
#define PT_CASE_NO_TEX(v) case VAR_NO_TEX + v: launch_bounce_t<FIRST, HAS_BVH, VAR_NO_TEX + v>(grid, in, out, b); break;
        PT_EACH_VARIANT(PT_CASE)
        PT_EACH_VARIANT_NO_TEX(PT_CASE_NO_TEX)
#undef PT_CASE
#undef PT_CASE_NO_TEX
        default: break;   // unreachable: pt_init refuses what variant_compiled does not list
    }
}
// the fused kernel's template variant for a bounce: the requested bits minus what this bounce /
// scene does not use
int effective_variant(bool first, int var) {
    var &= ~(VAR_BVH_NODES | VAR_NO_TEX);   // host-only bits (layout choice; texture-free build: below)
    // camera rays of neighbouring pixels share their candidates: redistribution only costs there
    // (A/B: bounce 0 0.164 -> 0.174 ms, bounces 1-7 ~6 % faster)
    if (first) var &= ~(VAR_WAVE_REDIST | VAR_BLOCK_REDIST);
    // tools: PT_SECTIONS_SKIP_CAMERA=1 leaves the camera bounce out of the section counters
    if (first && gp->tune.sections_skip_camera) var &= ~VAR_SECTION_TIMING;
    if (!gp->split) var &= ~VAR_BVH_SPLIT;
    // the texture-free build exists for the default variants (and their section-counter and
    // material-grouping forms); other variants keep the texture code
    if (gp->no_tex && variant_compiled(var | VAR_NO_TEX)) var |= VAR_NO_TEX;
    return var;
}
void launch_bounce(bool first, bool bvh, int var, dim3 grid, PathBuf in, PathBuf out, int b) {
    var = effective_variant(first, var);
    if (first) {
        if (bvh) launch_bounce_v<true, true>(var, grid, in, out, b);
        else launch_bounce_v<true, false>(var, grid, in, out, b);
    } else {
        if (bvh) launch_bounce_v<false, true>(var, grid, in, out, b);
        else launch_bounce_v<false, false>(var, grid, in, out, b);
    }
}

// stable compaction of the n_in paths of `pi` into `po` (three launches, see k_compact_*)
template <int CITEMS>
void launch_compact(PathBuf pi, PathBuf po, const int* n_in, int* n_out, int npaths) {
    constexpr int CTILE = BLOCK * CITEMS;
    const int ntiles = (npaths + CTILE - 1) / CTILE;
    launch(5, k_compact_count<CITEMS>, dim3(ntiles), dim3(BLOCK), 0, (const int*)gp->d_alive, n_in, gp->d_tile_cnt);
    launch(5, k_compact_scan, dim3(1), dim3(SCAN_THREADS), 0, (const int*)gp->d_tile_cnt, n_in, gp->d_tile_off, n_out,
           CTILE);
    launch(3, k_compact_scatter<CITEMS>, dim3(ntiles), dim3(BLOCK), 0, (const float4*)pi.A, (const float4*)pi.B,
           (const float4*)pi.C, po.A, po.B, po.C, (const int*)gp->d_alive, n_in, (const int*)gp->d_tile_off);
}

// Enqueue one pass's kernels (everything after k_frame_begin) on gp->stream: `batch` frames
// traced together as one wavefront of local_pixels x batch paths.
// single-frame passes of primitive-only scenes run bounces tail_from() .. depth-1 as one k_tail
// launch (PT_TAIL=0 turns it off for A/B); 0: no tail launch
// Bounces 0 and 1 as one k_head launch (PT_HEAD_FUSE=0 turns it off for A/B): primitive-only
// scenes whose geom table fits in LDS, on the default kernel variants only (no section counters,
// no material grouping), passes of any number of frames.
bool head_fused() {
    constexpr int V0 = VAR_CAND_QUEUE | VAR_BVH_FAST;
    constexpr int V1 = VAR_CAND_QUEUE | VAR_WAVE_REDIST | VAR_BVH_FAST | VAR_BLOCK_REDIST;
    const int var = gp->opts.variant & ~VAR_BVH_NODES;
    return gp->tune.head_fuse && gp->opts.pipeline == PT_PIPELINE_FUSED && !gp->has_bvh &&
           gp->sc.num_geoms <= LDS_GEOMS && gp->sc.trace_depth >= 2 &&
           (effective_variant(true, var) & ~VAR_NO_TEX) == V0 && (effective_variant(false, var) & ~VAR_NO_TEX) == V1;
}
int tail_from(int batch) {
    const int depth = gp->sc.trace_depth;
    const bool lds = gp->sc.num_geoms <= LDS_GEOMS;
    if (gp->tune.tail_off || (batch != 1 && !gp->tune.tail_any_batch) || gp->has_bvh || !lds || depth < 3 ||
        (effective_variant(false, gp->opts.variant) & ~VAR_NO_TEX) !=
            (VAR_CAND_QUEUE | VAR_WAVE_REDIST | VAR_BVH_FAST | VAR_BLOCK_REDIST))
        return 0;
    const int from = gp->tune.tail_from;
    // k_head traces bounce 1 itself: the tail then starts at bounce 2 at the earliest
    return std::min(depth - 1, std::max(head_fused() ? 2 : 1, from > 0 ? from : depth / 2));
}

int enqueue_pass_body(int batch) {
    const int depth = gp->sc.trace_depth;
    const int npaths = gp->local_pixels * batch;
    const int nb = nblocks(npaths);
    const int nbounces = std::max(1, depth);
    if (gp->opts.pipeline == PT_PIPELINE_FUSED) {
        const int t = tail_from(batch);
        const bool head = head_fused();
        if (head) {   // bounces 0 and 1; profiled as bounce 0 (bounce 1's entry stays 0)
            const size_t lds = geom_table_lds() + sizeof(BlockLds) + gp->tune.bounce_lds_pad;
            with_flag(gp->no_tex, [&](auto no_tex) {
                launch(100, k_head<no_tex.value ? VAR_NO_TEX : 0>, dim3(nb), dim3(BLOCK), lds, gp->sc, pathbuf(0),
                       gp->d_ctl, gp->d_image, gp->seg_stride);
            });
            HIPCHK(hipGetLastError());
        }
        for (int b = head ? 2 : 0; b < (t ? t : nbounces); ++b) {
            PathBuf in = pathbuf(b & 1), out = pathbuf((b + 1) & 1);
            launch_bounce(b == 0, gp->has_bvh, gp->opts.variant & ~VAR_BVH_NODES, dim3(nb), in, out, b);
            HIPCHK(hipGetLastError());
        }
        if (t) {
            constexpr int V = VAR_CAND_QUEUE | VAR_WAVE_REDIST | VAR_BVH_FAST | VAR_BLOCK_REDIST;
            const size_t lds = geom_table_lds() + sizeof(BlockLds);
            with_flag(gp->no_tex, [&](auto no_tex) {
                launch(300 + t, k_tail<V | (no_tex.value ? VAR_NO_TEX : 0)>, dim3(nb), dim3(BLOCK), lds, gp->sc,
                       pathbuf(t & 1), gp->d_ctl, gp->d_image, t, gp->seg_stride, depth);
            });
            HIPCHK(hipGetLastError());
        }
        return PT_OK;
    }
    // STAGED (k_combine after the pass is enqueued by enqueue_pass)
    // STAGED
    launch(0, k_camera, dim3(nb), dim3(BLOCK), 0, gp->sc, pathbuf(0), gp->d_ctl);
    HIPCHK(hipGetLastError());
    const int stiles = (npaths + STILE - 1) / STILE;   // material-sort tiles
    int cur = 0;
    for (int b = 0; b < nbounces; ++b) {
        // compaction off: paths never move, every bounce sees all of them (pathtrace.cu:690)
        const int* n_in = gp->opts.stream_compaction ? staged_count(b) : staged_count(0);
        HitBuf hits{gp->d_hit_nt, gp->d_hit_mat, gp->d_hit_uvd0, gp->d_hit_uvd1};
        if (gp->has_bvh && (gp->opts.variant & VAR_BVH_FAST))
            launch(1, k_intersect<true, true>, dim3(nb), dim3(BLOCK), gp->bvh_lds, gp->sc, pathbuf(cur), hits, n_in);
        else if (gp->has_bvh)
            launch(1, k_intersect<true, false>, dim3(nb), dim3(BLOCK), gp->bvh_lds, gp->sc, pathbuf(cur), hits, n_in);
        else
            launch(1, k_intersect<false, false>, dim3(nb), dim3(BLOCK), 0, gp->sc, pathbuf(cur), hits, n_in);
        // NAIVE_MESH_LOADING: every triangle in array order against the records just written
        if (gp->naive && gp->sc.num_tris > 0)
            launch(7, k_naive_mesh, dim3(nb), dim3(BLOCK), 0, gp->sc, (const DevTriHot*)gp->d_naive_hot, gp->sc.num_tris,
                   pathbuf(cur), hits.nt, hits.mat, hits.uvd0, hits.uvd1, n_in);
        HIPCHK(hipGetLastError());
        const int* perm = nullptr;
        if (gp->opts.material_sort) {
            const int nk = std::max(1, gp->sc.num_mats);
            launch(4, k_sort_hist, dim3(stiles), dim3(BLOCK), 0, (const int*)gp->d_hit_mat, n_in, nk, gp->d_tile_hist);
            launch(4, k_sort_scan, dim3(1), dim3(SCAN_THREADS), 0, gp->d_tile_hist, n_in, nk);
            launch(4, k_sort_scatter, dim3(stiles), dim3(BLOCK), 0, (const int*)gp->d_hit_mat, n_in, nk, gp->key_bits,
                   (const int*)gp->d_tile_hist, gp->d_perm);
            HIPCHK(hipGetLastError());
            perm = gp->d_perm;
        }
        launch(2, k_shade, dim3(nb), dim3(BLOCK), 0, gp->sc, pathbuf(cur), hits, perm, n_in, (const FrameCtl*)gp->d_ctl,
               0, gp->d_image, gp->opts.stream_compaction ? gp->d_alive : (int*)nullptr);
        HIPCHK(hipGetLastError());
        if (gp->opts.stream_compaction) {
            PathBuf pi = pathbuf(cur), po = pathbuf(cur ^ 1);
            int* n_out = &gp->d_ctl->cnt[b + 1][0][0];
            launch_compact<CITEMS>(pi, po, n_in, n_out, npaths);
            HIPCHK(hipGetLastError());
            cur ^= 1;
        }
    }
    return PT_OK;
}

int enqueue_pass(int set_iter, int batch, int plane = 0) {
    gp->ctl_rows = std::max(gp->ctl_rows, std::min(MAXB + 1, gp->sc.trace_depth + 1));
    launch(-1, k_frame_begin, dim3(1), dim3(256), 0, gp->d_ctl, set_iter, gp->local_pixels, batch, gp->ctl_rows, plane);
    HIPCHK(hipGetLastError());
    RC(enqueue_pass_body(batch));
    if (batch > 1) {
        launch(6, k_combine, dim3(nblocks(gp->local_pixels)), dim3(BLOCK), 0, gp->sc, (const FrameCtl*)gp->d_ctl,
               gp->d_image);
        HIPCHK(hipGetLastError());
    }
    return PT_OK;
}

int build_graph(int batch) {
    HIPCHK(hipStreamBeginCapture(gp->stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_pass(0, batch);
    hipGraph_t gr = nullptr;
    hipError_t e = hipStreamEndCapture(gp->stream, &gr);
    if (rc != PT_OK) return rc;
    HIPCHK(e);
    gp->graph[batch] = gr;
    HIPCHK(hipGraphInstantiate(&gp->graph_exec[batch], gr, nullptr, nullptr, 0));
    return PT_OK;
}
// the captured passes (release_graph, rt_spec.h, releases the speculative frame's with them)
void release_pass_graphs() {
    for (int f = 0; f <= MAXF; ++f) {
        if (gp->graph_exec[f]) (void)hipGraphExecDestroy(gp->graph_exec[f]);
        if (gp->graph[f]) (void)hipGraphDestroy(gp->graph[f]);
        gp->graph_exec[f] = nullptr;
        gp->graph[f] = nullptr;
    }
}

// frames of the next pass when `remaining` frames are left: the passes of a run are balanced
// (100 frames at F = 32 -> 4 x 25, not 32 + 32 + 32 + 4: a small last pass runs its launches
// with a fraction of the paths in flight at nearly full per-launch cost)
int pass_frames(int remaining) {
    const int passes = (remaining + gp->batch - 1) / gp->batch;
    return (remaining + passes - 1) / passes;
}

