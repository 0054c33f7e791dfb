// pt_pass_kernels.h — the kernels of a pass of the fused pipeline, and of what surrounds a pass.
//
//   k_frame_begin, k_combine            frame control, the planes of a multi-frame pass
//   k_spec_sum, k_adopt_frame           single-frame speculation
//   k_pack_tile, k_gather_shards        several devices: a shard's pixels into the first device's image
//   k_bounce, k_tail, k_head            one bounce / the last bounces / the first two, per launch
//   k_bvh_bounce, k_bvh_tail_trav, k_bvh_tail_shade   the split BVH traversal behind QueueBuf / TailBuf
//
// Included by pt_runtime.hip alone, at global scope after its `using namespace ptd`, before
// pt_staged_kernels.h: the kernels keep the names and the order they had inside that file.
#pragma once

#include "pt_kernels.h"

// Fold the previous pass's live counts into the running totals, advance (or set) the
// iteration, zero the per-pass counters and start a pass of `batch` frames.  One block.
// `rows`: the counter rows any pass since the last reset of the block wrote (trace depth + 1 at
// most; the rest stay zero), so a frame clears 9 rows of 8 segments at depth 8, not 65.
__global__ void k_frame_begin(FrameCtl* ctl, int set_iter, int local_pixels, int batch, int rows, int plane) {
    int t = threadIdx.x;
    if (ctl->frames > 0) {
        for (int b = t; b < rows; b += blockDim.x) {
            unsigned long long s = 0;
            for (int k = 0; k < NSEG; ++k) s += (unsigned)ctl->cnt[b][k][0];
            ctl->tot[b] += s;
            unsigned long long q = 0, h = 0, hs = 0;
            for (int k = 0; k < NSEG; ++k) {
                q += (unsigned)ctl->qcnt[b][k][0];
                h += (unsigned)ctl->qcnt[b][k][3];
                hs += (unsigned)ctl->qcnt[b][k][4];
            }
            ctl->qtot[b] += q;
            ctl->htot[b] += h;
            ctl->hstk[b] += hs;
        }
    }
    __syncthreads();
    for (int i = t; i < rows * NSEG; i += blockDim.x) (&ctl->cnt[0][0][0])[i * CNT_PAD] = 0;
    for (int i = t; i < rows * NSEG; i += blockDim.x) {
        (&ctl->qcnt[0][0][0])[i * CNT_PAD] = 0;
        (&ctl->qcnt[0][0][0])[i * CNT_PAD + 1] = 0;   // handed-over traversals
        (&ctl->qcnt[0][0][0])[i * CNT_PAD + 2] = 0;   // ... and those taken by k_bvh_tail_trav
        (&ctl->qcnt[0][0][0])[i * CNT_PAD + 3] = 0;   // handed-over traversals stored (stats)
        (&ctl->qcnt[0][0][0])[i * CNT_PAD + 4] = 0;   // ... and their stack entries (stats)
    }
    __syncthreads();
    if (t == 0) {
        ctl->iter = set_iter > 0 ? set_iter : ctl->iter + 1;
        ctl->batch = batch;
        ctl->plane = plane;
        ctl->cnt[0][0][0] = local_pixels * batch;
        ctl->frames += batch;
    }
}

PT_DEV uint64_t lanemask_lt() {
    uint32_t lane = threadIdx.x & 63u;
    return lane == 0 ? 0ull : (~0ull >> (64u - lane));
}
PT_DEV int mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// A pixel receives one contribution per frame (finalGather, pathtrace.cu:217-227, adds every
// path's colour once).  Single-frame pass: add it now.  Pass of F > 1 frames: store it in the
// frame's contribution plane; k_combine adds the planes in frame order afterwards, so the
// image sees the same float additions in the same order as F sequential frames.
PT_DEV void gather_into_image(float* image, const SceneDev& sc, bool to_plane, const PathReg& p) {
    if (to_plane) {
        float* px = sc.contrib + 3 * ((size_t)p.slot * (size_t)(sc.cam.resx * sc.cam.resy) + (size_t)p.pix);
        px[0] = p.c.x;
        px[1] = p.c.y;
        px[2] = p.c.z;
        return;
    }
    float* px = image + 3 * (size_t)p.pix;
    px[0] += p.c.x;
    px[1] += p.c.y;
    px[2] += p.c.z;
}

// end of a pass of F > 1 frames: image += plane 0, += plane 1, ... (local pixels only)
__global__ __launch_bounds__(BLOCK) void k_combine(SceneDev sc, const FrameCtl* ctl, float* __restrict__ image) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= sc.shard.local_pixels) return;
    const int batch = ctl->batch;
    if (batch <= 1) return;
    const size_t pix = (size_t)shard_pixel(sc, l);
    const size_t plane = (size_t)sc.cam.resx * sc.cam.resy;
    float* px = image + 3 * pix;
    float r = px[0], gch = px[1], b = px[2];
    const float* c = sc.contrib + 3 * pix;
    for (int k = 0; k < batch; ++k, c += 3 * plane) {
        r += c[0];
        gch += c[1];
        b += c[2];
    }
    px[0] = r;
    px[1] = gch;
    px[2] = b;
}

// A speculative single frame (spec_*).  At its end, on its own stream, k_spec_sum forms the image
// the call for its iteration will return: image + its plane (the same float additions, in the same
// order, as its paths' gathers into the image would have made), into a buffer of its own -- so
// that call copies it to the host at once, while k_adopt_frame makes it the image and gives the
// caller's FrameCtl the frame's counters (the previous frame folded into the running totals and
// the speculative frame's live counts in its place, as k_frame_begin and that frame's kernels
// would have left them).  Whole images, as float4 streams (single context, no pixel shards).
__global__ __launch_bounds__(BLOCK) void k_spec_sum(const float* __restrict__ image, const float* __restrict__ plane,
                                                    float* __restrict__ out, int nf) {
    const int i = 4 * (blockIdx.x * BLOCK + threadIdx.x);
    if (i + 3 < nf) {
        float4 x = *reinterpret_cast<const float4*>(image + i);
        const float4 c = *reinterpret_cast<const float4*>(plane + i);
        x.x += c.x;
        x.y += c.y;
        x.z += c.z;
        x.w += c.w;
        *reinterpret_cast<float4*>(out + i) = x;
    } else {
        for (int k = i; k < nf; ++k) out[k] = image[k] + plane[k];
    }
}
__global__ __launch_bounds__(BLOCK) void k_adopt_frame(const float* __restrict__ sum, float* __restrict__ image, int nf,
                                                       FrameCtl* ctl, const FrameCtl* spec, int rows) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {   // one thread per (bounce row, segment): all the loads at once
        const bool fold = ctl->frames > 0;
        for (int i = t; i < rows * NSEG; i += BLOCK) {
            int* c = &ctl->cnt[0][0][0] + i * CNT_PAD;
            int* q = &ctl->qcnt[0][0][0] + i * CNT_PAD;
            const int c0 = *c, q0 = q[0], h0 = q[3], hs0 = q[4];
            const int* qs = &spec->qcnt[0][0][0] + i * CNT_PAD;
            const int c1 = (&spec->cnt[0][0][0])[i * CNT_PAD], q1 = qs[0], h1 = qs[3], hs1 = qs[4];
            const int b = i / NSEG;
            if (fold && c0) atomicAdd(&ctl->tot[b], (unsigned long long)(unsigned)c0);
            if (fold && q0) atomicAdd(&ctl->qtot[b], (unsigned long long)(unsigned)q0);
            if (fold && h0) atomicAdd(&ctl->htot[b], (unsigned long long)(unsigned)h0);
            if (fold && hs0) atomicAdd(&ctl->hstk[b], (unsigned long long)(unsigned)hs0);
            *c = c1;
            q[0] = q1;
            q[3] = h1;
            q[4] = hs1;
        }
        __syncthreads();   // every thread read `frames` before it changes
        if (t == 0) {
            ctl->iter = spec->iter;
            ctl->batch = 1;
            ctl->plane = 0;
            ctl->frames += 1;
        }
    }
    const int i = 4 * (blockIdx.x * BLOCK + t);
    if (i + 3 < nf) {
        *reinterpret_cast<float4*>(image + i) = *reinterpret_cast<const float4*>(sum + i);
    } else {
        for (int k = i; k < nf; ++k) image[k] = sum[k];
    }
}

// Multi-device combine (pt_options.num_devices > 1): shard k owns the pixels
// shard_pixel_of(sh_k, W, l), l < sh_k.local_pixels, of every shard image; the first device's
// image receives them after each call.  Plain copies: the image is bit-identical to one device's.
__global__ __launch_bounds__(BLOCK) void k_pack_tile(const float* __restrict__ image, ShardDev sh, int W,
                                                     float* __restrict__ tile) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= sh.local_pixels) return;
    const size_t pix = 3 * (size_t)shard_pixel_of(sh, W, l);
    tile[3 * (size_t)l] = image[pix];
    tile[3 * (size_t)l + 1] = image[pix + 1];
    tile[3 * (size_t)l + 2] = image[pix + 2];
}
// The whole combine in ONE launch on the first device: every pixel of the frame finds its shard
// from its row band ((y / rows) % n) and copies its float3 from that shard's source -- the shard's
// own image over xGMI peer access (`local` 0: indexed by the global pixel), or the packed tile
// that RCCL / a peer copy brought over (`local` 1: indexed by the shard's local pixel).  All
// shards' reads are in flight together (on N GPUs: every xGMI link at once), instead of one
// launch per shard one after another.  Shard 0's pixels are already in place.
struct GatherSrc {
    const float* src[PT_MAX_DEVICES];
    int local[PT_MAX_DEVICES];
    int n, rows, W, H;
};
__global__ __launch_bounds__(BLOCK) void k_gather_shards(float* __restrict__ image, GatherSrc g) {
    const int pix = blockIdx.x * BLOCK + threadIdx.x;
    if (pix >= g.W * g.H) return;
    const int y = pix / g.W, x = pix - y * g.W;
    const int band = y / g.rows;
    const int k = band % g.n;
    if (k == 0) return;
    const int lrow = (band / g.n) * g.rows + (y - band * g.rows);
    const size_t i = 3 * (size_t)(g.local[k] ? lrow * g.W + x : pix);
    const float* s = g.src[k];
    const float r = s[i], gch = s[i + 1], b = s[i + 2];
    float* px = image + 3 * (size_t)pix;
    px[0] = r;
    px[1] = gch;
    px[2] = b;
}

// --------------------------------------------------------------------------------------------
// FUSED: camera (bounce 0) | load -> intersect -> shade -> gather dead -> compact survivors
// --------------------------------------------------------------------------------------------
// VAR_BVH_SPLIT traversal queue: the path (3 float4 as in PathBuf, C.w = frame slot | (winner
// geom + 1) << 8) and the primitive result it enters traversal with (t_min, normal seed)
struct QueueBuf {
    float4 *A, *B, *C, *D;   // D = t_min | seed.xyz
    int stride;              // entries per queue segment (segment s at s * stride, FrameCtl::qcnt)
};
// Traversals handed from k_bvh_bounce to k_bvh_tail_trav (see trav_run): per entry the queue slot
// and the saved node (trav_saved_node), the best hit so far (the final hit once k_bvh_tail_trav is
// done), and the stack (entry i of e at stack[i * cap + e]).  Segment s (at s * stride; counter
// FrameCtl::qcnt[b][s][1]) holds the rays of k_bvh_bounce's blocks of segment s, so
// k_bvh_tail_shade's survivors fit where theirs would have.
struct TailBuf {
    int2* node;     // queue slot | trav_saved_node
    float4* hit;    // trav_saved_hit
    int* stack;     // the LDS part of the stack (SceneDev::stack_lds entries; deeper ones stay spilled)
    int stride, cap, depth;
};
// queue entry k for path p and its primitive result
PT_DEV void queue_put(const QueueBuf& q, int k, const PathReg& p, float qt, int qw, f3 qs) {
    q.A[k] = make_float4(p.o.x, p.o.y, p.o.z, __int_as_float(p.pix));
    q.B[k] = make_float4(p.d.x, p.d.y, p.d.z, __int_as_float(p.rb));
    q.C[k] = make_float4(p.c.x, p.c.y, p.c.z, __int_as_float(p.slot | ((qw + 1) << 8)));
    q.D[k] = make_float4(qt, qs.x, qs.y, qs.z);
}

// Block-aggregated append of up to two flags: ballot -> per-wave counts -> one atomic per flag
// per block (counters on their own cache lines).  Returns each flagged lane's index.  Every
// thread of the block must call it.
// Slot of the gid-th entry of a segmented buffer: segment s holds entries [segoff[s], segoff[s+1])
// at s * stride.  Resolved once per wave on the scalar unit; per lane only if the wave straddles a
// segment boundary (at most NSEG-1 waves per launch).
PT_DEV int segment_slot(const int* segoff, int gid, int block_start, int stride) {
    const int w0 = block_start + (__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) << 6);
    int lo = 0, hi = segoff[1], sb = 0;
#pragma unroll
    for (int k = 1; k < NSEG; ++k)
        if (w0 >= segoff[k]) {
            lo = segoff[k];
            hi = segoff[k + 1];
            sb = k;
        }
    if (w0 + 63 < hi) return sb * stride - lo + gid;
    int sl = 0;
#pragma unroll
    for (int k = 1; k < NSEG; ++k) sl += (gid >= segoff[k]) ? 1 : 0;
    int sofs = 0;
#pragma unroll
    for (int k = 1; k < NSEG; ++k) sofs = (sl == k) ? segoff[k] : sofs;
    return sl * stride + (gid - sofs);
}

template <bool TWO>
PT_DEV void block_append(bool f0, int* ctr0, bool f1, int* ctr1, int& i0, int& i1) {
    __shared__ int s_w[2][BLOCK / 64];
    __shared__ int s_b[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t m0 = __ballot(f0);
    const uint64_t m1 = TWO ? __ballot(f1) : 0ull;
    if (lane == 0) {
        s_w[0][w] = __popcll(m0);
        if (TWO) s_w[1][w] = __popcll(m1);
    }
    __syncthreads();
    if (tid < (TWO ? 2 : 1)) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) {
            const int c = s_w[tid][i];
            s_w[tid][i] = tot;
            tot += c;
        }
        s_b[tid] = tot ? atomicAdd(tid == 0 ? ctr0 : ctr1, tot) : 0;
        PT_HOOK(ATOMIC_EXTRA, s_b[tid], tid == 0 ? ctr0 : ctr1);
    }
    __syncthreads();
    i0 = s_b[0] + s_w[0][w] + mbcnt(m0);
    i1 = TWO ? s_b[1] + s_w[1][w] + mbcnt(m1) : 0;
}

template <bool FIRST, bool HAS_BVH, int VAR>
__global__ __launch_bounds__(BLOCK) void k_bounce(SceneDev sc, PathBuf in, PathBuf out, FrameCtl* ctl,
                                                  float* __restrict__ image, int bounce, int seg_stride,
                                                  QueueBuf q) {
    // dynamic LDS: [geom table, sc.num_geoms <= LDS_GEOMS, candidate-queue variants]
    //              [HAS_BVH && !SPLIT: traversal stack, stack_depth x BLOCK ints]
    //              [VAR_WAVE_REDIST: one WaveLds per wave]
    extern __shared__ float4 s_dyn[];
    const int iter = ctl->iter;
    const bool to_plane = ctl->batch > 1 || ctl->plane != 0;   // gather into the frame planes
    int n;
    int segoff[NSEG + 1];
    if (FIRST) {
        n = ctl->cnt[0][0][0];          // local_pixels x batch
    } else {
        segoff[0] = 0;
#pragma unroll
        for (int s = 0; s < NSEG; ++s) segoff[s + 1] = segoff[s] + ctl->cnt[bounce][s][0];
        n = segoff[NSEG];
    }
    const int block_start = blockIdx.x * BLOCK;
    if (block_start >= n) return;
    constexpr bool TIMING = (VAR & VAR_SECTION_TIMING) != 0;
    constexpr bool QUEUE = (VAR & VAR_CAND_QUEUE) != 0;
    constexpr bool REDIST = (VAR & VAR_WAVE_REDIST) != 0;
    constexpr bool BVH_FAST = (VAR & VAR_BVH_FAST) != 0;
    // split: the launcher guarantees the pair layout and an LDS geom table (queue or redist)
    constexpr bool SPLIT = HAS_BVH && BVH_FAST && (VAR & VAR_BVH_SPLIT) && (QUEUE || REDIST);
    uint64_t tc = TIMING ? sec_clock() : 0;
    const int tid = threadIdx.x;
    const bool lds_geoms = (QUEUE || REDIST) && sc.num_geoms <= LDS_GEOMS;
    DevGeomHot* s_geoms = reinterpret_cast<DevGeomHot*>(s_dyn);
    int* s_stack = reinterpret_cast<int*>(s_dyn + (lds_geoms ? lds_geom_f4(sc) : 0));
    WaveLds* s_wave_isect =
        reinterpret_cast<WaveLds*>(s_stack + (HAS_BVH && !SPLIT ? sc.stack_depth * BLOCK : 0)) + (tid >> 6);
    const int gid = block_start + tid;
    bool active = gid < n;
    PathReg p;
    p.rb = 0;
    if (active) {
        if (FIRST) {
            const int slot = gid / sc.shard.local_pixels;
            p = camera_ray(sc.cam, iter + slot, sc.trace_depth, shard_pixel(sc, gid - slot * sc.shard.local_pixels));
            p.slot = slot;
        } else {
            p = load_path(in, segment_slot(segoff, gid, block_start, seg_stride));
        }
    }
    // the geom table after the path loads are issued (their latencies overlap); per-lane candidate
    // tests then read their geom from LDS, not L2
    if (lds_geoms) stage_geoms(sc, s_dyn);
    PT_HOOK(STAGE_EXTRA, lds_geoms, sc, s_dyn);
    if (TIMING && active) {
        __builtin_amdgcn_s_waitcnt(0);
        uint64_t t = sec_clock();
        sec_add(SEC_LOAD, t - tc);
        sec_add(SEC_N_WAVES, 1);
        sec_add_lanes(SEC_N_LANES, p.rb > 0 ? 1 : 0);
    }
    bool live = active && p.rb > 0;
    constexpr bool MG = (VAR & VAR_MAT_GROUP) != 0;
    Hit h;
    if (MG) h = Hit{-1.f, mk(0.f, 0.f, 0.f), 0, -1, 0.f, 0.f};
    bool queued = false;
    float qt = 0.f;
    int qw = -1;
    f3 qs = mk(0.f, 0.f, 0.f);
    if (REDIST && lds_geoms) {                     // wave-cooperative: every lane takes part
        if (VAR & VAR_BLOCK_REDIST)
            block_intersect<TIMING>(sc, s_geoms, live, p.o, p.d, reinterpret_cast<BlockLds*>(s_wave_isect - (tid >> 6)),
                                    qt, qw, qs);
        else
            wave_intersect<TIMING>(sc, s_geoms, live, p.o, p.d, s_wave_isect, qt, qw, qs);
    } else if (SPLIT && live) {
        prim_intersect_q<TIMING, FIRST && !TIMING>(sc, s_geoms, p.o, p.d, qt, qw, qs);
    }
    if (live) {
        if (SPLIT) {
            queued = bvh_root_needed(sc, p.o, p.d, qt);
            if (!queued) h = finish_hit<false>(sc, p.o, p.d, s_stack + tid, qt, qw, qs);
        } else if (REDIST && lds_geoms) {
            h = finish_hit<HAS_BVH, BVH_FAST>(sc, p.o, p.d, s_stack + tid, qt, qw, qs);
            PT_HOOK(DUP_HIT, HAS_BVH, BVH_FAST, sc, p.o, p.d, s_stack + tid, qt, qw, qs);
        } else {
            h = lds_geoms ? intersect_scene_q<HAS_BVH, TIMING, BVH_FAST, FIRST>(sc, s_geoms, p.o, p.d, s_stack + tid)
                          : intersect_scene<HAS_BVH, BVH_FAST>(sc, p.o, p.d, s_stack + tid);
        }
        if (!MG && !queued) {
            uint64_t ts = TIMING ? sec_clock() : 0;
            PT_HOOK(DUP_SHADE, (VAR & VAR_NO_TEX) == 0, sc, p, h, iter);
            shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
            if (TIMING) {
                tc = sec_clock();
                sec_add(SEC_SHADE, tc - ts);
            }
        }
    }
    if (MG) {   // MATERIAL_SORTING: regroup the block's paths by material, then shade
        if (SPLIT) {   // the rays queued for the mesh leave first, from their own threads
            int qi, unused;
            block_append<false>(queued, &ctl->qcnt[bounce][blockIdx.x & (NSEG - 1)][0], false, nullptr, qi, unused);
            qi += (blockIdx.x & (NSEG - 1)) * q.stride;
            if (queued) {
                queue_put(q, qi, p, qt, qw, qs);
                active = false;   // handed over to k_bvh_bounce
                live = false;
                queued = false;
            }
        }
        const int key = live ? (h.t > 0.0f ? h.mat : 0) : MG_KEYS - 1;
        MatGroupLds* mg = reinterpret_cast<MatGroupLds*>(s_wave_isect - (tid >> 6));
        group_by_material<HAS_BVH, false>(key, mg, active, live, queued, p, h, qt, qw, qs);
        if (live) shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
    }
    if (TIMING && active) tc = sec_clock();
    // later bounces: a path that came in with remainingBounces <= 0 was gathered when it terminated
    // (pathtrace.cu:535-537 skips it) -- it neither survives nor adds its colour again.  The camera
    // bounce gathers every path it made (trace depth 0: the untouched camera colour).
    const bool mine = FIRST ? active : live;
    const bool surv = mine && !queued && p.rb > 0;
    if (mine && !queued && !surv) gather_into_image(image, sc, to_plane, p);
    const int lane = tid & 63;
    const int seg = blockIdx.x & (NSEG - 1);
    if (VAR & VAR_WAVE_ATOMIC) {
        // one returning atomic per wave on a counter that owns its cache line; no barrier
        const uint64_t m = __ballot(surv);
        if (m != 0) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&ctl->cnt[bounce + 1][seg][0], __popcll(m));
            base = __shfl(base, 0);
            if (surv) store_path(out, seg * seg_stride + base + mbcnt(m), p);
        }
        if (!SPLIT) return;
        const uint64_t mq = __ballot(queued);
        if (mq != 0) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&ctl->qcnt[bounce][seg][0], __popcll(mq));
            base = __shfl(base, 0);
            if (queued) {
                const int k = seg * q.stride + base + mbcnt(mq);
                queue_put(q, k, p, qt, qw, qs);
            }
        }
        return;
    }
    // block-aggregated compaction (+ the traversal queue): one atomic per counter per block
    int si, qi;
    block_append<SPLIT>(surv, &ctl->cnt[bounce + 1][seg][0], queued, &ctl->qcnt[bounce][seg][0], si, qi);
    if (surv) store_path(out, seg * seg_stride + si, p);
    qi += seg * q.stride;
    if (SPLIT && queued) queue_put(q, qi, p, qt, qw, qs);
    if (TIMING && active) sec_add(SEC_STORE, sec_clock() - tc);
}

// Single-frame passes (the API's pathtrace(), F = 1): bounces `bounce` .. depth-1 of a
// primitive-only scene in ONE launch.  Each block keeps its paths in registers and loops over the
// remaining bounces (block-wide exact-test exchange, shading, gather at termination) until none of
// its paths is alive, with no compaction in between: the late bounces of a lone frame are a few
// thousand waves each, bound by launch and drain latency rather than by work.  Per-path
// arithmetic, RNG keys and the gather are those of k_bounce, so the image is the same bit for
// bit; per-bounce live counts go to the same counters (one atomic per block per bounce).
template <int VAR>
__global__ __launch_bounds__(BLOCK) void k_tail(SceneDev sc, PathBuf in, FrameCtl* ctl, float* __restrict__ image,
                                               int bounce, int seg_stride, int depth) {
    extern __shared__ float4 s_dyn[];
    __shared__ int s_cnt[BLOCK / 64];
    const int iter = ctl->iter;
    const bool to_plane = ctl->batch > 1 || ctl->plane != 0;   // gather into the frame planes
    int segoff[NSEG + 1];
    segoff[0] = 0;
#pragma unroll
    for (int s = 0; s < NSEG; ++s) segoff[s + 1] = segoff[s] + ctl->cnt[bounce][s][0];
    const int n = segoff[NSEG];
    const int block_start = blockIdx.x * BLOCK;
    if (block_start >= n) return;
    const int tid = threadIdx.x, lane = tid & 63;
    DevGeomHot* s_geoms = reinterpret_cast<DevGeomHot*>(s_dyn);
    BlockLds* s_block = reinterpret_cast<BlockLds*>(s_dyn + lds_geom_f4(sc));
    const int gid = block_start + tid;
    const bool active = gid < n;
    PathReg p;
    p.rb = 0;
    if (active) {
        int sl = 0;
#pragma unroll
        for (int k = 1; k < NSEG; ++k) sl += (gid >= segoff[k]) ? 1 : 0;
        int sofs = 0;
#pragma unroll
        for (int k = 1; k < NSEG; ++k) sofs = (sl == k) ? segoff[k] : sofs;
        p = load_path(in, sl * seg_stride + (gid - sofs));
    }
    stage_geoms(sc, s_dyn);   // after the path loads are issued
    const int seg = blockIdx.x & (NSEG - 1);
    for (int b = bounce; b < depth; ++b) {
        const bool live = active && p.rb > 0;
        float qt = 0.f;
        int qw = -1;
        f3 qs = mk(0.f, 0.f, 0.f);
        block_intersect<false>(sc, s_geoms, live, p.o, p.d, s_block, qt, qw, qs);
        if (live) {
            const Hit h = finish_hit<false>(sc, p.o, p.d, nullptr, qt, qw, qs);
            shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
            if (p.rb <= 0) gather_into_image(image, sc, to_plane, p);
        }
        // paths entering bounce b + 1 (k_bounce's survivor count for this bounce)
        const bool surv = live && p.rb > 0;
        const uint64_t m = __ballot(surv);
        if (lane == 0) s_cnt[tid >> 6] = __popcll(m);
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) tot += s_cnt[i];
        if (tid == 0 && tot) atomicAdd(&ctl->cnt[b + 1][seg][0], tot);
        __syncthreads();
        if (tot == 0) break;          // block-uniform
    }
}

// Bounces 0 and 1 of a primitive-only scene in ONE launch (PT_HEAD_FUSE, enqueue_pass_body): the
// camera bounce as k_bounce<true, false, 18> runs it (per-lane nearest-first queue), then, on the
// same registers, bounce 1 as k_bounce<false, false, 154> runs it (block-wide exact-test
// exchange), and only then the compaction, into the buffer bounce 1 writes.  82 % of the camera
// paths survive bounce 0: writing them out compacted and reading them straight back is the largest
// single piece of path traffic of the frame, and with it go a geom-table staging, a block_append
// and a launch.  Bounce 1 runs with the dead camera paths as idle lanes in the pre-test and the
// shading; the exact tests are dealt out over the block, so idle lanes cost nothing there.
// Per-path arithmetic, RNG keys and the gather are those of k_bounce, so the image is the same
// bit for bit; the survivors of bounce 0 are counted into cnt[1] as k_tail counts (one atomic per
// block), those of bounce 1 are appended to cnt[2] of the block's segment.  The exchange's region
// follows the geom table as in k_bounce; the camera queue needs none of its own, so the block's
// LDS is that of k_bounce<false, false, 154>.
template <int VAR>
__global__ __launch_bounds__(BLOCK) void k_head(SceneDev sc, PathBuf out, FrameCtl* ctl, float* __restrict__ image,
                                               int seg_stride) {
    extern __shared__ float4 s_dyn[];
    const int iter = ctl->iter;
    const bool to_plane = ctl->batch > 1 || ctl->plane != 0;   // gather into the frame planes
    const int n = ctl->cnt[0][0][0];                           // local_pixels x batch
    const int block_start = blockIdx.x * BLOCK;
    if (block_start >= n) return;
    const int tid = threadIdx.x, lane = tid & 63;
    DevGeomHot* s_geoms = reinterpret_cast<DevGeomHot*>(s_dyn);
    BlockLds* s_block = reinterpret_cast<BlockLds*>(s_dyn + lds_geom_f4(sc));
    // the per-wave survivor counts of bounce 0 borrow the exchange's result rows: block_intersect
    // first writes them after its own first barrier, which no wave passes before it has read these
    int* s_cnt = reinterpret_cast<int*>(s_block->rt);
    const int gid = block_start + tid;
    const bool active = gid < n;
    PathReg p;
    p.rb = 0;
    if (active) {
        const int slot = gid / sc.shard.local_pixels;
        p = camera_ray(sc.cam, iter + slot, sc.trace_depth, shard_pixel(sc, gid - slot * sc.shard.local_pixels));
        p.slot = slot;
    }
    stage_geoms(sc, s_dyn);
    const int seg = blockIdx.x & (NSEG - 1);
    // bounce 0
    if (active && p.rb > 0) {
        const Hit h = intersect_scene_q<false, false, true, true>(sc, s_geoms, p.o, p.d, nullptr);
        shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
    }
    bool live = active && p.rb > 0;
    if (active && !live) gather_into_image(image, sc, to_plane, p);
    {   // paths entering bounce 1 (k_bounce's survivor count for the camera bounce)
        const uint64_t m = __ballot(live);
        if (lane == 0) s_cnt[tid >> 6] = __popcll(m);
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) tot += s_cnt[i];
        if (tid == 0 && tot) atomicAdd(&ctl->cnt[1][seg][0], tot);
        if (tot == 0) return;         // block-uniform
    }
    // bounce 1
    float qt = 0.f;
    int qw = -1;
    f3 qs = mk(0.f, 0.f, 0.f);
    block_intersect<false>(sc, s_geoms, live, p.o, p.d, s_block, qt, qw, qs);
    if (live) {
        const Hit h = finish_hit<false>(sc, p.o, p.d, nullptr, qt, qw, qs);
        shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
        if (p.rb <= 0) gather_into_image(image, sc, to_plane, p);
    }
    const bool surv = live && p.rb > 0;
    int si, unused;
    block_append<false>(surv, &ctl->cnt[2][seg][0], false, nullptr, si, unused);
    if (surv) store_path(out, seg * seg_stride + si, p);
}

// VAR_BVH_SPLIT, second half of a bounce: the queued paths, 64 to a wave, traverse the mesh
// (bvh_intersect_pairs via finish_hit, entering with their primitive winner), are shaded, and
// gathered / compacted into the same output segments as k_bounce (blockIdx % NSEG; the host
// doubles seg_stride so both kernels' survivors fit).
// __launch_bounds__(256, 7): 7 waves per SIMD (<= 72 VGPRs; a few bytes of scratch in the cold
// exact-fallback paths).  Occupancy is what this latency-bound traversal lives on: with the SLP
// vectorizer on (packed-f32 pairs built from duplicated registers) it needed 96 VGPRs for 5
// waves; without it (Makefile) 79 VGPRs natural, and 72 at this bound (bunny 0.489 -> 0.477
// ms/frame); 8 waves (64 VGPRs) spill 100 B
#ifndef BVH_WAVES
#define BVH_WAVES 7
#endif

// after the traversal: the path's other words, the hit, shading (the shared end of k_bvh_bounce
// and k_bvh_tail_shade)
template <int VAR>
PT_DEV void bvh_finish_path(const SceneDev& sc, const QueueBuf& q, int qs, int iter, PathReg& p, const TravState& st) {
    float u = 0.f, v = 0.f;
    int tri = -1;
    const float tb = trav_result(st, u, v, tri);
    // the other words re-read here (L2): reading every word once, before the traversal,
    // keeps 5 more registers live across it -- bunny +6.7 %, khaslana +5.5 % (A/B, round 3)
    const float4 c = q.C[qs], d = q.D[qs];
    p.pix = __float_as_int(q.A[qs].w);
    p.rb = __float_as_int(q.B[qs].w);
    p.c = mk(c.x, c.y, c.z);
    const int cw = __float_as_int(c.w);
    p.slot = cw & 255;
    const int win = (cw >> 8) - 1;
    const Hit h = make_hit(sc, p.d, d.x, win, mk(d.y, d.z, d.w), tb, u, v, tri, sc.hot4);
    shade_path<(VAR & VAR_NO_TEX) == 0>(sc, p, h, iter + p.slot, [&]() { return hit_attr(sc, h); });
}
template <bool COUNT>
PT_DEV void bvh_count_ray(const TravState& st, float t_prim, int n_nodes) {
    if (COUNT) {
        sec_add_lanes(SEC_N_BVH_RAYS, 1);
        const bool hit = st.btri != 0x7fffffff && st.t_hit < t_prim;   // the mesh changes the winner
        sec_add_lanes(SEC_N_BVH_HITS, hit ? 1 : 0);
        sec_add_lanes(SEC_N_MISS_NODES, hit ? 0 : n_nodes);   // (a handed-over ray: its tail's nodes)
    }
}

// hand the calling lanes' traversals (st.cur >= 0) over to k_bvh_tail_trav: one atomic per wave.
// false: the segment is full at this lane's slot -- the caller finishes it itself.  The counter
// still counts it; every slot below min(counter, stride) is written by the lane that reserved it.
PT_DEV bool tail_put(const TailBuf& t, int* ctr, int seg, int qs, const TravState& st, const int* s_stack) {
    const uint64_t m = __ballot(1);
    const int lead = __builtin_ctzll(m);
    int base = 0;
    if ((int)(threadIdx.x & 63) == lead) base = atomicAdd(ctr, __popcll(m));
    const int slot = __builtin_amdgcn_readlane(base, lead) + mbcnt(m);
    if (slot >= t.stride) return false;
    const int e = seg * t.stride + slot;
    t.node[e] = make_int2(qs, trav_saved_node(st));
    t.hit[e] = trav_saved_hit(st);
    for (int i = 0; i < min(st.sp, t.depth); ++i) t.stack[(size_t)i * t.cap + e] = s_stack[i * BLOCK];
    // stats (pt_frame_stats handed_total / handed_stack_total): same-address atomics, one per
    // wave after the compiler's wave reduction, on the counter line the reservation just used
    atomicAdd(ctr + 2, 1);
    atomicAdd(ctr + 3, st.sp);
    return true;
}

template <int VAR, bool QUAD>
__global__ __launch_bounds__(BLOCK, BVH_WAVES) void k_bvh_bounce(SceneDev sc, QueueBuf q, TailBuf tail, int defer,
                                                                 PathBuf out, FrameCtl* ctl, float* __restrict__ image,
                                                                 int bounce, int seg_stride) {
    extern __shared__ float4 s_dyn[];   // traversal stack, stack_depth x BLOCK ints
    int segoff[NSEG + 1];
    segoff[0] = 0;
#pragma unroll
    for (int s = 0; s < NSEG; ++s) segoff[s + 1] = segoff[s] + ctl->qcnt[bounce][s][0];
    const int n = segoff[NSEG];
    const int block_start = blockIdx.x * BLOCK;
    if (block_start >= n) return;
    int* s_stack = reinterpret_cast<int*>(s_dyn);
    const int iter = ctl->iter;
    const bool to_plane = ctl->batch > 1 || ctl->plane != 0;   // gather into the frame planes
    const int tid = threadIdx.x;
    const int gid = block_start + tid;
    const int seg = blockIdx.x & (NSEG - 1);
    const bool active = gid < n;
    bool handed = false;
    const int qs = active ? segment_slot(segoff, gid, block_start, q.stride) : 0;
    PathReg p;
    p.rb = 0;
    if (active) {
        // traversal needs only the ray and its primitive t; the rest of the path is fetched
        // afterwards (fewer registers live across the traversal loop -> occupancy)
        const float4 a = q.A[qs], b = q.B[qs];
        const float t_prim = q.D[qs].x;
        p.o = mk(a.x, a.y, a.z);
        p.d = mk(b.x, b.y, b.z);
        constexpr bool CNT = (VAR & VAR_SECTION_TIMING) != 0;
        int n_nodes = 0, n_tris = 0;
        TravState st;
        trav_begin(sc, st, p.o, p.d, t_prim);
        st.qs = qs;   // deep stack entries spill to the slot's row (SceneDev::spill)
        if (CNT) sec_add_lanes(SEC_N_ROOT_CULLED, st.cur < 0 ? 1 : 0);
        // handed over: the wave's last few traversals go on 64 to a wave (no room: finish here)
        for (int d = defer;; d = 0) {
            trav_run<CNT, QUAD>(sc, st, s_stack + tid, d, n_nodes, n_tris);
            if (st.cur < 0) break;
            if (tail_put(tail, &ctl->qcnt[bounce][seg][1], seg, qs, st, s_stack + tid)) {
                handed = true;
                break;
            }
        }
        if (CNT) {
            sec_add_lanes(SEC_N_NODES, n_nodes);
            sec_add_lanes(SEC_N_TRIS, n_tris);
        }
        if (!handed) {
            bvh_count_ray<CNT>(st, t_prim, n_nodes);
            bvh_finish_path<VAR>(sc, q, qs, iter, p, st);
        }
    }
    const bool surv = active && !handed && p.rb > 0;
    if (active && !handed && !surv) gather_into_image(image, sc, to_plane, p);
    int si, unused;
    block_append<false>(surv, &ctl->cnt[bounce + 1][seg][0], false, nullptr, si, unused);
    if (surv) store_path(out, seg * seg_stride + si, p);
}

// The handed-over traversals, run by a fixed grid of waves that refill their lanes as rays
// finish: whenever `refill` or more of a wave's lanes are idle, it takes that many entries of its
// segment from the segment's counter of taken entries (FrameCtl::qcnt[b][s][2]; one atomic per
// refill), so a wave drains once, when its segment is done, instead of once per 64 rays.
// Traversal only: a finished ray's result (t, u, v, triangle) replaces its saved hit, and
// k_bvh_tail_shade shades the entries in full waves.  No barrier: waves leave on their own.
template <int VAR, bool QUAD>
__global__ __launch_bounds__(BLOCK, BVH_WAVES) void k_bvh_tail_trav(SceneDev sc, QueueBuf q, TailBuf t, FrameCtl* ctl,
                                                                    int bounce, int refill) {
    extern __shared__ float4 s_dyn[];
    int* s_stack = reinterpret_cast<int*>(s_dyn) + threadIdx.x;
    const int seg = blockIdx.x & (NSEG - 1);
    const int n = min(ctl->qcnt[bounce][seg][1], t.stride);
    if (n == 0) return;
    int next = 0;   // the segment's next untaken entry, as of this wave's last refill
    constexpr bool CNT = (VAR & VAR_SECTION_TIMING) != 0;
    int e = -1, qs = 0, n_nodes = 0, n_tris = 0, sp0 = 0;
    bool hit0 = false;
    TravState st;
    st.cur = -1;
    while (true) {
        const uint64_t idle = __ballot(e < 0);
        const int n_idle = __popcll(idle);
        if (next < n && (n_idle >= refill || n_idle == 64)) {
            const int lead = __builtin_ctzll(idle);
            int b0 = 0;
            if ((int)(threadIdx.x & 63) == lead) b0 = atomicAdd(&ctl->qcnt[bounce][seg][2], n_idle);
            next = __builtin_amdgcn_readlane(b0, lead);
            if (e < 0) {
                const int k = next + mbcnt(idle);
                if (k < n) {
                    e = seg * t.stride + k;
                    const int2 nd = t.node[e];
                    qs = nd.x;
                    const float4 a = q.A[qs], b = q.B[qs];
                    trav_resume(st, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), t.hit[e], nd.y, qs);
                    // the LDS part of its stack (spilled entries stay in the slot's row)
                    for (int i = 0; i < min(st.sp, sc.stack_lds); ++i) s_stack[i * BLOCK] = t.stack[(size_t)i * t.cap + e];
                    n_nodes = n_tris = 0;
                    if (CNT) {
                        sp0 = st.sp;
                        hit0 = st.btri != 0x7fffffff;
                    }
                }
            }
            next += n_idle;
        }
        const int lanes = __popcll(__ballot(e >= 0));
        if (lanes == 0) break;   // nothing left in the range
        if (e >= 0) {
            if (CNT) {
                sec_add(SEC_N_BVH_WITERS, 1);
                sec_add(SEC_TAIL_LANES_HIST + (lanes - 1) / 4, 1);
            }
            trav_step<CNT, QUAD>(sc, st, s_stack, n_nodes, n_tris);
            if (st.cur < 0) {
                t.hit[e] = trav_saved_hit(st);
                if (CNT) {
                    sec_add_lanes(SEC_N_NODES, n_nodes);
                    sec_add_lanes(SEC_N_TRIS, n_tris);
                    bvh_count_ray<CNT>(st, q.D[qs].x, n_nodes);
                    const int bk = sp0 < 4 ? sp0 : sp0 < 6 ? 4 : sp0 < 8 ? 5 : sp0 < 12 ? 6 : 7;
                    sec_add_lanes(SEC_TAIL_BY_SP + 2 * bk, 1);
                    sec_add_lanes(SEC_TAIL_BY_SP + 2 * bk + 1, n_nodes);
                    sec_add_lanes(SEC_TAIL_BY_HIT + (hit0 ? 2 : 0), 1);
                    sec_add_lanes(SEC_TAIL_BY_HIT + (hit0 ? 3 : 1), n_nodes);
                }
                e = -1;
            }
        }
    }
}
// ... and their shading, gather and compaction, as k_bvh_bounce's: block b takes the chunks
// j = b / NSEG, + gridDim / NSEG, .. of BLOCK entries of segment s = b % NSEG, survivors to output
// segment s (a grid for the usual counts, not for the capacity: empty blocks cost dispatch time)
template <int VAR>
__global__ __launch_bounds__(BLOCK) void k_bvh_tail_shade(SceneDev sc, QueueBuf q, TailBuf t, PathBuf out, FrameCtl* ctl,
                                                          float* __restrict__ image, int bounce, int seg_stride) {
    const int seg = blockIdx.x & (NSEG - 1);
    const int n = min(ctl->qcnt[bounce][seg][1], t.stride);
    const int iter = ctl->iter;
    const bool to_plane = ctl->batch > 1 || ctl->plane != 0;
    const int tid = threadIdx.x;
    for (int block_start = (blockIdx.x / NSEG) * BLOCK; block_start < n; block_start += (gridDim.x / NSEG) * BLOCK) {
        const bool active = block_start + tid < n;
        PathReg p;
        p.rb = 0;
        if (active) {
            const int e = seg * t.stride + block_start + tid;
            const int qs = t.node[e].x;
            const float4 a = q.A[qs], b = q.B[qs], h = t.hit[e];
            p.o = mk(a.x, a.y, a.z);
            p.d = mk(b.x, b.y, b.z);
            TravState st;
            st.t_hit = h.x;
            st.bu = h.y;
            st.bv = h.z;
            st.btri = __float_as_int(h.w);
            bvh_finish_path<VAR>(sc, q, qs, iter, p, st);
        }
        const bool surv = active && p.rb > 0;
        if (active && !surv) gather_into_image(image, sc, to_plane, p);
        int si, unused;
        block_append<false>(surv, &ctl->cnt[bounce + 1][seg][0], false, nullptr, si, unused);
        if (surv) store_path(out, seg * seg_stride + si, p);
    }
}
