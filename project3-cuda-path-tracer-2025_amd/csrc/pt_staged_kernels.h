// pt_staged_kernels.h — the staged pipeline, one kernel per reference stage, and two utilities.
//
//   k_camera, k_intersect, k_shade      the stages, over HitBuf
//   k_compact_count / _scan / _scatter  stable compaction
//   k_sort_hist / _scan / _scatter      stable counting sort by material
//   k_to_pbo, k_rng                     image -> 8-bit PBO; the RNG stream (pt_test_rng)
//
// Included by pt_runtime.hip alone, at global scope after its `using namespace ptd`, after
// pt_pass_kernels.h.
#pragma once

#include "pt_kernels.h"

// --------------------------------------------------------------------------------------------
// STAGED kernels (single contiguous segment)
// --------------------------------------------------------------------------------------------
struct HitBuf {
    float4* nt;     // surfaceNormal.xyz | t
    int* mat;       // materialId
    float4* uvd0;   // textured scenes only (else null): uv.xy | dpdu.xy
    float4* uvd1;   //                                    dpdu.z | dpdv.xyz
};

__global__ __launch_bounds__(BLOCK) void k_camera(SceneDev sc, PathBuf out, FrameCtl* ctl) {
    int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= ctl->cnt[0][0][0]) return;
    const int slot = gid / sc.shard.local_pixels;
    PathReg p = camera_ray(sc.cam, ctl->iter + slot, sc.trace_depth, shard_pixel(sc, gid - slot * sc.shard.local_pixels));
    p.slot = slot;
    store_path(out, gid, p);
}

template <bool HAS_BVH, bool BVH_FAST>
__global__ __launch_bounds__(BLOCK) void k_intersect(SceneDev sc, PathBuf in, HitBuf hits, const int* n_ptr) {
    extern __shared__ int s_stack[];
    const int n = *n_ptr;
    int gid = blockIdx.x * BLOCK + threadIdx.x;
    if (blockIdx.x * BLOCK >= n || gid >= n) return;
    float4 a = in.A[gid], b = in.B[gid];
    Hit h = intersect_scene<HAS_BVH, BVH_FAST>(sc, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), s_stack + threadIdx.x);
    hits.nt[gid] = make_float4(h.n.x, h.n.y, h.n.z, h.t);
    hits.mat[gid] = h.mat;
    if (hits.uvd0) {
        const HitAttr a = hit_attr(sc, h);
        hits.uvd0[gid] = make_float4(a.u, a.v, a.dpdu.x, a.dpdu.y);
        hits.uvd1[gid] = make_float4(a.dpdu.z, a.dpdv.x, a.dpdv.y, a.dpdv.z);
    }
}

// shade (optionally through a material-sorted permutation); terminated paths are gathered
// into the image unless image == nullptr; alive flags feed the compaction kernel.
__global__ __launch_bounds__(BLOCK) void k_shade(SceneDev sc, PathBuf buf, HitBuf hits, const int* perm,
                                                 const int* n_ptr, const FrameCtl* ctl, int iter_override,
                                                 float* image, int* alive) {
    const int n = *n_ptr;
    int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    int i = perm ? perm[j] : j;
    PathReg p = load_path(buf, i);
    if (p.rb <= 0) {                 // pathtrace.cu:535-537
        if (alive) alive[i] = 0;
        return;
    }
    float4 nt = hits.nt[i];
    Hit h;
    h.t = nt.w;
    h.n = mk(nt.x, nt.y, nt.z);
    h.mat = hits.mat[i];
    h.tri = -1;
    h.u = h.v = 0.f;
    const int iter = iter_override > 0 ? iter_override : ctl->iter;
    shade_path(sc, p, h, iter + p.slot, [&]() {
        HitAttr a;
        a.u = a.v = 0.0f;
        a.dpdu = a.dpdv = mk(0.f, 0.f, 0.f);
        if (hits.uvd0) {
            const float4 x = hits.uvd0[i], y = hits.uvd1[i];
            a.u = x.x;
            a.v = x.y;
            a.dpdu = mk(x.z, x.w, y.x);
            a.dpdv = mk(y.y, y.z, y.w);
        }
        return a;
    });
    store_path(buf, i, p);
    if (p.rb <= 0 && image)
        gather_into_image(image, sc, iter_override > 0 ? false : (ctl->batch > 1 || ctl->plane != 0), p);
    if (alive) alive[i] = p.rb > 0;
}

// ---- stable compaction (thrust::stable_partition(PathAlive), pathtrace.cu:750-757) ----
// Reduce-then-scan, three launches with no inter-workgroup waiting (dispatch order on MI355X is
// undefined by contract, and a single-word ticket / hop-by-hop look-back serialises at the
// device-scope atomic rate):
//   k_compact_count   per tile of CTILE items: popcount of ballot(alive) -> tile_cnt[t]
//   k_compact_scan    one workgroup: exclusive scan of tile_cnt -> tile_off, total -> n_out
//   k_compact_scatter per tile: flags + survivor payload loaded together, wave ballot/mbcnt
//                     ranks in item order, stores to tile_off[t] + rank (stable)
constexpr int CITEMS = 4;                       // items per thread (8 spills: measured slower)
constexpr int CTILE_MIN = BLOCK * CITEMS;       // 1024-item tiles (sizes the tile arrays)
constexpr int STILE = BLOCK * 8;                // material-sort tile (2048 items)
constexpr int SCAN_THREADS = 1024;

template <int CITEMS>
__global__ __launch_bounds__(BLOCK) void k_compact_count(const int* __restrict__ alive, const int* n_ptr,
                                                         int* __restrict__ tile_cnt) {
    constexpr int CTILE = BLOCK * CITEMS;
    __shared__ int s_w[BLOCK / 64];
    const int n = *n_ptr;
    const int base = blockIdx.x * CTILE;
    if (base >= n) return;
    const int tid = threadIdx.x;
    int av[CITEMS];
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) av[k] = alive[base + k * BLOCK + tid];   // capacity is tile-padded
    int c = 0;
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) c += __popcll(__ballot((base + k * BLOCK + tid < n) & (av[k] != 0)));
    if ((tid & 63) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) t += s_w[i];
        tile_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_compact_scan(const int* __restrict__ tile_cnt, const int* n_ptr,
                                                                int* __restrict__ tile_off, int* n_out, int CTILE) {
    __shared__ int s_part[SCAN_THREADS];
    const int n = *n_ptr;
    const int ntiles = (n + CTILE - 1) / CTILE;
    const int per = (ntiles + SCAN_THREADS - 1) / SCAN_THREADS;
    const int tid = threadIdx.x;
    const int lo = tid * per, hi = min(ntiles, lo + per);
    int sum = 0;
    for (int t = lo; t < hi; ++t) sum += tile_cnt[t];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {   // Hillis-Steele inclusive scan in LDS
        int v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = tid ? s_part[tid - 1] : 0;
    for (int t = lo; t < hi; ++t) {
        tile_off[t] = run;
        run += tile_cnt[t];
    }
    if (tid == SCAN_THREADS - 1) *n_out = s_part[SCAN_THREADS - 1];
}

// native 4-float vector: arrays of it stay in VGPRs (HIP's float4 is a union wrapper, and
// arrays of it were demoted to LDS/scratch, serialising each item's loads behind a wait)

template <int CITEMS>
__global__ __launch_bounds__(BLOCK) void k_compact_scatter(const float4* __restrict__ inA, const float4* __restrict__ inB,
                                                           const float4* __restrict__ inC, float4* __restrict__ outA,
                                                           float4* __restrict__ outB, float4* __restrict__ outC,
                                                           const int* __restrict__ alive, const int* n_ptr,
                                                           const int* __restrict__ tile_off) {
    constexpr int CTILE = BLOCK * CITEMS;
    __shared__ int s_cnt[CITEMS][BLOCK / 64];
    const int n = *n_ptr;
    const int base = blockIdx.x * CTILE;
    if (base >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const v4f* iA = reinterpret_cast<const v4f*>(inA);
    const v4f* iB = reinterpret_cast<const v4f*>(inB);
    const v4f* iC = reinterpret_cast<const v4f*>(inC);
    bool f[CITEMS];
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) f[k] = (base + k * BLOCK + tid < n) & (alive[base + k * BLOCK + tid] != 0);
    v4f a[CITEMS], b[CITEMS], c[CITEMS];
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) {
        const int idx = base + k * BLOCK + tid;
        if (f[k]) {
            a[k] = __builtin_nontemporal_load(iA + idx);
            b[k] = __builtin_nontemporal_load(iB + idx);
            c[k] = __builtin_nontemporal_load(iC + idx);
        }
    }
    uint64_t m[CITEMS];
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) {
        m[k] = __ballot(f[k]);
        if (lane == 0) s_cnt[k][w] = __popcll(m[k]);
    }
    __syncthreads();
    // exclusive offsets in item order (k-major, then wave): every thread recomputes its own
    int run = tile_off[blockIdx.x];
    int off[CITEMS];
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) {
        int mine = run;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) {
            const int cnt = s_cnt[k][i];
            mine = (i < w) ? mine + cnt : mine;
            run += cnt;
        }
        off[k] = mine;
    }
    v4f* oA = reinterpret_cast<v4f*>(outA);
    v4f* oB = reinterpret_cast<v4f*>(outB);
    v4f* oC = reinterpret_cast<v4f*>(outC);
#pragma unroll
    for (int k = 0; k < CITEMS; ++k) {
        if (f[k]) {
            const int dst = off[k] + mbcnt(m[k]);
            __builtin_nontemporal_store(a[k], oA + dst);
            __builtin_nontemporal_store(b[k], oB + dst);
            __builtin_nontemporal_store(c[k], oC + dst);
        }
    }
}

// ---- stable counting sort of materialId (MATERIAL_SORTING, pathtrace.cu:730-735) ----
// (at most MAXMAT keys, pt_records.h)

// per-tile key histogram, tile = STILE items
__global__ __launch_bounds__(BLOCK) void k_sort_hist(const int* __restrict__ keys, const int* n_ptr, int nkeys,
                                                     int* tile_hist) {
    __shared__ int h[MAXMAT];
    const int n = *n_ptr;
    const int tile = blockIdx.x, base = tile * STILE;
    for (int i = threadIdx.x; i < nkeys; i += BLOCK) h[i] = 0;
    __syncthreads();
    if (base < n) {
        for (int k = 0; k < STILE / BLOCK; ++k) {
            int idx = base + k * BLOCK + threadIdx.x;
            if (idx < n) atomicAdd(&h[keys[idx]], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nkeys; i += BLOCK) tile_hist[(size_t)tile * nkeys + i] = h[i];
}

// exclusive scan over (key, tile) in key-major order: one block of SCAN_THREADS, each thread a
// contiguous run of the flattened (key, tile) index space (tile_hist is stored [tile][key]),
// then a block scan of the run sums.  (The earlier one-thread-per-key loop over all tiles ran
// ~780 us at 10k tiles: 5-27 busy threads out of 256.)
__global__ __launch_bounds__(SCAN_THREADS) void k_sort_scan(int* tile_hist, const int* n_ptr, int nkeys) {
    __shared__ int s_part[SCAN_THREADS];
    const int n = *n_ptr;
    const int ntiles = (n + STILE - 1) / STILE;
    const int total = ntiles * nkeys;
    const int per = (total + SCAN_THREADS - 1) / SCAN_THREADS;
    const int tid = threadIdx.x;
    const int lo = min(total, tid * per), hi = min(total, lo + per);
    const int key0 = ntiles ? lo / ntiles : 0, t0 = lo - key0 * ntiles;
    int sum = 0;
    for (int f = lo, key = key0, t = t0; f < hi; ++f) {
        sum += tile_hist[(size_t)t * nkeys + key];
        if (++t == ntiles) { t = 0; ++key; }
    }
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {   // Hillis-Steele inclusive scan in LDS
        const int v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = tid ? s_part[tid - 1] : 0;
    for (int f = lo, key = key0, t = t0; f < hi; ++f) {
        const size_t at = (size_t)t * nkeys + key;
        const int c = tile_hist[at];
        tile_hist[at] = run;
        run += c;
        if (++t == ntiles) { t = 0; ++key; }
    }
}

// stable scatter: rank among equal keys = earlier items of the tile (item order k-major, wave,
// lane) — peers found with one ballot per key bit
__global__ __launch_bounds__(BLOCK) void k_sort_scatter(const int* __restrict__ keys, const int* n_ptr, int nkeys,
                                                        int key_bits, const int* tile_off, int* perm) {
    __shared__ int run[MAXMAT];           // items of each key already placed in this tile
    __shared__ int wcnt[BLOCK / 64][MAXMAT];
    const int n = *n_ptr;
    const int tile = blockIdx.x, base = tile * STILE;
    if (base >= n) return;
    const int tid = threadIdx.x, w = tid >> 6;
    for (int i = tid; i < nkeys; i += BLOCK) run[i] = 0;
    __syncthreads();
    for (int k = 0; k < STILE / BLOCK; ++k) {
        int idx = base + k * BLOCK + tid;
        bool valid = idx < n;
        int key = valid ? keys[idx] : 0;
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < key_bits; ++b) {
            uint64_t bb = __ballot(valid && ((key >> b) & 1));
            peers &= ((key >> b) & 1) ? bb : ~bb;
        }
        for (int i = tid; i < (BLOCK / 64) * MAXMAT; i += BLOCK) (&wcnt[0][0])[i] = 0;
        __syncthreads();
        // the lowest lane of each peer group publishes the group size for its wave
        if (valid && mbcnt(peers) == 0) wcnt[w][key] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int r = run[key] + mbcnt(peers);
            for (int ww = 0; ww < w; ++ww) r += wcnt[ww][key];
            perm[tile_off[(size_t)tile * nkeys + key] + r] = idx;
        }
        __syncthreads();
        for (int key2 = tid; key2 < nkeys; key2 += BLOCK) {
            int s = 0;
            for (int ww = 0; ww < BLOCK / 64; ++ww) s += wcnt[ww][key2];
            run[key2] += s;
        }
        __syncthreads();
    }
}

// sendImageToPBO (pathtrace.cu:59-80)
__global__ void k_to_pbo(const float* __restrict__ image, pt_uchar4* pbo, int n, int iter) {
    int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double d = (double)(image[3 * (size_t)i + k] / (float)iter) * 255.0;
        int v = (d != d) ? 0 : (d >= 2147483647.0 ? 2147483647 : (d <= -2147483648.0 ? (-2147483647 - 1) : (int)d));
        c[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    pt_uchar4 o;
    o.x = (uint8_t)c[0];
    o.y = (uint8_t)c[1];
    o.z = (uint8_t)c[2];
    o.w = 0;
    pbo[i] = o;
}

__global__ void k_rng(const int* iid, int m, int n, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Rng r = rng_make(iid[3 * i], iid[3 * i + 1], iid[3 * i + 2]);
    for (int k = 0; k < n; ++k) out[(size_t)i * n + k] = u01(r);
}
