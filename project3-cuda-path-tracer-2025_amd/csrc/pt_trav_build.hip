// pt_trav_build.hip — pth::build_sah_tree (host/trav_tree.cpp) on the GPU, the SAME tree bit for bit
// (pt/pt_trav_build.h has the argument and the one known divergence).
//
// The host recursion, per segment [begin, end) of the leaf index array:
//   centroid bounds cl / ch in double; per axis with extent, 32 bins of (count, float box); the
//   93 (axis, split) candidates' costs l.area()*lc + r.area()*rc; the first strict minimum; the
//   stable partition by bin <= bsplit (index-order halving if no axis has extent); the median split
//   on the same axis by (centroid, leaf id) where a child would have no room below max_height.
// Nodes are created in preorder, which has a closed form top-down: the left child of node p is
// p + 1, the right child p + (leaves of the left child).  So every segment knows its node's final
// preorder id when it is created, and the device only has to write each node's two child codes.
//
// GPU formulation:
//   * segments of more than SUBT leaves, level by level, all of a level at once; a segment is cut into
//     pieces of PIECE leaves, one workgroup per piece, so the top levels fill the chip:
//       k_piece_cbounds / k_seg_cbounds   centroid bounds (wave shuffles + LDS, pieces joined per segment)
//       k_piece_bins                      3 x 32 bins in LDS, LDS atomics on the ordered-integer floats
//       k_seg_split                       one wave per segment: joins the pieces' bins, deals the 93
//                                         candidates over the lanes, one wave-wide argmin (wave_split)
//       k_piece_hist / k_seg_pick         median split: radix select, 12 digits of 8 bits over the
//                                         ordered 64-bit centroid bits, then the leaf id
//       k_piece_count / k_seg_scan / k_piece_scatter / k_piece_copy   the stable partition
//   * every segment of at most SUBT leaves is finished with its whole subtree by k_subtree, one wave
//     per segment, boxes and index order LDS-resident, in a single launch after the levels.  It uses
//     the same wave_split and the same predicate (goes_left) as the level kernels.
// Min / max and integer counts are order-free and exact, so none of this depends on how the work is
// split.  Boxes, cull sizes, height and the final numbering are the host's own pth::finish_sah_tree.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt/pt_trav_build.h"
#include "trav_tree.h"

namespace {

constexpr int BT = 256;                          // threads per workgroup of the piece kernels
constexpr int WAVE = 64;
constexpr int PIECE = PT_TRAV_BUILD_PIECE;
constexpr int SUBT = PT_TRAV_BUILD_SUBTREE;
constexpr int BINS = 32;
constexpr int NB = 3 * BINS;                     // bins of one segment: axis-major
constexpr int NCAND = 3 * (BINS - 1);            // (axis, split after bin b) candidates
constexpr int BINW = 7;                          // words per bin: count, lo.xyz, hi.xyz (ordered-integer floats)
constexpr int DIGITS = 12;                       // radix select: 8 digits of the key, 4 of the leaf id

struct Seg {
    int begin, end;
    int node;      // preorder id of the segment's inner node
    int depth;     // the host's Work::depth (root: 1)
};
struct Piece {
    int seg;
    int start, end;
};
struct Decision {
    int mode;      // 0: partition by bin <= bsplit; 1: halve in index order; 2: median split
    int axis, bsplit, nleft;
    double cl, ext;              // of `axis` (mode 0)
    unsigned long long pkey;     // mode 2: the pivot, element of rank nleft by (key, leaf id) ...
    unsigned pid;
    int rank;                    // ... and what is left of that rank while the select runs
};

// floats as unsigned integers of the same order (-0 sorts below +0; both give the same areas)
__device__ __forceinline__ unsigned f_ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_f(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// the median split's key: the centroid's order (cx < cy), with -0 == +0 as the host compares them
__device__ __forceinline__ unsigned long long d_ord(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double centroid(float lo, float hi) { return 0.5 * ((double)lo + (double)hi); }
__device__ __forceinline__ int bin_of(double cen, double cl, double ext) {
    return min(BINS - 1, (int)((cen - cl) / ext * BINS));
}
__device__ __forceinline__ int ceil_log2(int c) {
    int h = 0;
    while ((1 << h) < c) ++h;
    return h;
}

// does leaf k, at position `at` of its segment, go to the left child?
__device__ __forceinline__ bool goes_left(const Decision& d, float lo, float hi, int k, int at) {
    if (d.mode == 1) return at < d.nleft;
    const double c = centroid(lo, hi);
    if (d.mode == 0) return bin_of(c, d.cl, d.ext) <= d.bsplit;
    const unsigned long long key = d_ord(c);
    return key < d.pkey || (key == d.pkey && (unsigned)k < d.pid);
}

__device__ __forceinline__ double wave_min(double v) {
    for (int m = 1; m < WAVE; m <<= 1) {
        const double o = __shfl_xor(v, m, WAVE);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int m = 1; m < WAVE; m <<= 1) {
        const double o = __shfl_xor(v, m, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// The split of one segment from its joined bins (bins[w * NB + axis * BINS + b], in LDS), by one
// wave: lane c and lane c + 64 take candidates c = axis * 31 + split; each unions the bins on either
// side, and the wave keeps the smallest (cost, candidate) -- the host's first strict minimum, since it
// walks the candidates in that order.  Then the host's mid / height rule.  Every lane returns the same.
__device__ Decision wave_split(const unsigned* bins, int lane, int len, int depth, int max_height, const double* cl,
                               const double* ch) {
    double best = HUGE_VAL;
    int bidx = 1 << 30;
    for (int c = lane; c < NCAND; c += WAVE) {
        const int a = c / (BINS - 1), s = c % (BINS - 1);
        const unsigned* col = bins + a * BINS;
        // count and area of the union of bins [b0, b1) (an empty bin is the identity of min / max)
        auto side = [&](int b0, int b1, int& count) {
            unsigned lx = ~0u, ly = ~0u, lz = ~0u, hx = 0u, hy = 0u, hz = 0u;
            count = 0;
            for (int b = b0; b < b1; ++b) {
                count += (int)col[b];
                lx = min(lx, col[1 * NB + b]);
                ly = min(ly, col[2 * NB + b]);
                lz = min(lz, col[3 * NB + b]);
                hx = max(hx, col[4 * NB + b]);
                hy = max(hy, col[5 * NB + b]);
                hz = max(hz, col[6 * NB + b]);
            }
            if (count == 0) return 0.0;
            const double x = (double)ord_f(hx) - (double)ord_f(lx);
            const double y = (double)ord_f(hy) - (double)ord_f(ly);
            const double z = (double)ord_f(hz) - (double)ord_f(lz);
            return x * y + y * z + z * x;
        };
        int lc, rc;
        const double larea = side(0, s + 1, lc), rarea = side(s + 1, BINS, rc);
        if (lc == 0 || rc == 0) continue;
        const double cost = larea * lc + rarea * rc;
        if (cost < best) {   // a lane's candidates rise, so strict < keeps its first minimum; inf never wins
            best = cost;
            bidx = c;
        }
    }
    for (int m = 1; m < WAVE; m <<= 1) {
        const double oc = __shfl_xor(best, m, WAVE);
        const int oi = __shfl_xor(bidx, m, WAVE);
        if (oc < best || (oc == best && oi < bidx)) {
            best = oc;
            bidx = oi;
        }
    }
    Decision d;
    d.pkey = 0;
    d.pid = 0;
    d.rank = 0;
    const int half = len / 2;
    if (bidx >= NCAND) {   // every centroid equal: halve in index order
        d.mode = 1;
        d.axis = 0;
        d.bsplit = -1;
        d.nleft = half;
        d.cl = 0.0;
        d.ext = 0.0;
    } else {
        d.mode = 0;
        d.axis = bidx / (BINS - 1);
        d.bsplit = bidx % (BINS - 1);
        int lc = 0;
        for (int b = 0; b <= d.bsplit; ++b) lc += (int)bins[d.axis * BINS + b];
        d.nleft = lc;   // 0 < lc < len: both sides of a candidate hold a leaf
        d.cl = cl[d.axis];
        d.ext = ch[d.axis] - cl[d.axis];
    }
    if (depth + 1 + ceil_log2(max(d.nleft, len - d.nleft)) > max_height) {
        d.mode = 2;
        d.nleft = half;
        d.rank = half;
    }
    return d;
}

// ---- level kernels ----

// centroid bounds of one piece: 6 doubles (min.xyz, max.xyz)
__global__ __launch_bounds__(BT) void k_piece_cbounds(const float* __restrict__ lo, const float* __restrict__ hi,
                                                      const int* __restrict__ idx, const Piece* __restrict__ pieces,
                                                      double* __restrict__ pb) {
    __shared__ double red[BT / WAVE][6];
    const Piece pc = pieces[blockIdx.x];
    double v[6] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int p = pc.start + (int)threadIdx.x; p < pc.end; p += BT) {
        const size_t k = 3 * (size_t)idx[p];
        for (int a = 0; a < 3; ++a) {
            const double c = centroid(lo[k + a], hi[k + a]);
            v[a] = c < v[a] ? c : v[a];
            v[3 + a] = c > v[3 + a] ? c : v[3 + a];
        }
    }
    for (int a = 0; a < 3; ++a) {
        v[a] = wave_min(v[a]);
        v[3 + a] = wave_max(v[3 + a]);
    }
    const int w = threadIdx.x / WAVE;
    if (threadIdx.x % WAVE == 0)
        for (int a = 0; a < 6; ++a) red[w][a] = v[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        double r = red[0][threadIdx.x];
        for (int q = 1; q < BT / WAVE; ++q) {
            const double o = red[q][threadIdx.x];
            r = threadIdx.x < 3 ? (o < r ? o : r) : (o > r ? o : r);
        }
        pb[6 * (size_t)blockIdx.x + threadIdx.x] = r;
    }
}

// the pieces of each segment joined: sb[6 seg ..]
__global__ void k_seg_cbounds(const int* __restrict__ first, const double* __restrict__ pb, double* __restrict__ sb,
                              int nseg) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = t / 8, a = t % 8;
    if (s >= nseg || a >= 6) return;
    double r = a < 3 ? HUGE_VAL : -HUGE_VAL;
    for (int p = first[s]; p < first[s + 1]; ++p) {
        const double o = pb[6 * (size_t)p + a];
        r = a < 3 ? (o < r ? o : r) : (o > r ? o : r);
    }
    sb[6 * (size_t)s + a] = r;
}

__device__ __forceinline__ void bins_clear(unsigned* bins, int tid, int nthreads) {
    for (int i = tid; i < BINW * NB; i += nthreads) bins[i] = i < NB ? 0u : i < 4 * NB ? 0xffffffffu : 0u;
}
// one leaf into the LDS bins of every axis that has extent
__device__ __forceinline__ void bins_add(unsigned* bins, const double* cl, const double* ch, const float* l,
                                         const float* h) {
    for (int a = 0; a < 3; ++a) {
        const double ext = ch[a] - cl[a];
        if (!(ext > 0.0)) continue;
        const int e = a * BINS + bin_of(centroid(l[a], h[a]), cl[a], ext);
        atomicAdd(&bins[e], 1u);
        for (int k = 0; k < 3; ++k) {
            atomicMin(&bins[(1 + k) * NB + e], f_ord(l[k]));
            atomicMax(&bins[(4 + k) * NB + e], f_ord(h[k]));
        }
    }
}

// the bins of one piece, built in LDS, written as BINW * NB words
__global__ __launch_bounds__(BT) void k_piece_bins(const float* __restrict__ lo, const float* __restrict__ hi,
                                                   const int* __restrict__ idx, const Piece* __restrict__ pieces,
                                                   const double* __restrict__ sb, unsigned* __restrict__ pbins) {
    __shared__ unsigned bins[BINW * NB];
    const Piece pc = pieces[blockIdx.x];
    double cl[3], ch[3];
    for (int a = 0; a < 3; ++a) {
        cl[a] = sb[6 * (size_t)pc.seg + a];
        ch[a] = sb[6 * (size_t)pc.seg + 3 + a];
    }
    bins_clear(bins, threadIdx.x, BT);
    __syncthreads();
    for (int p = pc.start + (int)threadIdx.x; p < pc.end; p += BT) {
        const size_t k = 3 * (size_t)idx[p];
        const float l[3] = {lo[k], lo[k + 1], lo[k + 2]}, h[3] = {hi[k], hi[k + 1], hi[k + 2]};
        bins_add(bins, cl, ch, l, h);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINW * NB; i += BT) pbins[(size_t)blockIdx.x * BINW * NB + i] = bins[i];
}

// one wave per segment: its pieces' bins joined in LDS, then the split
__global__ __launch_bounds__(WAVE) void k_seg_split(const Seg* __restrict__ segs, const int* __restrict__ first,
                                                    const unsigned* __restrict__ pbins, const double* __restrict__ sb,
                                                    int max_height, Decision* __restrict__ dec) {
    __shared__ unsigned bins[BINW * NB];
    const int s = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < BINW * NB; i += WAVE) {
        unsigned r = i < NB ? 0u : i < 4 * NB ? 0xffffffffu : 0u;
        for (int p = first[s]; p < first[s + 1]; ++p) {
            const unsigned o = pbins[(size_t)p * BINW * NB + i];
            r = i < NB ? r + o : i < 4 * NB ? min(r, o) : max(r, o);
        }
        bins[i] = r;
    }
    __syncthreads();
    double cl[3], ch[3];
    for (int a = 0; a < 3; ++a) {
        cl[a] = sb[6 * (size_t)s + a];
        ch[a] = sb[6 * (size_t)s + 3 + a];
    }
    const Seg sg = segs[s];
    const Decision d = wave_split(bins, lane, sg.end - sg.begin, sg.depth, max_height, cl, ch);
    if (lane == 0) dec[s] = d;
}

// the digit of (key, leaf id) the select looks at in pass `pass`, or -1 if the element no longer
// shares the pivot's prefix
__device__ __forceinline__ int select_digit(const Decision& d, unsigned long long key, unsigned id, int pass) {
    if (pass < 8) {
        const int sh = 56 - 8 * pass;   // the digit's shift; the prefix is everything above it
        if (pass > 0 && (key >> (sh + 8)) != (d.pkey >> (sh + 8))) return -1;
        return (int)((key >> sh) & 255u);
    }
    if (key != d.pkey) return -1;
    const int sh = 24 - 8 * (pass - 8);
    if (pass > 8 && (id >> (sh + 8)) != (d.pid >> (sh + 8))) return -1;
    return (int)((id >> sh) & 255u);
}

// median split, one digit: the histogram of the digit over the elements that still match, per piece
// in LDS, then added to its segment's (integer adds: order-free)
__global__ __launch_bounds__(BT) void k_piece_hist(const float* __restrict__ lo, const float* __restrict__ hi,
                                                   const int* __restrict__ idx, const Piece* __restrict__ pieces,
                                                   const Decision* __restrict__ dec, int pass, unsigned* __restrict__ hist) {
    __shared__ unsigned h[256];
    const Piece pc = pieces[blockIdx.x];
    const Decision d = dec[pc.seg];
    if (d.mode != 2) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int p = pc.start + (int)threadIdx.x; p < pc.end; p += BT) {
        const int k = idx[p];
        const size_t e = 3 * (size_t)k + d.axis;
        const int g = select_digit(d, d_ord(centroid(lo[e], hi[e])), (unsigned)k, pass);
        if (g >= 0) atomicAdd(&h[g], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[256 * (size_t)pc.seg + threadIdx.x], h[threadIdx.x]);
}
// the digit that holds the wanted rank becomes part of the pivot; the histogram is cleared for the next pass
__global__ __launch_bounds__(256) void k_seg_pick(Decision* __restrict__ dec, int pass, unsigned* __restrict__ hist) {
    __shared__ unsigned h[256];
    const int s = blockIdx.x;
    if (dec[s].mode != 2) return;
    h[threadIdx.x] = hist[256 * (size_t)s + threadIdx.x];
    hist[256 * (size_t)s + threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        Decision d = dec[s];
        int g = 0;
        while (g < 255 && d.rank >= (int)h[g]) {
            d.rank -= (int)h[g];
            ++g;
        }
        if (pass < 8) d.pkey |= (unsigned long long)g << (56 - 8 * pass);
        else d.pid |= (unsigned)g << (24 - 8 * (pass - 8));
        dec[s] = d;
    }
}

// the stable partition, step 1: left-going elements per piece
__global__ __launch_bounds__(BT) void k_piece_count(const float* __restrict__ lo, const float* __restrict__ hi,
                                                    const int* __restrict__ idx, const Piece* __restrict__ pieces,
                                                    const Seg* __restrict__ segs, const Decision* __restrict__ dec,
                                                    int* __restrict__ cnt) {
    __shared__ int red[BT];
    const Piece pc = pieces[blockIdx.x];
    const Decision d = dec[pc.seg];
    const int begin = segs[pc.seg].begin;
    int c = 0;
    for (int p = pc.start + (int)threadIdx.x; p < pc.end; p += BT) {
        const int k = idx[p];
        const size_t e = 3 * (size_t)k + d.axis;
        c += goes_left(d, lo[e], hi[e], k, p - begin) ? 1 : 0;
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = BT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[blockIdx.x] = red[0];
}
// step 2: per segment, the exclusive scan of its pieces' counts (pieces of a segment are consecutive)
__global__ void k_seg_scan(const int* __restrict__ first, int* __restrict__ cnt_to_off, int nseg) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    int run = 0;
    for (int p = first[s]; p < first[s + 1]; ++p) {
        const int c = cnt_to_off[p];
        cnt_to_off[p] = run;
        run += c;
    }
}
// step 3: threads take contiguous chunks of the piece, so ranks follow the index order: the k-th left
// element of the segment lands at begin + k, the k-th right one at begin + nleft + k
__global__ __launch_bounds__(BT) void k_piece_scatter(const float* __restrict__ lo, const float* __restrict__ hi,
                                                      const int* __restrict__ idx_in, int* __restrict__ idx_out,
                                                      const Piece* __restrict__ pieces, const Seg* __restrict__ segs,
                                                      const Decision* __restrict__ dec, const int* __restrict__ off) {
    __shared__ int scan[BT];
    const Piece pc = pieces[blockIdx.x];
    const Decision d = dec[pc.seg];
    const Seg sg = segs[pc.seg];
    const int chunk = (pc.end - pc.start + BT - 1) / BT;
    const int a = min(pc.end, pc.start + (int)threadIdx.x * chunk), b = min(pc.end, a + chunk);
    int c = 0;
    for (int p = a; p < b; ++p) {
        const int k = idx_in[p];
        const size_t e = 3 * (size_t)k + d.axis;
        c += goes_left(d, lo[e], hi[e], k, p - sg.begin) ? 1 : 0;
    }
    scan[threadIdx.x] = c;
    __syncthreads();
    for (int s = 1; s < BT; s <<= 1) {   // inclusive Hillis-Steele scan
        const int x = (int)threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
        __syncthreads();
        scan[threadIdx.x] += x;
        __syncthreads();
    }
    int lefts = off[blockIdx.x] + scan[threadIdx.x] - c;   // left elements of the segment before position a
    for (int p = a; p < b; ++p) {
        const int k = idx_in[p];
        const size_t e = 3 * (size_t)k + d.axis;
        const int dst = goes_left(d, lo[e], hi[e], k, p - sg.begin) ? sg.begin + lefts++
                                                                    : sg.begin + d.nleft + (p - sg.begin) - lefts;
        if (dst < sg.end) idx_out[dst] = k;   // always: the decision's nleft is this predicate's count
    }
}
// step 4: back into the index array (the segments that are not split this level never left it)
__global__ __launch_bounds__(BT) void k_piece_copy(const int* __restrict__ from, int* __restrict__ to,
                                                   const Piece* __restrict__ pieces) {
    const Piece pc = pieces[blockIdx.x];
    for (int p = pc.start + (int)threadIdx.x; p < pc.end; p += BT) to[p] = from[p];
}

// ---- subtrees: a segment of at most SUBT leaves, with everything below it, by one wave in LDS ----
struct SubLds {
    float lo[3][SUBT], hi[3][SUBT];      // per local element
    int id[SUBT];                        // local element -> leaf id
    unsigned short pos[SUBT], tmp[SUBT]; // position (relative to the subtree's begin) -> local element
    int stk_node[SUBT];                  // right children waiting: node id, range, depth
    int stk_d[SUBT];
    unsigned short stk_s[SUBT], stk_t[SUBT];
    unsigned bins[BINW * NB];
    Decision dec;
};

__global__ __launch_bounds__(WAVE) void k_subtree(const float* __restrict__ lo, const float* __restrict__ hi,
                                                  const int* __restrict__ idx, const Seg* __restrict__ roots,
                                                  int max_height, int* __restrict__ kids) {
    __shared__ SubLds L;
    const Seg r = roots[blockIdx.x];
    const int m = r.end - r.begin, lane = threadIdx.x;
    for (int e = lane; e < m; e += WAVE) {
        const int k = idx[r.begin + e];
        for (int a = 0; a < 3; ++a) {
            L.lo[a][e] = lo[3 * (size_t)k + a];
            L.hi[a][e] = hi[3 * (size_t)k + a];
        }
        L.id[e] = k;
        L.pos[e] = (unsigned short)e;
    }
    __syncthreads();
    int sp = 0, s = 0, t = m, node = r.node, depth = r.depth;
    while (true) {   // the nodes depth-first, left first; s, t, node, depth are the same in every lane
        const int len = t - s;
        // centroid bounds
        double cl[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, ch[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (int p = s + lane; p < t; p += WAVE) {
            const int e = L.pos[p];
            for (int a = 0; a < 3; ++a) {
                const double c = centroid(L.lo[a][e], L.hi[a][e]);
                cl[a] = c < cl[a] ? c : cl[a];
                ch[a] = c > ch[a] ? c : ch[a];
            }
        }
        for (int a = 0; a < 3; ++a) {
            cl[a] = wave_min(cl[a]);
            ch[a] = wave_max(ch[a]);
        }
        // bins and split
        bins_clear(L.bins, lane, WAVE);
        __syncthreads();
        for (int p = s + lane; p < t; p += WAVE) {
            const int e = L.pos[p];
            const float l[3] = {L.lo[0][e], L.lo[1][e], L.lo[2][e]}, h[3] = {L.hi[0][e], L.hi[1][e], L.hi[2][e]};
            bins_add(L.bins, cl, ch, l, h);
        }
        __syncthreads();
        Decision d = wave_split(L.bins, lane, len, depth, max_height, cl, ch);
        if (d.mode == 2) {
            // the pivot is the element that exactly nleft others precede by (key, leaf id): each lane
            // counts for its elements (a segment this small needs no radix passes)
            for (int p = s + lane; p < t; p += WAVE) {
                const int e = L.pos[p];
                const unsigned long long key = d_ord(centroid(L.lo[d.axis][e], L.hi[d.axis][e]));
                const unsigned id = (unsigned)L.id[e];
                int before = 0;
                for (int q = s; q < t; ++q) {
                    const int f = L.pos[q];
                    const unsigned long long kq = d_ord(centroid(L.lo[d.axis][f], L.hi[d.axis][f]));
                    before += (kq < key || (kq == key && (unsigned)L.id[f] < id)) ? 1 : 0;
                }
                if (before == d.nleft) {
                    d.pkey = key;
                    d.pid = id;
                    L.dec = d;
                }
            }
            __syncthreads();
            d = L.dec;
            __syncthreads();
        }
        // stable partition: lanes take contiguous chunks, ranks by a scan over the lanes
        {
            const int chunk = (len + WAVE - 1) / WAVE;
            const int a = min(t, s + lane * chunk), b = min(t, a + chunk);
            int c = 0;
            for (int p = a; p < b; ++p) {
                const int e = L.pos[p];
                c += goes_left(d, L.lo[d.axis][e], L.hi[d.axis][e], L.id[e], p - s) ? 1 : 0;
            }
            int incl = c;
            for (int k = 1; k < WAVE; k <<= 1) {
                const int y = __shfl_up(incl, k, WAVE);
                if (lane >= k) incl += y;
            }
            int lefts = incl - c;
            for (int p = a; p < b; ++p) {
                const int e = L.pos[p];
                const int dst = goes_left(d, L.lo[d.axis][e], L.hi[d.axis][e], L.id[e], p - s) ? s + lefts++
                                                                                                : s + d.nleft + (p - s) - lefts;
                if (dst < t) L.tmp[dst] = (unsigned short)e;
            }
            __syncthreads();
            for (int p = s + lane; p < t; p += WAVE) L.pos[p] = L.tmp[p];
            __syncthreads();
        }
        // children: a single leaf is a code in the parent, a larger left child is next, a larger
        // right child waits on the stack
        const int mid = s + d.nleft;
        const bool lleaf = d.nleft == 1, rleaf = t - mid == 1;
        if (lane == 0) {
            kids[2 * (size_t)node] = lleaf ? -(L.id[L.pos[s]] + 1) : node + 1;
            kids[2 * (size_t)node + 1] = rleaf ? -(L.id[L.pos[mid]] + 1) : node + d.nleft;
            if (!rleaf) {
                L.stk_node[sp] = node + d.nleft;
                L.stk_s[sp] = (unsigned short)mid;
                L.stk_t[sp] = (unsigned short)t;
                L.stk_d[sp] = depth + 1;
            }
        }
        if (!rleaf) ++sp;
        __syncthreads();
        if (!lleaf) {
            t = mid;
            node = node + 1;
            depth = depth + 1;
            continue;
        }
        if (sp == 0) break;
        --sp;
        node = L.stk_node[sp];
        s = L.stk_s[sp];
        t = L.stk_t[sp];
        depth = L.stk_d[sp];
        __syncthreads();
    }
}

std::string g_err;

int host_ceil_log2(int c) {
    int h = 0;
    while ((1 << h) < c) ++h;
    return h;
}

// the tree's shape on the current device: kids[2 (n - 1)] as finish_sah_tree reads them.  The input
// is valid (n >= 2, finite, ordered).  PT_OK, or PT_E_HIP with g_err set.
int32_t device_shape(const float* leaf_lo, const float* leaf_hi, int n, int max_height, std::vector<int>& kids) {
    int32_t rc = PT_OK;
    float *d_lo = nullptr, *d_hi = nullptr;
    int *d_idx = nullptr, *d_idx2 = nullptr, *d_kids = nullptr, *d_lvl = nullptr, *d_cnt = nullptr;
    double *d_pb = nullptr, *d_sb = nullptr;
    unsigned *d_pbins = nullptr, *d_hist = nullptr;
    Decision* d_dec = nullptr;
    Seg* d_roots = nullptr;
    size_t lvl_cap = 0, piece_cap = 0, seg_cap = 0;
#define TCHK(x)                                                      \
    do {                                                             \
        hipError_t e_ = (x);                                         \
        if (e_ != hipSuccess) {                                      \
            g_err = std::string(#x) + ": " + hipGetErrorString(e_);  \
            rc = PT_E_HIP;                                           \
            goto done;                                               \
        }                                                            \
    } while (0)
    std::vector<Seg> level, next, roots;
    struct Fix {
        size_t slot;
        int at;
    };
    std::vector<Fix> fixes;   // leaf children of level nodes: the leaf id is idx[at], known at the end
    std::vector<int> idx;
    max_height = std::max(max_height, 1 + host_ceil_log2(n));
    kids.assign(2 * (size_t)(n - 1), 0);
    TCHK(hipMalloc(&d_lo, sizeof(float) * 3 * (size_t)n));
    TCHK(hipMalloc(&d_hi, sizeof(float) * 3 * (size_t)n));
    TCHK(hipMalloc(&d_idx, sizeof(int) * (size_t)n));
    TCHK(hipMalloc(&d_idx2, sizeof(int) * (size_t)n));
    TCHK(hipMalloc(&d_kids, sizeof(int) * 2 * (size_t)(n - 1)));
    TCHK(hipMemcpy(d_lo, leaf_lo, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(d_hi, leaf_hi, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice));
    idx.resize(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    TCHK(hipMemcpy(d_idx, idx.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    (n > SUBT ? level : roots).push_back(Seg{0, n, 0, 1});
    while (!level.empty()) {
        const int S = (int)level.size();
        std::vector<Piece> pieces;
        std::vector<int> first(S + 1);
        for (int k = 0; k < S; ++k) {
            first[k] = (int)pieces.size();
            for (int a = level[k].begin; a < level[k].end; a += PIECE)
                pieces.push_back(Piece{k, a, std::min(level[k].end, a + PIECE)});
        }
        first[S] = (int)pieces.size();
        const unsigned NP = (unsigned)pieces.size();
        if (pieces.size() > piece_cap) {
            (void)hipFree(d_pb);
            (void)hipFree(d_pbins);
            (void)hipFree(d_cnt);
            d_pb = nullptr;
            d_pbins = nullptr;
            d_cnt = nullptr;
            piece_cap = std::max(pieces.size(), 2 * piece_cap);
            TCHK(hipMalloc(&d_pb, sizeof(double) * 6 * piece_cap));
            TCHK(hipMalloc(&d_pbins, sizeof(unsigned) * BINW * NB * piece_cap));
            TCHK(hipMalloc(&d_cnt, sizeof(int) * piece_cap));
        }
        if ((size_t)S > seg_cap) {
            (void)hipFree(d_sb);
            (void)hipFree(d_dec);
            (void)hipFree(d_hist);
            d_sb = nullptr;
            d_dec = nullptr;
            d_hist = nullptr;
            seg_cap = std::max<size_t>(S, 2 * seg_cap);
            TCHK(hipMalloc(&d_sb, sizeof(double) * 6 * seg_cap));
            TCHK(hipMalloc(&d_dec, sizeof(Decision) * seg_cap));
            TCHK(hipMalloc(&d_hist, sizeof(unsigned) * 256 * seg_cap));
            TCHK(hipMemset(d_hist, 0, sizeof(unsigned) * 256 * seg_cap));   // k_seg_pick leaves it cleared
        }
        // segments, pieces and the per-segment first piece in one upload
        std::vector<int> up(4 * (size_t)S + 3 * pieces.size() + S + 1);
        memcpy(up.data(), level.data(), sizeof(Seg) * S);
        memcpy(up.data() + 4 * (size_t)S, pieces.data(), sizeof(Piece) * pieces.size());
        memcpy(up.data() + 4 * (size_t)S + 3 * pieces.size(), first.data(), sizeof(int) * (S + 1));
        if (up.size() > lvl_cap) {
            (void)hipFree(d_lvl);
            d_lvl = nullptr;
            lvl_cap = std::max(up.size(), 2 * lvl_cap);
            TCHK(hipMalloc(&d_lvl, sizeof(int) * lvl_cap));
        }
        TCHK(hipMemcpy(d_lvl, up.data(), sizeof(int) * up.size(), hipMemcpyHostToDevice));
        const Seg* d_segs = reinterpret_cast<const Seg*>(d_lvl);
        const Piece* d_pieces = reinterpret_cast<const Piece*>(d_lvl + 4 * (size_t)S);
        const int* d_first = d_lvl + 4 * (size_t)S + 3 * pieces.size();

        hipLaunchKernelGGL(k_piece_cbounds, dim3(NP), dim3(BT), 0, 0, d_lo, d_hi, d_idx, d_pieces, d_pb);
        hipLaunchKernelGGL(k_seg_cbounds, dim3((unsigned)((8 * S + 255) / 256)), dim3(256), 0, 0, d_first, d_pb, d_sb, S);
        hipLaunchKernelGGL(k_piece_bins, dim3(NP), dim3(BT), 0, 0, d_lo, d_hi, d_idx, d_pieces, d_sb, d_pbins);
        hipLaunchKernelGGL(k_seg_split, dim3((unsigned)S), dim3(WAVE), 0, 0, d_segs, d_first, d_pbins, d_sb, max_height,
                           d_dec);
        TCHK(hipGetLastError());
        std::vector<Decision> dec(S);
        TCHK(hipMemcpy(dec.data(), d_dec, sizeof(Decision) * S, hipMemcpyDeviceToHost));
        bool median = false;
        for (const Decision& d : dec) median = median || d.mode == 2;
        if (median)
            for (int pass = 0; pass < DIGITS; ++pass) {
                hipLaunchKernelGGL(k_piece_hist, dim3(NP), dim3(BT), 0, 0, d_lo, d_hi, d_idx, d_pieces, d_dec, pass, d_hist);
                hipLaunchKernelGGL(k_seg_pick, dim3((unsigned)S), dim3(256), 0, 0, d_dec, pass, d_hist);
            }
        hipLaunchKernelGGL(k_piece_count, dim3(NP), dim3(BT), 0, 0, d_lo, d_hi, d_idx, d_pieces, d_segs, d_dec, d_cnt);
        hipLaunchKernelGGL(k_seg_scan, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, 0, d_first, d_cnt, S);
        hipLaunchKernelGGL(k_piece_scatter, dim3(NP), dim3(BT), 0, 0, d_lo, d_hi, d_idx, d_idx2, d_pieces, d_segs, d_dec,
                           d_cnt);
        hipLaunchKernelGGL(k_piece_copy, dim3(NP), dim3(BT), 0, 0, d_idx2, d_idx, d_pieces);
        TCHK(hipGetLastError());
        next.clear();
        for (int k = 0; k < S; ++k) {
            const Seg& sg = level[k];
            const int mid = sg.begin + dec[k].nleft;
            const Seg child[2] = {Seg{sg.begin, mid, sg.node + 1, sg.depth + 1},
                                  Seg{mid, sg.end, sg.node + dec[k].nleft, sg.depth + 1}};
            for (int c = 0; c < 2; ++c) {
                const int len = child[c].end - child[c].begin;
                const size_t slot = 2 * (size_t)sg.node + c;
                if (len == 1) {
                    fixes.push_back(Fix{slot, child[c].begin});
                    continue;
                }
                kids[slot] = child[c].node;
                (len > SUBT ? next : roots).push_back(child[c]);
            }
        }
        level.swap(next);
    }
    if (!roots.empty()) {
        TCHK(hipMalloc(&d_roots, sizeof(Seg) * roots.size()));
        TCHK(hipMemcpy(d_roots, roots.data(), sizeof(Seg) * roots.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_subtree, dim3((unsigned)roots.size()), dim3(WAVE), 0, 0, d_lo, d_hi, d_idx, d_roots,
                           max_height, d_kids);
        TCHK(hipGetLastError());
    }
    {
        // the subtrees' nodes from the device (a subtree of m leaves is the preorder range
        // [node, node + m - 1)); the level nodes' codes are the host's own
        std::vector<int> dk(2 * (size_t)(n - 1));
        TCHK(hipMemcpy(dk.data(), d_kids, sizeof(int) * dk.size(), hipMemcpyDeviceToHost));
        TCHK(hipMemcpy(idx.data(), d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        for (const Seg& r : roots)
            memcpy(&kids[2 * (size_t)r.node], &dk[2 * (size_t)r.node], sizeof(int) * 2 * (size_t)(r.end - r.begin - 1));
        for (const Fix& f : fixes) kids[f.slot] = -(idx[f.at] + 1);
    }
done:
#undef TCHK
    for (void* q : {(void*)d_lo, (void*)d_hi, (void*)d_idx, (void*)d_idx2, (void*)d_kids, (void*)d_lvl, (void*)d_cnt,
                    (void*)d_pb, (void*)d_sb, (void*)d_pbins, (void*)d_hist, (void*)d_dec, (void*)d_roots})
        (void)hipFree(q);
    return rc;
}

bool valid_leaves(const std::vector<float>& lo, const std::vector<float>& hi, const std::vector<float>& s) {
    const int n = (int)s.size();
    if (n < 2 || (int)lo.size() != 3 * n || (int)hi.size() != 3 * n) return false;
    for (int i = 0; i < 3 * n; ++i)
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || lo[i] > hi[i]) return false;
    return true;
}

}  // namespace

int pth::build_sah_tree_device(const std::vector<float>& leaf_lo, const std::vector<float>& leaf_hi,
                               const std::vector<float>& leaf_s, std::vector<TravInner>& out, int& height,
                               int bfs_levels, int max_height, bool& ok) {
    out.clear();
    height = 0;
    ok = false;
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count <= 0) {
        (void)hipGetLastError();
        g_err = "no HIP device visible";
        return PT_E_NODEVICE;
    }
    if (!valid_leaves(leaf_lo, leaf_hi, leaf_s)) return PT_OK;   // the host function's rejections
    std::vector<int> kids;
    const int32_t rc = device_shape(leaf_lo.data(), leaf_hi.data(), (int)leaf_s.size(), max_height, kids);
    if (rc != PT_OK) return rc;
    finish_sah_tree(kids, leaf_lo, leaf_hi, leaf_s, out, height, bfs_levels);
    ok = true;
    return PT_OK;
}

extern "C" const char* pt_trav_build_last_error(void) { return g_err.c_str(); }

extern "C" int32_t pt_trav_build(const float* leaf_lo, const float* leaf_hi, const float* leaf_s, int32_t n,
                                 int32_t bfs_levels, int32_t max_height, int32_t where, pt_trav_inner* out, int32_t cap,
                                 int32_t* num_inner, int32_t* height) {
    if (num_inner) *num_inner = 0;
    if (height) *height = 0;
    if (where != 0 && where != 1) {
        g_err = "where must be 0 (host) or 1 (device)";
        return PT_E_INVALID;
    }
    if (n < 0 || !num_inner || !height || (n > 0 && (!leaf_lo || !leaf_hi || !leaf_s))) {
        g_err = "bad arguments";
        return PT_E_INVALID;
    }
    const std::vector<float> lo(leaf_lo, leaf_lo + 3 * (size_t)n), hi(leaf_hi, leaf_hi + 3 * (size_t)n), s(leaf_s, leaf_s + n);
    std::vector<pth::TravInner> tt;
    int th = 0;
    bool ok = false;
    if (where == 0) {
        ok = pth::build_sah_tree(lo, hi, s, tt, th, bfs_levels, max_height);
    } else {
        const int rc = pth::build_sah_tree_device(lo, hi, s, tt, th, bfs_levels, max_height, ok);
        if (rc != PT_OK) return rc;
    }
    if (!ok) {
        g_err = "no tree: fewer than 2 leaves, a non-finite coordinate, or lo > hi";
        return PT_E_INVALID;
    }
    if (!out || cap < (int32_t)tt.size()) {
        g_err = "node capacity must be >= n - 1";
        return PT_E_INVALID;
    }
    for (size_t i = 0; i < tt.size(); ++i)
        for (int c = 0; c < 2; ++c) {
            const pth::TravChild& a = tt[i].c[c];
            pt_trav_child& b = out[i].c[c];
            memcpy(b.lo, a.lo, sizeof b.lo);
            memcpy(b.hi, a.hi, sizeof b.hi);
            b.ref = a.ref;
            b.leaf = a.leaf ? 1 : 0;
            b.s = a.s;
        }
    *num_inner = (int32_t)tt.size();
    *height = th;
    return PT_OK;
}
