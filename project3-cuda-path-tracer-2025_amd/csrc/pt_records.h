// pt_records.h — the records of the device scene buffers and the constants their layout depends on.
//
// No device code: a plain C++ compiler accepts this header (float4 comes from HIP's vector types,
// nothing else of HIP is used), so the host code that builds the buffers' byte images
// (host/scene_layout.cpp) and the kernels that read them (pt_device.h, pt_kernels.h) share one
// definition of every record.
#pragma once

#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>

namespace ptd {

constexpr int LDS_GEOMS = 64;  // fused kernel: geom tables up to this size are staged in LDS
constexpr int BLOCK = 256;     // threads per block of the per-path kernels
constexpr int MAXSTACK = 64;   // reference BVH stack (intersections.cu:167)
constexpr int MAXMAT = 256;    // materials a scene may hold (the staged pipeline's counting sort keys)

// kernel variants (pt_options.variant bits), selectable at run time for in-process A/B
enum : int {
    VAR_WAVE_ATOMIC = 1,   // compaction: one atomic per wave, no block barrier
    VAR_CAND_QUEUE = 2,    // intersection: per-lane queue of candidate geoms (see intersect_scene_q)
    VAR_SECTION_TIMING = 4,    // tools only: per-wave shader-clock section times into g_sections
    VAR_WAVE_REDIST = 8,   // intersection: the wave's (ray, candidate) pairs spread over all 64 lanes
    VAR_BVH_FAST = 16,     // BVH: exact-decision fast AABB test, near-first order, certified t-culling
    VAR_CTILE8 = 16,       // staged compaction: 8 items per thread (2048-item tiles)
    VAR_BVH_SPLIT = 32,    // fused + BVH_FAST + pair layout: rays that enter the mesh's root box are
                           // queued and traversed (then shaded) by k_bvh_bounce in full waves
    VAR_BVH_NODES = 64,    // host only: BVH_FAST on the node array instead of the DevPair layout (A/B)
    VAR_BLOCK_REDIST = 128,  // with VAR_WAVE_REDIST: the exchange spans the block (block_intersect)
    VAR_MAT_GROUP = 512,   // fused MATERIAL_SORTING: the block's paths regrouped by material between
                           // intersection and shading (group_by_material); set by pt_options.material_sort
    VAR_NO_TEX = 1024,     // host-set: no material samples a texture or bump map, so the fused kernels'
                           // shading is compiled without the texel fetches (whose registers otherwise set
                           // the kernels' VGPR count and occupancy)
    // pt_default_options: fastest in the in-process A/B (tools/ab_variants.py); every variant is bit-identical
    VAR_DEFAULT = VAR_CAND_QUEUE | VAR_WAVE_REDIST | VAR_BVH_FAST | VAR_BVH_SPLIT | VAR_BLOCK_REDIST,
};

// The candidate table's resolution: GRID_G^3 origin cells x 6 faces x GRID_B^2 direction bins.
// An entry is the AND of one mask per ratio bin (host/scene_layout.cpp, build_candidate_table), so the table is stored
// separably (PT_GRID_SEP): 2 GRID_B masks per (cell, face), 2.65 MB at 12 / 16 (L2-resident).
// 16 / 16 against 8 / 8: khaslana superset 5.68 -> 3.60 per ray, 13.8 -> 8.4 at the wave maximum,
// frame -3 %; 12 / 16 times the same as 16 / 16 with 10 % less k_bounce traffic
#ifndef PT_GRID_G
#define PT_GRID_G 12
#endif
#ifndef PT_GRID_B
#define PT_GRID_B 16
#endif
#ifndef PT_GRID_SEP
#define PT_GRID_SEP 1
#endif
constexpr int GRID_G = PT_GRID_G;
constexpr int GRID_B = PT_GRID_B;
constexpr int GRID_MIN_GEOMS = 16;

// DevCull records cull_candidates reads at a time; the host pads the record array to a multiple
#ifndef CULL_GROUP
#define CULL_GROUP 4
#endif

// 192-byte geom: inverseTransform | transform | invTranspose (affine rows, column-major
// m[c*3 + r]), a conservative world-space box (center, half extents incl. a safety margin) used
// only to SKIP exact tests that cannot change the result, + type + material
// The first 112 bytes are what the exact tests read (DevGeomHot): the fused kernel stages only
// that prefix in LDS, so a 44-geom table takes 4.9 KB instead of 8.4 KB of the block's LDS.
struct DevGeomHot {
    float inv[12];
    float fwd[12];
    int32_t type;
    int32_t materialid;
    int32_t away_axis;  // cubes: object axis of the smallest scale for the pre-test's "away" drop
                        // (see away_on_axis); -1: none (spheres, or matrices too large to bound)
    int32_t _pad0;
};
static_assert(sizeof(DevGeomHot) == 112, "DevGeomHot");
struct DevGeom {
    float inv[12];
    float fwd[12];
    int32_t type;
    int32_t materialid;
    int32_t away_axis;
    int32_t _pad0;
    float itr[12];
    float box_lo[3];    // conservative world box (outward-rounded, margin included)
    float box_hi[3];
    int32_t _pad[2];
};
static_assert(sizeof(DevGeom) == 192, "DevGeom");
static_assert(offsetof(DevGeom, itr) == sizeof(DevGeomHot), "DevGeomHot is DevGeom's prefix");

// Per-geom record of the candidate pre-test (block_intersect / wave_intersect), 48 bytes read
// as 3 float4 with no branch between them: the conservative world box of cull_geom, and the
// inverse-matrix row of away_on_axis's axis (all zero, never "away", for spheres and for cubes
// without one).
struct DevCull {
    float lo[3], hi[3];
    float row[4];          // inv[a], inv[3 + a], inv[6 + a], inv[9 + a]
    int32_t has_row;       // 1: a cube with an away axis (row valid)
    float _pad;
};
static_assert(sizeof(DevCull) == 48, "DevCull");

// 64-byte material: only what shading reads (sceneStructs.h:36-57)
struct DevMaterial {
    float color[3];
    float emittance;
    float hasReflective, hasRefractive, roughness, metallic;
    float ior;
    int32_t hasTexture;
    int32_t textureID;
    int32_t hasBumpMap;
    int32_t bumpID;
    float bumpScale;
    int32_t _pad[2];
};
static_assert(sizeof(DevMaterial) == 64, "DevMaterial");

// 32-byte BVH node: (min.xyz, a) (max.xyz, b); internal: a = left, b = right (<0: none);
// leaf (reference: triCount > 0 && start >= 0): a = start, b = -(triCount + 2)
struct DevNode {
    float4 lo;
    float4 hi;
};

// The two children of one internal BVH node, 64 bytes (VAR_BVH_FAST layout): popping a node
// costs ONE dependent record fetch that holds both child boxes and everything needed to push
// them.  ref >= 0 names the child's own pair record when ref < num_pairs, else the leaf
// ref - num_pairs, whose triangles sit in the 4-slot group hot4[4 * leaf ..]; leaves are numbered
// in the reference's visit order (push left, push right, pop: right subtree first), so a smaller
// hot4 index is an earlier triangle in the reference's DFS.  The cull constants are those of
// cull_threshold for s = max triangle edge below the child (x 1.01), precomputed per child.
struct DevPair {
    float4 l_lo;   // left box min.xyz  | left ref (int bits)
    float4 l_hi;   // left box max.xyz  | left cull constants (A | d, 16 bits each, pack_cull)
    float4 r_lo;   // right box min.xyz | right ref (int bits)
    float4 r_hi;   // right box max.xyz | right cull constants
};

// hot triangle record in leaf order (index k = node.start + i): 3 positions, 48 bytes
struct DevTriHot {
    float4 a;   // v0.xyz, v1.x
    float4 b;   // v1.yz, v2.xy
    float4 c;   // v2.z, triIndex (int bits), -, -
};

// cold triangle data, by reference triangle index (read once for the winner)
struct DevTriCold {
    float n0[3], n1[3], n2[3];   // vertex normals
    float uv0[2], uv1[2], uv2[2];
    float dpdu[3], dpdv[3];
    int32_t materialID;
    int32_t _pad;
};

}  // namespace ptd
