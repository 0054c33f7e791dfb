"""Parity of the HIP kernels (through the C-ABI) with the CPU oracle — needs an MI355X.

Bar: BIT-EXACT.  The kernels and the oracle's "portable" trig mode (trig_mode=1) evaluate every
float expression in the reference's order with the same deterministic sin/cos/pow
(include/pt/pt_libm.h), so camera rays, intersections, shading, compaction, sorting, the 8-bit
preview and whole accumulated images must agree to the last bit.  Against the oracle's glibc
mode (the configuration the SURVEY known answers pin) images agree within the statistical
tolerance of SURVEY §8c, checked in test_statistical_tolerance_vs_glibc_oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO, scene_path

pytestmark = pytest.mark.gpu

BIT = dict(trig_mode=1, arg_order=0)


def _oracle_pair(oracle, ptamd, name, res, depth=None):
    a = oracle.load_scene(scene_path(name), res=res, depth=depth)
    b = ptamd.SceneFile(scene_path(name), res=res, depth=depth)
    assert a.camera.tobytes() == b.camera.tobytes()
    return a, b


def _eq(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_rng_matches_rocthrust_on_gpu(ptamd):
    with open(os.path.join(GOLDEN, "rng_pin.json")) as f:
        pin = json.load(f)
    seeds = np.array([[it, idx, d] for it, idx, d, _, _ in pin["cases"]], np.int32)
    got = ptamd.rng_draws(seeds, 8)
    want = np.array([c[4] for c in pin["cases"]], np.uint32)
    assert _eq(got.view(np.uint32), want)


@pytest.mark.parametrize("name", ["cornell", "cornell_glass_test"])
def test_camera_rays_bitexact(name, oracle, ptamd):
    a, b = _oracle_pair(oracle, ptamd, name, (64, 48))
    tr = ptamd.PathTracer(b)
    o = oracle.options(**BIT)
    for it in (1, 7, 5000):
        gpu = tr.test_camera(it)
        ref = np.zeros(a.pixelcount, oracle.PATH)
        cam = a.camera.ctypes.data
        for y in range(a.height):
            for x in range(a.width):
                oracle.lib().or_generate_ray(cam, it, a.trace_depth, x, y, __import__("ctypes").byref(o),
                                             ref[x + y * a.width:].ctypes.data)
        assert _eq(gpu, ref), it
    tr.free()


def _random_paths(n, seed, box=5.0):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("color", "<f4", (3,)),
                              ("pixelIndex", "<i4"), ("remainingBounces", "<i4")]))
    p["origin"] = rng.uniform([-box, 0.05, -box], [box, 2 * box - 0.05, box], (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # axis-aligned and degenerate directions exercise the slab tests' inf / NaN paths
    d[: n // 16] = np.eye(3, dtype=np.float32)[np.arange(n // 16) % 3] * np.where(np.arange(n // 16) % 2, 1, -1)[:, None]
    d[n // 16: n // 16 + 4] = np.nan
    # components around geom_test's shared-reciprocal bound (|qd| >= 2^-40 in object space)
    k = np.arange(24)
    tiny = np.ldexp(np.where(k % 2, -1.0, 1.0) * (1 + (k % 3 - 1) * 2.0 ** -23), -34 - k // 2)
    d[n // 16 + 4: n // 16 + 28] = np.stack([np.full(24, 0.6), tiny, np.full(24, -0.8)], 1)
    p["direction"] = d
    p["color"] = rng.uniform(0.1, 1.0, (n, 3)).astype(np.float32)
    p["pixelIndex"] = rng.integers(0, 640000, n)
    p["remainingBounces"] = rng.integers(1, 9, n)
    return p


def _oracle_isects(oracle, a, paths):
    import ctypes
    s = a.c_struct()
    o = oracle.options(**BIT)
    out = np.zeros(len(paths), oracle.ISECT)
    pa = np.ascontiguousarray(paths, oracle.PATH)
    for i in range(len(paths)):
        oracle.lib().or_compute_intersection(ctypes.byref(s), ctypes.byref(o), pa[i:].ctypes.data, out[i:].ctypes.data)
    return out


@pytest.mark.parametrize("name,variant", [("cornell", 10), ("cornell_obj_bnnuy", 10), ("cornell_obj_khaslana", 10),
                                          ("synthetic_textured_bump", 10), ("cornell_obj_bnnuy", 26),
                                          ("cornell_obj_khaslana", 26), ("synthetic_textured_bump", 26),
                                          ("cornell_obj_bnnuy", 90), ("cornell_obj_khaslana", 90)])
def test_intersect_bitexact(name, variant, oracle, ptamd):
    a, b = _oracle_pair(oracle, ptamd, name, (96, 96))      # wavefront capacity >= 9216 paths
    tr = ptamd.PathTracer(b, variant=variant)
    paths = _random_paths(3000, 11)
    cam = tr.test_camera(3)[:4000]
    paths = np.concatenate([paths.astype(oracle.PATH), cam])
    gpu = tr.test_intersect(paths)
    ref = _oracle_isects(oracle, a, paths)
    fields = ("t", "surfaceNormal", "materialId")
    if len(a.textures):                      # textured scenes also carry uv / dpdu / dpdv
        hit = ref["t"] > 0
        ref["uv"][~hit], ref["dpdu"][~hit], ref["dpdv"][~hit] = 0, 0, 0
        fields += ("uv", "dpdu", "dpdv")
    for f in fields:
        assert _eq(gpu[f], ref[f]), (name, f, np.where(gpu[f].view(np.uint32) != ref[f].view(np.uint32))[0][:10])
    assert (gpu["t"] > 0).mean() > 0.3
    tr.free()


@pytest.mark.parametrize("name", ["cornell", "cornell_glass_test", "cornell_microfacet_test",
                                  "cornell_reflective_test", "cornell_transmissive_test", "cornell_obj_bnnuy",
                                  "synthetic_textured_bump", "cornell_obj_phatphuck_microfacet"])
def test_shade_bitexact(name, oracle, ptamd):
    import ctypes
    a, b = _oracle_pair(oracle, ptamd, name, (80, 80))      # wavefront capacity >= 6400 paths
    tr = ptamd.PathTracer(b)
    paths = np.concatenate([tr.test_camera(2)[:3000], _random_paths(2000, 5).astype(oracle.PATH)])
    isects = _oracle_isects(oracle, a, paths)
    s = a.c_struct()
    o = oracle.options(**BIT)
    for it in (2, 9):
        ref = paths.copy()
        for i in range(len(ref)):
            oracle.lib().or_shade(ctypes.byref(s), ctypes.byref(o), it, isects[i:].ctypes.data, ref[i:].ctypes.data)
        gpu = tr.test_shade(it, isects, paths)
        assert _eq(gpu, ref), (name, it, np.where(gpu.tobytes() != ref.tobytes()))
    tr.free()


@pytest.mark.parametrize("n", [0, 1, 63, 2047, 2048, 2049, 100000, 640000])
@pytest.mark.parametrize("frac", [0.0, 0.82, 1.0])
def test_stable_compaction(n, frac, oracle, ptamd):
    a, b = _oracle_pair(oracle, ptamd, "cornell", (800, 800))
    tr = ptamd.PathTracer(b)
    rng = np.random.default_rng(n + int(frac * 100))
    p = np.zeros(n, oracle.PATH)
    p["pixelIndex"] = np.arange(n)
    p["origin"] = rng.normal(size=(n, 3))
    p["remainingBounces"] = np.where(rng.random(n) < frac, rng.integers(1, 9, n), rng.integers(-2, 1, n))
    got = tr.test_compact(p)
    want = p[p["remainingBounces"] > 0]          # thrust::stable_partition(PathAlive) order
    assert _eq(got, want)
    tr.free()


@pytest.mark.parametrize("nkeys,n", [(5, 10000), (27, 70000), (1, 3000), (7, 2049), (27, 20_000_003),
                                     (5, 30_720_000)])
def test_material_sort_stable(nkeys, n, ptamd, oracle):
    """k_sort_hist / k_sort_scan / k_sort_scatter == np.argsort(kind="stable") (thrust::
    stable_sort_by_key, pathtrace.cu:730-735), up to the ~20-30M paths of a benched 48-frame pass:
    there k_sort_scan's 1024 threads each scan a run of ~260 (key, tile) entries."""
    a, b = _oracle_pair(oracle, ptamd, "cornell_obj_khaslana" if nkeys > 7 else "cornell", (400, 400))
    tr = ptamd.PathTracer(b)
    rng = np.random.default_rng(nkeys)
    k = min(nkeys, len(b.materials))
    isects = np.zeros(n, ptamd.ISECT)
    if n > 10_000_000:    # runs of equal keys as well as scattered ones
        isects["materialId"] = np.where(rng.random(n) < 0.5, rng.integers(0, k, n),
                                        (np.arange(n) // 4099) % k)
    else:
        isects["materialId"] = rng.integers(0, k, n)
    perm = tr.test_sort(isects)
    assert _eq(perm, np.argsort(isects["materialId"], kind="stable").astype(np.int32))
    tr.free()


def test_pbo_bitexact(oracle, ptamd):
    rng = np.random.default_rng(3)
    img = rng.uniform(-1, 40, (5000, 3)).astype(np.float32)
    img[0, 0], img[1, 1], img[2, 2] = np.nan, np.inf, -np.inf
    for it in (1, 9, 37):
        gpu = ptamd.image_to_pbo(img, it)
        ref = np.zeros((len(img), 4), np.uint8)
        oracle.lib().or_image_to_pbo(img.ctypes.data, len(img), it, ref.ctypes.data)
        assert _eq(gpu, ref)


FRAME_CASES = [
    ("cornell", (64, 64), None, {}),
    ("cornell", (64, 64), None, {"pipeline": 1}),
    ("cornell", (64, 64), None, {"pipeline": 1, "stream_compaction": 0}),
    ("cornell_glass_test", (64, 64), None, {"pipeline": 1, "material_sort": 1}),
    ("cornell_glass_test", (64, 64), None, {}),
    ("cornell_microfacet_test", (64, 64), None, {}),
    ("cornell_reflective_test", (48, 48), None, {}),
    ("cornell_transmissive_test", (48, 48), None, {"pipeline": 1}),
    ("cornell_obj_bnnuy", (64, 64), None, {}),
    ("cornell_obj_bnnuy", (64, 64), None, {"pipeline": 1, "material_sort": 1}),
    ("cornell_obj_khaslana", (48, 48), 12, {}),
    ("cornell", (40, 30), 0, {}),
    ("cornell", (40, 30), 1, {"pipeline": 1}),
    ("synthetic_textured_bump", (64, 64), None, {}),
    ("cornell", (64, 64), None, {"variant": 10}),                       # wave-redistributed exact tests
    ("cornell_glass_test", (64, 64), None, {"variant": 10}),
    ("cornell_obj_bnnuy", (48, 48), None, {"variant": 10}),
    ("synthetic_textured_bump", (48, 48), None, {"variant": 10}),
    ("cornell_obj_bnnuy", (64, 64), None, {"variant": 26}),             # fast BVH traversal
    ("cornell_obj_bnnuy", (64, 64), None, {"variant": 18, "pipeline": 1}),
    ("cornell_obj_khaslana", (48, 48), 12, {"variant": 26}),
    ("cornell_obj_bnnuy", (64, 64), None, {"variant": 90}),             # fast BVH on the node array
    ("cornell_obj_khaslana", (48, 48), 12, {"variant": 90, "pipeline": 1}),
    ("cornell", (64, 64), None, {"variant": 154}),                      # block-wide exchange
    ("cornell_glass_test", (64, 64), None, {"variant": 154}),
    ("cornell_obj_khaslana", (48, 48), 12, {"variant": 58}),             # per-wave exchange
    ("synthetic_textured_bump", (48, 48), None, {"variant": 58}),
    ("cornell_obj_bnnuy", (64, 64), None, {"variant": 58}),             # split: traversal queue kernel
    ("cornell_obj_khaslana", (48, 48), 12, {"variant": 58}),
    ("synthetic_textured_bump", (48, 48), None, {"variant": 58}),
    ("cornell_obj_phatphuck_texture_test", (48, 48), None, {"variant": 58}),
    ("synthetic_textured_bump", (48, 48), None, {"variant": 26}),
    ("synthetic_textured_bump", (64, 64), None, {"pipeline": 1}),
    ("synthetic_textured_bump", (48, 48), None, {"pipeline": 1, "material_sort": 1}),
    ("cornell_obj_phatphuck_texture_test", (48, 48), None, {}),
    ("cornell_obj_phatphuck_microfacet", (48, 48), None, {"pipeline": 1}),
    # MATERIAL_SORTING on the fused pipeline (block-local regrouping by material, VAR_MAT_GROUP)
    ("cornell_glass_test", (64, 64), None, {"material_sort": 1}),
    ("cornell_multiple_glass", (64, 64), None, {"material_sort": 1}),
    ("cornell_obj_khaslana", (48, 48), 12, {"material_sort": 1}),
    ("synthetic_textured_bump", (48, 48), None, {"material_sort": 1}),
    ("cornell_obj_phatphuck_microfacet", (48, 48), None, {"material_sort": 1}),
]


@pytest.mark.parametrize("name,res,depth,opts", FRAME_CASES)
def test_frames_bitexact(name, res, depth, opts, oracle, ptamd):
    a, b = _oracle_pair(oracle, ptamd, name, res, depth)
    tr = ptamd.PathTracer(b, **opts)
    r = oracle.Renderer(a, oracle.options(stream_compaction=opts.get("stream_compaction", 1),
                                          material_sort=opts.get("material_sort", 0), **BIT))
    for it in (1, 2, 3):
        live = r.trace(it)
        tr.trace(it)
        st = tr.stats()
        if opts.get("stream_compaction", 1) and a.trace_depth > 0:
            want = [int(x) if x >= 0 else 0 for x in live]    # oracle: -1 = bounce not run (n hit 0)
            assert st["live"] == want, (it, st["live"], live.tolist())
        img = tr.image()
        assert _eq(img, r.image), (name, it, int(np.sum(img.view(np.uint32) != r.image.view(np.uint32))))
    tr.free()


PASS_CASES = [
    ("cornell", (64, 64), None, {}, 2),
    ("cornell", (64, 64), None, {}, 4),
    ("cornell", (64, 64), None, {"pipeline": 1}, 3),
    ("cornell", (96, 96), None, {"pipeline": 1}, 5),
    ("cornell", (64, 64), None, {"pipeline": 1, "stream_compaction": 0}, 4),
    ("cornell_glass_test", (64, 64), None, {"pipeline": 1, "material_sort": 1}, 2),
    ("cornell_glass_test", (48, 40), None, {"use_graph": 0}, 5),
    ("cornell_obj_bnnuy", (48, 48), None, {}, 0),
    ("cornell_obj_khaslana", (32, 32), 12, {"pipeline": 1}, 16),
    ("cornell", (40, 30), 0, {}, 3),
    ("cornell_microfacet_test", (50, 50), None, {"shard_mode": 1, "shard_rank": 1, "shard_count": 2}, 4),
    ("synthetic_textured_bump", (48, 48), None, {}, 4),
    ("cornell_multiple_glass", (64, 64), None, {"variant": 10}, 8),
    ("cornell_multiple_glass", (64, 64), None, {"material_sort": 1}, 4),
    ("cornell_obj_bnnuy", (48, 48), None, {"material_sort": 1}, 3),
]


@pytest.mark.parametrize("name,res,depth,opts,fpp", PASS_CASES)
def test_multi_frame_passes_bitexact(name, res, depth, opts, fpp, oracle, ptamd):
    """pt_trace_frames traces F frames per wavefront pass (frames_per_pass; 0 = auto); the image
    after 5 frames (passes F, F, ..., remainder) equals 5 sequential oracle frames bit-for-bit,
    and the device path-segment counters equal the oracle's."""
    a, b = _oracle_pair(oracle, ptamd, name, res, depth)
    tr = ptamd.PathTracer(b, frames_per_pass=fpp, **opts)
    r = oracle.Renderer(a, oracle.options(stream_compaction=opts.get("stream_compaction", 1),
                                          material_sort=opts.get("material_sort", 0), **BIT))
    segs = 0
    for it in range(1, 6):
        live = r.trace(it)
        segs += int(np.maximum(live, 0).sum()) if a.trace_depth > 0 else 0
    tr.trace_frames(1, 5)
    st = tr.stats()
    assert st["frames_total"] == 5
    img = tr.image()
    want = r.image
    if opts.get("shard_mode") == 1:                 # only this shard's rows are traced
        from ptamd import dist as D
        w, h = res
        mask = np.zeros(h, bool)
        mask[D.owned_rows(h, 8, opts["shard_count"], opts["shard_rank"])] = True
        want = want.copy()
        want[~np.repeat(mask, w)] = 0.0
    elif opts.get("stream_compaction", 1) and a.trace_depth > 0:
        assert st["segments_total"] == segs
    assert _eq(img, want), (name, fpp, int(np.sum(img.view(np.uint32) != want.view(np.uint32))))
    # the profiling path groups frames the same way and traces the same image
    p = tr.profile(6, 3)
    assert p["frames"] == 3
    for it in range(6, 9):
        r.trace(it)
    if opts.get("shard_mode") != 1:
        assert _eq(tr.image(), r.image)
    tr.free()


def test_full_resolution_cornell(oracle, ptamd):
    """BASELINE config 2 (800x800, depth 8): fused == staged == oracle, live counts included."""
    a, b = _oracle_pair(oracle, ptamd, "cornell", None)
    r = oracle.Renderer(a, oracle.options(**BIT))
    live = r.trace(1)
    imgs = []
    for pipe in (0, 1):
        tr = ptamd.PathTracer(b, pipeline=pipe)
        tr.trace(1)
        assert tr.stats()["live"] == live.tolist()
        imgs.append(tr.image())
        tr.free()
    assert _eq(imgs[0], r.image) and _eq(imgs[1], r.image)


@pytest.mark.parametrize("name", ["cornell_obj_bnnuy", "cornell_obj_khaslana"])
def test_full_resolution_mesh_fast_bvh(name, oracle, ptamd):
    """800x800 frames of the BVH scenes with the fast traversal (variant 26): bit-exact vs the
    oracle's reference-order DFS, live counts included."""
    a, b = _oracle_pair(oracle, ptamd, name, None)
    r = oracle.Renderer(a, oracle.options(**BIT))
    tr = ptamd.PathTracer(b, variant=26)
    for it in (1, 2):
        live = r.trace(it)
        tr.trace(it)
        assert tr.stats()["live"] == [int(x) if x >= 0 else 0 for x in live]
    assert _eq(tr.image(), r.image)
    tr.free()


def _many_geoms_scene(path, n):
    """cornell.json plus n small cubes / spheres (mixed materials, some rotated and scaled
    non-uniformly): more geoms than the fused kernel stages in LDS (LDS_GEOMS = 64), so the
    global-table intersection path runs."""
    with open(scene_path("cornell")) as f:
        d = json.load(f)
    d["Materials"]["mirror"] = {"RGB": [0.9, 0.9, 0.9], "TYPE": "Specular"}
    d["Materials"]["glass"] = {"RGB": [0.95, 0.95, 0.95], "TYPE": "Refractive", "IOR": 1.5}
    rng = np.random.default_rng(7)
    mats = ["diffuse_red", "diffuse_green", "diffuse_white", "mirror", "glass"]
    for i in range(n):
        d["Objects"].append({"TYPE": "cube" if i % 2 else "sphere", "MATERIAL": mats[i % len(mats)],
                             "TRANS": [float(x) for x in rng.uniform([-4, 0.5, -4], [4, 9, 3])],
                             "ROTAT": [float(x) for x in rng.uniform(0, 90, 3)],
                             "SCALE": [float(x) for x in rng.uniform(0.2, 0.9, 3)]})
    with open(path, "w") as f:
        json.dump(d, f)
    return str(path)


@pytest.mark.parametrize("opts", [{}, {"pipeline": 1}, {"variant": 10}])
def test_more_geoms_than_lds_table(opts, tmp_path, oracle, ptamd):
    path = _many_geoms_scene(tmp_path / "many.json", 72)
    a, b = _oracle_pair(oracle, ptamd, path, (48, 48))
    assert len(b.geoms) > 64
    tr = ptamd.PathTracer(b, **opts)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in (1, 2):
        r.trace(it)
        tr.trace(it)
    assert _eq(tr.image(), r.image)
    assert np.isfinite(r.image).mean() > 0.99 and r.image.sum() > 0
    tr.free()


@pytest.mark.parametrize("n,res,iters", [(12, (64, 64), 3), (33, (64, 64), 3), (55, (48, 48), 2)])
def test_candidate_table_scenes_bitexact(n, res, iters, tmp_path, oracle, ptamd):
    """Scenes of GRID_MIN_GEOMS..64 geoms run the pre-test from the candidate table (a per-lane
    superset of the geoms a ray from its origin cell in its direction bin can hit): random cubes
    and spheres, rotated and scaled, mirrors and glass sending rays everywhere, two objects
    outside the room (origins outside the walls) -- bit-exact against the oracle, live counts too."""
    path = _many_geoms_scene(tmp_path / "grid.json", n)
    with open(path) as f:
        d = json.load(f)
    d["Objects"] += [{"TYPE": "sphere", "MATERIAL": "mirror", "TRANS": [0, 5, 14], "ROTAT": [0, 0, 0],
                      "SCALE": [3, 3, 3]},
                     {"TYPE": "cube", "MATERIAL": "diffuse_white", "TRANS": [-9, 2, 0], "ROTAT": [10, 20, 30],
                      "SCALE": [1, 6, 2]}]
    with open(path, "w") as f:
        json.dump(d, f)
    a, b = _oracle_pair(oracle, ptamd, path, res)
    assert 16 <= len(b.geoms) <= 64
    tr = ptamd.PathTracer(b)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in range(1, iters + 1):
        live = r.trace(it)
        tr.trace(it)
        assert tr.stats()["live"] == [int(x) if x >= 0 else 0 for x in live]
    assert _eq(tr.image(), r.image)
    tr.trace_frames(iters + 1, 4)
    for it in range(iters + 1, iters + 5):
        r.trace(it)
    assert _eq(tr.image(), r.image)
    tr.free()


def test_prepared_graphs_equal_oracle(oracle, ptamd):
    """pt_prepare_frames captures the pass graphs a later pt_trace_frames replays (bench.py keeps
    the capture out of its timed region); the frames traced through them equal the oracle."""
    a, b = _oracle_pair(oracle, ptamd, "cornell_glass_test", (40, 40))
    tr = ptamd.PathTracer(b, frames_per_pass=4)
    tr.prepare_frames(7)                       # passes of 4 and 3
    tr.trace_frames(1, 7)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in range(1, 8):
        r.trace(it)
    assert tr.stats()["frames_total"] == 7
    assert _eq(tr.image(), r.image)
    tr.free()


def test_graph_replay_equals_eager(oracle, ptamd):
    a, b = _oracle_pair(oracle, ptamd, "cornell_glass_test", (96, 96))
    imgs = []
    for g in (1, 0):
        tr = ptamd.PathTracer(b, use_graph=g)
        tr.trace_frames(1, 6)
        imgs.append(tr.image())
        tr.free()
    assert _eq(imgs[0], imgs[1])


@pytest.mark.parametrize("name,depth,sort", [
    ("cornell", None, 0),                    # BASELINE configs[1]
    ("cornell_glass_test", None, 1),         # configs[2]: specular / refractive + material sort
    ("cornell_obj_bnnuy", None, 0),          # configs[3]: glass mesh, BVH traversal
    ("cornell_obj_khaslana", 12, 0),         # configs[4]: 44 geoms + mesh, microfacet, depth 12
])
def test_statistical_tolerance_vs_glibc_oracle(name, depth, sort, oracle, ptamd):
    """SURVEY §8c policy against the oracle's glibc (reference-pinned) mode, 100x100, 4 spp, for
    every BASELINE GPU workload: NaN counts within max(2, 20%); >= 99.9% of finite pixels within
    1e-4 abs per channel; |mean_gpu - mean_oracle| / mean_oracle <= 1e-4.  (Measured with the
    oracle's two modes on the host: khaslana d12 has 1 pixel of 10,000 beyond 1e-4 -- a path whose
    glibc and deterministic sincos differ by an ulp and then diverge -- the others none.)"""
    a, b = _oracle_pair(oracle, ptamd, name, (100, 100), depth)
    r = oracle.Renderer(a, oracle.options(trig_mode=0, arg_order=0, material_sort=sort))
    tr = ptamd.PathTracer(b, material_sort=sort)
    for it in range(1, 5):
        r.trace(it)
        tr.trace(it)
    g, c = tr.image() / 4, r.image / 4
    tr.free()
    ng, nc = np.isnan(g).any(1).sum(), np.isnan(c).any(1).sum()
    assert abs(int(ng) - int(nc)) <= max(2, 0.2 * max(ng, nc))
    fin = np.isfinite(g).all(1) & np.isfinite(c).all(1)
    close = (np.abs(g[fin] - c[fin]) <= 1e-4).all(1).mean()
    assert close >= 0.999, close
    assert abs(g[fin].mean() - c[fin].mean()) / c[fin].mean() <= 1e-4


def test_cpp_boundary_pt_render(tmp_path, oracle, ptamd):
    """The reference's C++ boundary (pathtraceInit / pathtrace / pathtraceFree) driven by the
    headless main.cpp replacement; its PFM (accumulated image) equals the oracle's."""
    exe = os.path.join(PKG, "build", "pt_render")
    out = str(tmp_path / "cornell")
    subprocess.run([exe, scene_path("cornell"), "--spp", "3", "--res", "64x64", "--out", out], check=True,
                   timeout=120)
    with open(out + ".pfm", "rb") as f:
        head = [f.readline() for _ in range(3)]
        data = np.frombuffer(f.read(), np.float32).reshape(64, 64, 3)[::-1].reshape(-1, 3)
    assert head[0].strip() == b"PF"
    a = oracle.load_scene(scene_path("cornell"), res=(64, 64))
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in (1, 2, 3):
        r.trace(it)
    assert _eq(data, r.image)
    # the PNG is saveImage's (flip, 1/spp, clamp, x255) in stb_image_write's exact bytes
    ref_png = str(tmp_path / "ref")
    ptamd.save_png(r.image, 64, 64, 3, ref_png)
    with open(out + ".png", "rb") as f, open(ref_png + ".png", "rb") as g:
        assert f.read() == g.read()


def test_pixel_shards_sum_to_full_frame(oracle, ptamd):
    """PIXELS sharding (ptamd/dist.py): 3 row-band shards traced separately sum, exactly, to the
    unsharded frame — what the RCCL combine does across GPUs."""
    _, b = _oracle_pair(oracle, ptamd, "cornell_glass_test", (64, 50))
    tr = ptamd.PathTracer(b)
    tr.trace_frames(1, 2)
    full = tr.image()
    tr.free()
    acc = np.zeros_like(full)
    live = 0
    for r in range(3):
        tr = ptamd.PathTracer(b, shard_mode=ptamd.SHARD_PIXELS, shard_rank=r, shard_count=3, shard_rows=8)
        tr.trace_frames(1, 2)
        acc += tr.image()
        live += tr.stats()["pixels"]
        tr.free()
    assert live == 64 * 50
    assert _eq(acc, full)


# ---- the HIP intersection path against the reference's OWN intersections.cu (tests/golden/ref_pin.json) ----
with open(os.path.join(GOLDEN, "ref_pin.json")) as _f:
    _REF_PIN = json.load(_f)


@pytest.mark.parametrize("variant", [None, 26, 10])
@pytest.mark.parametrize("name", sorted(_REF_PIN["isect"]))
def test_intersections_match_reference(name, variant, ptamd):
    """computeIntersections of the reference (box / sphere / bvhMeshIntersectionTest compiled from
    /root/reference/src/intersections.cu, oracle/ref_pins/ref_harness.cpp) on 4096 probe rays per
    scene: axis-aligned, sub-1e-5 and signed-zero components, NaN / inf / zero rays, rays aimed at
    triangle vertices and shared-edge midpoints (t ties).  The full 52-B records are compared
    (NaNs canonicalised), with the default kernel variant and the reference-order / node-array
    traversals."""
    import refpins as R
    ref = _REF_PIN["isect"][name]
    b = ptamd.SceneFile(scene_path(name), res=(96, 96))       # wavefront capacity >= 9216 paths
    raw = ptamd.SceneFile(scene_path(name), viewer_camera=False)
    rays = R.rays(R.ISECT_RAYS, seed=len(name), targets=R.scene_targets(raw.geoms, raw.triangles))
    assert R.digest(rays) == ref["rays_sha256"]
    opts = {} if variant is None else {"variant": variant}
    tr = ptamd.PathTracer(b, **opts)
    got = tr.test_intersect(rays.astype(ptamd.PATH))
    tr.free()
    assert int((got["t"] > 0).sum()) == ref["hits"]
    assert R.digest(R.pack(got, R.P_ISECT)) == ref["isect_sha256"]


# ---- the configurations bench.py times, at their full size (round-1 VERDICT "What's weak" 2) ----
@pytest.mark.parametrize("name", ["cornell", "cornell_obj_bnnuy"])
def test_benched_configuration_bitexact(name, oracle, ptamd):
    """Exactly what bench.py times for BASELINE configs[1] / configs[3]: 800x800, default options
    (variant 186: block exchange, split BVH queue, pair layout), auto frames-per-pass (128 at 800x800:
    the 40 frames run as one wavefront pass of 40).  Image and per-bounce live totals == the oracle's
    (OpenMP over paths) frame by frame."""
    a, b = _oracle_pair(oracle, ptamd, name, None)
    tr = ptamd.PathTracer(b)
    tr.trace_frames(1, 40)
    st = tr.stats()
    assert st["frames_per_pass"] == 128 and st["last_pass_frames"] == 40 and st["frames_total"] == 40
    r = oracle.Renderer(a, oracle.options(**BIT))
    tot = np.zeros(a.trace_depth, np.int64)
    for it in range(1, 41):
        tot += np.maximum(r.trace(it), 0)
    assert st["live_total"][:a.trace_depth] == tot.tolist()
    img = tr.image()
    assert _eq(img, r.image), (name, int(np.sum(img.view(np.uint32) != r.image.view(np.uint32))))
    tr.free()


@pytest.mark.parametrize("pipeline", ["fused", "staged"])
def test_benched_sort_configuration_bitexact(pipeline, oracle, ptamd):
    """What bench.py's configs[2] sub-records time: cornell_glass_test 800x800 depth 8 WITH the
    material sort -- fused (the block-local regrouping by material between intersection and
    shading) and staged (k_sort_hist / k_sort_scan / k_sort_scatter before every k_shade) --, auto
    frames per pass, 48 frames as one wavefront pass of ~30M paths.  Image and per-bounce live
    totals == the oracle's (material_sort=1) frame by frame."""
    a, b = _oracle_pair(oracle, ptamd, "cornell_glass_test", None)
    tr = ptamd.PathTracer(b, pipeline=ptamd.PIPELINE_STAGED if pipeline == "staged" else ptamd.PIPELINE_FUSED,
                          material_sort=1)
    tr.prepare_frames(48)
    tr.trace_frames(1, 48)
    st = tr.stats()
    assert st["frames_per_pass"] >= 48 and st["last_pass_frames"] == 48 and st["frames_total"] == 48
    r = oracle.Renderer(a, oracle.options(material_sort=1, **BIT))
    tot = np.zeros(a.trace_depth, np.int64)
    for it in range(1, 49):
        tot += np.maximum(r.trace(it), 0)
    assert st["live_total"][:a.trace_depth] == tot.tolist()
    img = tr.image()
    assert _eq(img, r.image), int(np.sum(img.view(np.uint32) != r.image.view(np.uint32)))
    tr.free()


def test_rccl_framebuffer_combine_device_branches():
    """The RCCL (nccl backend) branches of ptamd/dist.py, which only an N-GPU run executes:
    a world-size-1 RCCL group in a fresh child process runs TileGather.run() and
    ImageReduce.run() on the library's HBM framebuffer, and scatters 3 pixel shards' device tiles
    (traced one after another on this GPU) into rank 0's framebuffer through the same
    index_select / index_copy_ code, with the tracer's host-copy methods disabled: bit-identical
    to the unsharded frame (tests/rccl_child.py)."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "rccl_child.py"),
                        scene_path("cornell_glass_test"), "3", "3"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["tilegather_run_identity"] and out["imagereduce_run_identity"]
    assert out["shards_scatter_equal"], out
    assert out["image_sum"] > 0


def test_pass_buffers_sized_on_first_use(oracle, ptamd):
    """pt_init holds one frame's wavefront (what the drop-in pathtrace() and the viewer use); a
    pass of F frames grows the buffers when it is first prepared or traced, and the frames after the
    growth are still bit-exact (the pass graphs captured before it are released)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so.7")          # the HIP runtime libptamd.so runs on (not torch's)

    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    a, b = _oracle_pair(oracle, ptamd, "cornell_obj_bnnuy", None)
    free0 = free_bytes()
    tr = ptamd.PathTracer(b)                       # auto F = 128 at 800x800
    used_init = free0 - free_bytes()
    assert used_init < 1.0e9, used_init             # ~0.25 GB: one frame (x2 for the split queue's segments)
    r = oracle.Renderer(a, oracle.options(**BIT))
    tr.trace(1)
    r.trace(1)
    tr.prepare_frames(16)
    used_pass = free0 - free_bytes()
    assert used_pass > 8 * used_init, (used_init, used_pass)
    tr.trace_frames(2, 16)
    tr.trace(18)
    for it in range(2, 19):
        r.trace(it)
    assert _eq(tr.image(), r.image)
    tr.free()


def test_config5_khaslana_1600_depth12(oracle, ptamd):
    """BASELINE configs[4] at its stated size: cornell_obj_khaslana 1600x1600, depth 12 (stand-in
    meshes, 49760 triangles), default options, 2 frames: image and live counts bit-exact."""
    a, b = _oracle_pair(oracle, ptamd, "cornell_obj_khaslana", (1600, 1600), 12)
    tr = ptamd.PathTracer(b)
    tr.trace_frames(1, 2)
    st = tr.stats()
    r = oracle.Renderer(a, oracle.options(**BIT))
    tot = np.zeros(12, np.int64)
    for it in (1, 2):
        tot += np.maximum(r.trace(it), 0)
    assert st["live_total"][:12] == tot.tolist()
    assert _eq(tr.image(), r.image)
    tr.free()


def test_api_frame_traced_depth_and_host_copy(oracle, ptamd):
    """pathtrace() as main.cpp:463 calls it: F = 1, the accumulated image copied to the (page-
    locked) host buffer every call, TracedDepth = the bounces the frame actually ran
    (pathtrace.cu:759-770)."""
    import ctypes
    a, b = _oracle_pair(oracle, ptamd, "cornell", (64, 64))
    td = ctypes.c_int32(-7)
    ptamd.lib.pt_init_data_container(ctypes.byref(td))
    tr = ptamd.PathTracer(b)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in (1, 2, 3):
        live = r.trace(it)
        img = tr.trace(it, copy_image=True)
        assert _eq(img, r.image) and img is tr.trace.__self__._host_image
        ran = next((k for k in range(1, a.trace_depth) if live[k] <= 0), a.trace_depth)
        assert td.value == ran
    tr.free()
    # depth 1 scene: every path ends after one bounce
    a1, b1 = _oracle_pair(oracle, ptamd, "cornell", (32, 32), 1)
    tr = ptamd.PathTracer(b1)
    tr.trace(1, copy_image=True)
    assert td.value == 1
    tr.free()
    ptamd.lib.pt_init_data_container(None)


def _skewed_mesh_scene(tmp_path, base, n=140000):
    """cornell.json plus an OBJ of n small triangles whose x centroids shrink geometrically
    (base^-(i mod 20000)): the reference's midpoint splits make a tree far deeper than its
    reference-order DFS stack, with > 65535 node refs (no pair layout)."""
    rng = np.random.default_rng(1)
    k = np.arange(n) % 20000
    c = np.stack([10.0 * base ** (-k.astype(np.float64)) - 5.0, 1.0 + 8.0 * rng.random(n),
                  -4.0 + 8.0 * rng.random(n)], 1).astype(np.float32)
    lines = []
    for p in c:
        lines.append("v %.6f %.6f %.6f\nv %.6f %.6f %.6f\nv %.6f %.6f %.6f" % (
            p[0], p[1], p[2], p[0] + 0.02, p[1], p[2], p[0], p[1] + 0.02, p[2] + 0.01))
    faces = "\n".join("f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(n))
    (tmp_path / "mesh.obj").write_text("\n".join(lines) + "\n" + faces + "\n")
    with open(scene_path("cornell")) as f:
        d = json.load(f)
    d["Objects"].append({"TYPE": "obj", "PATH": "/mesh.obj", "MATERIAL": "diffuse_red",
                         "TRANS": [0, 0, 0], "ROTAT": [0, 0, 0], "SCALE": [1, 1, 1]})
    path = tmp_path / "skewed.json"
    path.write_text(json.dumps(d))
    return str(path)


@pytest.mark.parametrize("base", [1.001, 1.002])
def test_deep_skewed_bvh_intersections(base, tmp_path, oracle, ptamd):
    """Deep trees (height 43 / 71 against a reference DFS stack of 13 / 12, ~96k nodes): the
    near-first traversal gets a stack of height + 1 (base 1.001), or, when that exceeds the 64
    entries the reference's own stack holds, the reference-order traversal runs (base 1.002).
    No push is dropped: full records bit-exact against the oracle on rays aimed at the triangles."""
    import ctypes
    import refpins as R
    path = _skewed_mesh_scene(tmp_path, base)
    a = oracle.load_scene(path, res=(96, 96))
    b = ptamd.SceneFile(path, res=(96, 96))
    assert len(a.bvh_nodes) > 65535
    rays = R.rays(8192, seed=3, targets=R.scene_targets(b.geoms, b.triangles)).astype(ptamd.PATH)
    tr = ptamd.PathTracer(b)
    got = tr.test_intersect(rays)
    tr.free()
    want = np.zeros(len(rays), oracle.ISECT)
    oracle.lib().or_compute_intersections(ctypes.byref(a.c_struct()), ctypes.byref(oracle.options()),
                                          rays.ctypes.data, len(rays), want.ctypes.data)
    assert (want["t"] > 0).sum() > 4000
    assert R.digest(R.pack(got, R.P_ISECT)) == R.digest(R.pack(want, R.P_ISECT))


def test_bench_two_ranks_pixel_tiles(tmp_path, oracle):
    """`bench.py --gpus 2` (no launcher): the parent starts torch.distributed.run with 2 ranks
    (gloo, sharing this GPU), each traces its interleaved row bands of 2 x (W + K) frames, rank 0
    gathers the tiles; the line reports n_gpus 2 and the image is bit-identical to one GPU's."""
    dump = tmp_path / "img.npy"
    env = dict(os.environ, PT_BENCH_BACKEND="gloo", PT_BENCH_INPROC_DEVICES="0,0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup",
                        "1", "--full", "--no-cpu-baseline", "--no-configs", "--no-api", "--dump-image", str(dump)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["distributed"]["world_size"] == 2
    assert line["scaling"] == "weak" and line["distributed"]["shard"] == "pixels"
    # rank 0's follow-up: the same N as ONE process behind one pathtrace() (here both shards on GPU 0)
    ip = line["inproc"]
    assert ip.get("mode") == "inproc" and ip["n_gpus"] == 2 and ip["devices"] == [0, 0], ip
    assert ip["value"] > 0 and ip["ms_per_step"] > 0 and ip["api_ms_per_frame"] > 0
    a = oracle.load_scene(scene_path("cornell"))
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in range(1, 2 * (1 + 3) + 1):
        r.trace(it)
    got = np.load(dump)
    assert _eq(got, r.image), int(np.sum(got.view(np.uint32) != r.image.view(np.uint32)))


def test_bench_plain_run_is_lean_and_dumps_its_image(tmp_path, oracle):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and reports only the headline
    fields (everything else needs --full); `--dump-outputs DIR` writes the image those W + K frames
    left: with its NaN pixels put back it equals the oracle's bit for bit."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--res", "96x80", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mpaths/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for k in ("roofline", "kernels", "pcie_ms_per_frame", "api", "configs", "cpu_baseline", "inproc"):
        assert k not in line, k
    assert sorted(os.listdir(out)) == ["image.npy", "image_nonfinite.npy"]
    img, code = np.load(out / "image.npy"), np.load(out / "image_nonfinite.npy")
    assert img.dtype == np.float32 and code.dtype == np.float32 and img.shape == code.shape == (96 * 80, 3)
    assert np.isfinite(img).all() and set(np.unique(code)) <= {0.0, 1.0, 2.0, 3.0}
    a = oracle.load_scene(scene_path("cornell"), res=(96, 80))
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in range(1, 2 + 3 + 1):
        r.trace(it)
    want = np.asarray(r.image, np.float32).reshape(-1, 3)
    assert np.array_equal(code == 1, np.isnan(want)) and np.array_equal(code == 2, np.isposinf(want))
    assert np.array_equal(code == 3, np.isneginf(want))
    assert _eq(img[code == 0], want[code == 0])


# ---- GPU BVH build (csrc/pt_bvh_build.hip) == scene.cpp:445-525, bit for bit ----
def _oracle_bvh(oracle, tris):
    n = len(tris)
    nodes = np.zeros(max(1, 2 * n), oracle.BVHNODE)
    idx = np.zeros(max(1, n), np.int32)
    nn = oracle.lib().or_build_bvh(tris.ctypes.data, n, nodes.ctypes.data, idx.ctypes.data) if n else 0
    return nodes[:nn], idx[:n]


def _adversarial_tris(oracle, kind, n, seed):
    """triangles whose build exercises ties, signed zeros, NaN coordinates, equal centroids
    (median fallback) and long swap-partition chains"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, oracle.TRIANGLE)
    if kind == "random":
        p = rng.standard_normal((n, 3, 3)).astype(np.float32)
    elif kind == "grid":          # many equal coordinates and centroids, +-0
        p = (rng.integers(-2, 3, (n, 3, 3)) * 0.5).astype(np.float32)
        p[rng.random((n, 3, 3)) < 0.2] = -0.0
    elif kind == "same":          # identical centroids: every split falls back to the median
        p = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (n, 1, 1))
    elif kind == "nan":           # NaN coordinates (the glm min/max fold resets on them)
        p = rng.standard_normal((n, 3, 3)).astype(np.float32)
        p[rng.random((n, 3, 3)) < 0.05] = np.nan
    else:                         # "alternating": less / not-less alternate along the range
        x = np.where(np.arange(n) % 2 == 0, -1.0, 1.0) * (1 + np.arange(n) / n)
        p = np.zeros((n, 3, 3), np.float32)
        p[:, :, 0] = x[:, None]
        p[:, 1, 1] = 0.01
        p[:, 2, 2] = 0.01
    for k, v in enumerate(("v1", "v2", "v3")):
        t[v]["position"] = p[:, k]
    t["centroid"] = ((p[:, 0] + p[:, 1] + p[:, 2]) / np.float32(3)).astype(np.float32)
    return t


@pytest.mark.parametrize("kind,n", [("random", 1), ("random", 4), ("random", 5), ("random", 37), ("random", 20000),
                                    ("grid", 3000), ("same", 1000), ("nan", 2000), ("alternating", 4097)])
def test_gpu_bvh_build_bitexact(kind, n, oracle, ptamd):
    tris = _adversarial_tris(oracle, kind, n, n)
    want_nodes, want_idx = _oracle_bvh(oracle, tris)
    nodes, idx = ptamd.build_bvh(tris)
    assert len(nodes) == len(want_nodes)
    assert nodes.tobytes() == want_nodes.tobytes()
    assert idx.tobytes() == want_idx.tobytes()


@pytest.mark.parametrize("name", ["cornell_obj_bnnuy", "cornell_obj_khaslana", "cornell_obj_phatphuck"])
def test_scene_gpu_bvh_matches_host_and_reference(name, ptamd):
    """SceneFile(gpu_bvh=True) builds the tree on the GPU: the same nodes / triIndices as the
    host build, hence the reference's (tests/golden/ref_pin.json digests)."""
    import refpins as R
    ref = _REF_PIN["scenes"][name]["sha256"]
    g = ptamd.SceneFile(scene_path(name), viewer_camera=False, gpu_bvh=True)
    assert R.digest(R.pack(g.bvh_nodes, R.P_BVHNODE)) == ref["bvhNodes"]
    assert R.digest(g.tri_indices.astype("<i4")) == ref["triIndices"]


def test_deep_skewed_gpu_bvh(tmp_path, oracle, ptamd):
    path = _skewed_mesh_scene(tmp_path, 1.002, n=60000)
    h = ptamd.SceneFile(path, viewer_camera=False)
    g = ptamd.SceneFile(path, viewer_camera=False, gpu_bvh=True)
    assert g.bvh_nodes.tobytes() == h.bvh_nodes.tobytes() and g.tri_indices.tobytes() == h.tri_indices.tobytes()


def test_bench_four_ranks_config5_shape(tmp_path, oracle):
    """BASELINE configs[4]'s shape (khaslana, depth 12, pixel tiles + tile gather) with 4 ranks
    sharing this GPU (gloo) at 160x160: `bench.py --gpus 4` traces 4 x (W + K) frames over the
    ranks' row bands, rank 0 gathers the tiles; bit-identical to the oracle's frames."""
    dump = tmp_path / "img.npy"
    env = dict(os.environ, PT_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--scene",
                        scene_path("cornell_obj_khaslana"), "--res", "160x160", "--depth", "12", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--no-configs", "--no-api", "--dump-image", str(dump)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 4 and line["distributed"]["world_size"] == 4
    a = oracle.load_scene(scene_path("cornell_obj_khaslana"), res=(160, 160), depth=12)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in range(1, 4 * (1 + 2) + 1):
        r.trace(it)
    got = np.load(dump)
    assert _eq(got, r.image), int(np.sum(got.view(np.uint32) != r.image.view(np.uint32)))


def test_triangle_material_out_of_range_refused(ptamd):
    """A triangle whose materialID names no material is refused at pt_init (PT_E_INVALID), as a
    geom's is: the reference would index past its material array (pathtrace.cu:545)."""
    sc = ptamd.SceneFile(scene_path("cornell_obj_bnnuy"), res=(16, 16), depth=2)
    tris = sc.triangles.copy()
    tris["materialID"][7] = len(sc.materials)
    v = ptamd.scene_view_from_arrays(sc.geoms, sc.materials, sc.camera, 2, tris, sc.tri_indices, sc.bvh_nodes)
    with pytest.raises(ptamd.PtError, match="triangle 7 material"):
        ptamd.PathTracer(v)
    ok = ptamd.PathTracer(ptamd.scene_view_from_arrays(sc.geoms, sc.materials, sc.camera, 2, sc.triangles,
                                                       sc.tri_indices, sc.bvh_nodes))
    ok.trace(1)
    ok.free()
