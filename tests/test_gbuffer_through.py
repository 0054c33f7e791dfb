"""The through-capture on the GPU (include/pt/pt_gbuffer_through.h): the planes of the first
non-specular hit against the oracle's plain C chained from Python (or_generate_ray, then per round
or_compute_intersections and or_scatter), bit for bit; the cap, K = 0, determinism, errors and state.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import SCENES, scene_path

pytestmark = pytest.mark.gpu

PT_E_INVALID, PT_E_STATE, PT_E_UNSUPPORTED = -1, -2, -5
RES = (50, 46)      # 2300 pixels: no multiple of 64 or 256 (the last wave, the queues' partial waves)
PLANES = ("normal_t", "position", "albedo_mat", "followed")


def expected(O, a, it, K):
    """The header's definition on the oracle: the four planes, and per pixel whether the chain missed."""
    L, o, cs, n = O.lib(), O.options(trig_mode=1, arg_order=0), a.c_struct(), a.pixelcount
    cur = np.zeros(n, O.PATH)
    for i in range(n):
        L.or_generate_ray(a.camera.ctypes.data, it, a.trace_depth, i % a.width, i // a.width, ctypes.byref(o),
                          cur[i:].ctypes.data)
    mats = a.materials.copy()
    mats["hasReflective"][mats["hasRefractive"] > 0] = 0            # glass always refracts
    nt, pos, am = (np.zeros((n, 4), np.float32) for _ in range(3))
    nt[:, 3] = am[:, 3] = -1
    followed, missed = np.zeros(n, np.int32), np.zeros(n, bool)
    pix, tsum = np.arange(n), np.zeros(n, np.float32)
    for k in range(K + 1):
        rec = np.zeros(len(cur), O.ISECT)
        L.or_compute_intersections(ctypes.byref(cs), ctypes.byref(o), cur.ctypes.data, len(cur), rec.ctypes.data)
        hit = rec["t"] > 0
        m = a.materials[rec["materialId"]]
        go = hit & (m["emittance"] <= 0) & ((m["hasReflective"] > 0) | (m["hasRefractive"] > 0)) & (k < K)
        tsum = tsum + rec["t"]                                      # float32, in chain order
        x = cur["origin"] + cur["direction"] * rec["t"][:, None]    # multiply, then add, both rounded
        end = hit & ~go
        nt[pix[end]] = np.c_[rec["surfaceNormal"][end], tsum[end]]
        pos[pix[end]] = np.c_[x[end], np.ones(end.sum(), np.float32)]
        am[pix[end]] = np.c_[m["color"][end], rec["materialId"][end].astype(np.float32)]
        followed[pix[~go]], missed[pix[~hit]] = k, True
        for i in np.flatnonzero(go):
            L.or_scatter(ctypes.byref(o), cur[i:].ctypes.data, O.v3(x[i]), O.v3(rec["surfaceNormal"][i]),
                         mats[rec["materialId"][i]:].ctypes.data, it)
        cur, pix, tsum = np.ascontiguousarray(cur[go]), pix[go], tsum[go]
    return dict(zip(PLANES, (nt, pos, am, followed))), missed


def check(got, want):
    for k in PLANES:
        g, w = got[k].reshape(want[k].shape), want[k]
        bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(w), -1).any(1))
        assert len(bad) == 0, (k, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def mirror_wall_mesh_scene(tmp_path):
    """cornell_obj_bnnuy (a glass mesh) with its red wall turned into a mirror"""
    scene = json.load(open(scene_path("cornell_obj_bnnuy")))
    scene["Materials"]["diffuse_red"] = {"RGB": [0.98, 0.98, 0.98], "ROUGHNESS": 0.0, "TYPE": "Reflective"}
    os.symlink(os.path.join(SCENES, "obj"), tmp_path / "obj")
    (tmp_path / "mesh_mirror.json").write_text(json.dumps(scene))
    return str(tmp_path / "mesh_mirror.json")


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("name", ["cornell_glass_test", "cornell_transmissive_test", "cornell_reflective_test", "mesh"])
def test_chain_equals_oracle(name, K, tmp_path, ptamd, oracle):
    path = mirror_wall_mesh_scene(tmp_path) if name == "mesh" else scene_path(name)
    a = oracle.load_scene(path, res=RES)
    tr = ptamd.PathTracer(ptamd.SceneFile(path, res=RES))
    for it in (1, 7):
        want, missed = expected(oracle, a, it, K)
        f = want["followed"]
        assert (f == 0).any() and (f > 0).any() and missed.any(), "the case proves nothing"
        assert K > 1 or (f == K).any()
        check(tr.capture_gbuffer(it, through=K), want)
    tr.free()


def test_cap_k0_and_determinism(tmp_path, ptamd, oracle):
    """Two facing mirrors (the side walls) in a closed box, the camera inside looking at one of them."""
    scene = json.load(open(scene_path("cornell")))
    scene["Camera"].update(EYE=[0.0, 5.0, 0.0], LOOKAT=[-5.0, 5.0, -0.1], FOVY=10.0)
    scene["Objects"] = [ob for ob in scene["Objects"] if ob["TYPE"] != "sphere"]
    scene["Materials"]["mirror"] = {"RGB": [0.9, 0.95, 0.98], "ROUGHNESS": 0.0, "TYPE": "Reflective"}
    walls = {tuple(ob["TRANS"]): ob for ob in scene["Objects"]}
    walls[(-5.0, 5.0, 0.0)]["MATERIAL"] = walls[(5.0, 5.0, 0.0)]["MATERIAL"] = "mirror"
    scene["Objects"].append(dict(walls[(0.0, 5.0, -5.0)], TRANS=[0.0, 5.0, 5.0]))      # the open front, closed
    (tmp_path / "mirrors.json").write_text(json.dumps(scene))
    path = str(tmp_path / "mirrors.json")
    a = oracle.load_scene(path, res=RES)
    sc = ptamd.SceneFile(path, res=RES)
    tr = ptamd.PathTracer(sc)
    mirror = sc.material_names.index("mirror")
    for K in (2, 8):
        want, _ = expected(oracle, a, 3, K)
        capped = (want["followed"] == K) & (want["albedo_mat"][:, 3] == mirror)
        assert capped.sum() > 100
        assert (want["albedo_mat"][capped, :3] == sc.materials["color"][mirror]).all()   # the mirror's own guides
        got = tr.capture_gbuffer(3, through=K)
        check(got, want)
        again = tr.capture_gbuffer(3, through=K)
        assert all(got[k].tobytes() == again[k].tobytes() for k in PLANES)
    first = tr.capture_gbuffer(3)
    assert ptamd.lib.pt_gbuffer_capture_through(3, 0) == 0
    k0 = {k: np.empty_like(first[k]) for k in PLANES[:3]}
    chain = np.full(tr.pixels, -1, np.int32)
    assert ptamd.lib.pt_gbuffer_get(*(k0[k].ctypes.data for k in PLANES[:3]), tr.pixels) == 0
    assert ptamd.lib.pt_gbuffer_get_chain(chain.ctypes.data, tr.pixels) == 0
    tr.free()
    assert all(k0[k].tobytes() == first[k].tobytes() for k in PLANES[:3]) and (chain == 0).all()


def test_errors_and_state(ptamd):
    L = ptamd.lib
    sc = ptamd.SceneFile(scene_path("cornell_glass_test"), res=(32, 24))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 1)
    chain = np.zeros(tr.pixels, np.int32)
    for it, K in ((1, -1), (1, 9), (0, 2)):
        assert L.pt_gbuffer_capture_through(it, K) == PT_E_INVALID and L.pt_last_error(), (it, K)
    tr.capture_gbuffer(1)
    assert L.pt_gbuffer_get_chain(chain.ctypes.data, tr.pixels) == PT_E_STATE      # a first-hit capture has no chain
    assert L.pt_denoise_temporal(None, None, 1, None, None) == 0
    tr.capture_gbuffer(1, through=4)
    assert np.isfinite(tr.denoise(1)).any()                                        # pt_denoise accepts it
    assert L.pt_denoise_temporal(None, None, 1, None, None) == PT_E_UNSUPPORTED    # the temporal stage does not
    assert b"through" in L.pt_last_error()
    assert L.pt_gbuffer_capture_through(1, 0) == 0                                 # K = 0 lifts that
    assert L.pt_denoise_temporal(None, None, 1, None, None) == 0
    tr.capture_gbuffer(1, through=4)
    cam = sc.camera.copy()
    cam["position"][0][1] += 0.25
    assert L.pt_set_camera(cam.ctypes.data) == 0                                   # moved: the planes are stale
    assert L.pt_gbuffer_get_chain(chain.ctypes.data, tr.pixels) == PT_E_STATE
    assert L.pt_denoise(None, 1, None, None) == PT_E_STATE
    tr.free()
    for kw in (dict(devices=[0, 0]), dict(shard_mode=ptamd.SHARD_PIXELS, shard_rank=0, shard_count=2),
               dict(naive_mesh=True, pipeline=ptamd.PIPELINE_STAGED)):
        tr = ptamd.PathTracer(sc, **kw)
        assert L.pt_gbuffer_capture_through(1, 2) == PT_E_UNSUPPORTED, kw
        tr.free()


def test_through_guides_lower_the_error_behind_glass(ptamd):
    """4 spp of cornell_glass_test at 64^2 against 4096 spp of the same tracer, over the pixels whose
    ray followed a specular surface: pt_denoise at its defaults, through-guides (K = 4) against first hits."""
    sc = ptamd.SceneFile(scene_path("cornell_glass_test"), res=(64, 64))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 4)
    tr.capture_gbuffer(1)
    first = tr.denoise(4)
    on = tr.capture_gbuffer(1, through=4)["followed"] > 0
    through = tr.denoise(4)
    tr.trace_frames(5, 4092)
    truth = tr.image().reshape(64, 64, 3) / np.float32(4096)
    tr.free()
    ok = on & np.isfinite(truth).all(-1) & np.isfinite(first).all(-1) & np.isfinite(through).all(-1)
    mse_first, mse_through = (float(((d[ok] - truth[ok]) ** 2).mean()) for d in (first, through))
    print(f"MSE against 4096 spp over {ok.sum()} specular pixels: first-hit guides {mse_first:.4e}, through {mse_through:.4e}")
    assert ok.sum() > 30 and mse_through < mse_first      # the sphere covers ~57 of the 4096 pixels
