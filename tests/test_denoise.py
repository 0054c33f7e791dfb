"""The denoiser on the GPU (include/pt/pt_denoise.h): the first-hit feature buffer against the
production intersection, the a-trous filter against a numpy restatement of its definition, the
PBO output, determinism, non-interference with next-frame speculation, errors, pt_render --denoise.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, scene_path

pytestmark = pytest.mark.gpu

PT_E_INVALID, PT_E_STATE, PT_E_UNSUPPORTED = -1, -2, -5
PT_RENDER = os.path.join(REPO, "project3-cuda-path-tracer-2025_amd", "build", "pt_render")


def _bits(a):
    """float32 bit patterns with every NaN mapped to one pattern"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _eq(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1. feature buffer == the production intersection --------------------------------------------
def _check_gbuffer(tr, materials, it):
    g = tr.capture_gbuffer(it)
    paths = tr.test_camera(it)
    rec = tr.test_intersect(paths)
    n = tr.pixels
    nt, pos, am = (g[k].reshape(n, 4) for k in ("normal_t", "position", "albedo_mat"))
    assert _eq(nt[:, :3], rec["surfaceNormal"]) and _eq(nt[:, 3], rec["t"])
    hit = rec["t"] > 0
    assert np.array_equal(pos[:, 3], hit.astype(np.float32))
    t = rec["t"].astype(np.float32)[:, None]
    prod = paths["direction"].astype(np.float32) * t            # separate multiply ...
    want = paths["origin"].astype(np.float32) + prod            # ... and add, both rounded to float32
    assert _eq(pos[hit, :3], want[hit])
    assert np.array_equal(am[hit, 3], rec["materialId"][hit].astype(np.float32))
    assert _eq(am[hit, :3], materials["color"][rec["materialId"][hit]])
    # the sentinels of a miss
    miss = ~hit
    assert (nt[miss, :3] == 0).all() and (nt[miss, 3] == -1).all()
    assert (pos[miss] == 0).all()
    assert (am[miss, :3] == 0).all() and (am[miss, 3] == -1).all()
    return int(miss.sum()), int(hit.sum())


@pytest.mark.parametrize("name,res", [("cornell", (48, 40)), ("cornell_glass_test", (48, 40)),
                                      ("cornell_obj_bnnuy", (32, 32))])
def test_gbuffer_equals_production_intersection(name, res, ptamd):
    sc = ptamd.SceneFile(scene_path(name), res=res)
    tr = ptamd.PathTracer(sc)
    misses = 0
    for it in (1, 7):
        m, h = _check_gbuffer(tr, sc.materials, it)
        assert h > 0
        misses += m
    tr.free()
    if name == "cornell":
        assert misses > 0          # the open front of the box: rays past the walls' edges


def test_gbuffer_miss_sentinels_camera_turned_away(ptamd):
    """a camera that looks out of the box's open side: (nearly) every pixel is a miss"""
    sc = ptamd.SceneFile(scene_path("cornell"), res=(32, 24))
    tr = ptamd.PathTracer(sc)
    cam = sc.camera.copy()
    cam["view"][0] = -cam["view"][0]
    assert ptamd.lib.pt_set_camera(cam.ctypes.data) == 0
    m, h = _check_gbuffer(tr, sc.materials, 1)
    assert m > tr.pixels // 2
    tr.free()


# ---- 2. textured albedo ---------------------------------------------------------------------------
_CUBE_OBJ = """\
v -1 -1 -1
v 1 -1 -1
v 1 1 -1
v -1 1 -1
v -1 -1 1
v 1 -1 1
v 1 1 1
v -1 1 1
vt 0.05 0.1
vt 0.9 0.15
vt 0.95 0.85
vt 0.1 0.8
vn 0 0 1
vn 0 0 -1
vn 1 0 0
vn -1 0 0
vn 0 1 0
vn 0 -1 0
f 5/1/1 6/2/1 7/3/1
f 5/1/1 7/3/1 8/4/1
f 2/1/2 1/2/2 4/3/2
f 2/1/2 4/3/2 3/4/2
f 6/1/3 2/2/3 3/3/3
f 6/1/3 3/3/3 7/4/3
f 1/1/4 5/2/4 8/3/4
f 1/1/4 8/3/4 4/4/4
f 8/1/5 7/2/5 3/3/5
f 8/1/5 3/3/5 4/4/5
f 1/1/6 2/2/6 6/3/6
f 1/1/6 6/3/6 5/4/6
"""

_TEX_PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "pt/pt_texture.h"
int main(void) {
    int w, h, n;
    if (scanf("%d %d %d", &w, &h, &n) != 3) return 1;
    static uint32_t tex[4096];
    for (int i = 0; i < w * h; ++i) if (scanf("%x", &tex[i]) != 1) return 1;
    for (int i = 0; i < n; ++i) {
        uint32_t ub, vb;
        if (scanf("%x %x", &ub, &vb) != 2) return 1;
        float u, v, out[4];
        memcpy(&u, &ub, 4);
        memcpy(&v, &vb, 4);
        pt_tex2d(tex, w, h, u, v, out);
        uint32_t o[3];
        memcpy(o, out, 12);
        printf("%08x %08x %08x\n", o[0], o[1], o[2]);
    }
    return 0;
}
"""


def test_textured_albedo(tmp_path, ptamd):
    from PIL import Image
    rng = np.random.default_rng(5)
    Image.fromarray(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), "RGBA").save(tmp_path / "tex.png")
    (tmp_path / "cube.obj").write_text(_CUBE_OBJ)
    scene = {
        "Camera": {"APERTURE": 0.0, "DEPTH": 4, "EYE": [0.0, 5.0, 10.5], "FILE": "textured_cube", "FOVY": 45.0,
                   "ITERATIONS": 8, "LOOKAT": [0.0, 5.0, 0.0], "RES": [40, 36], "UP": [0.0, 1.0, 0.0]},
        "Materials": {"white": {"RGB": [0.9, 0.8, 0.7], "TYPE": "Diffuse"},
                      "light": {"EMITTANCE": 5.0, "RGB": [1.0, 1.0, 1.0], "TYPE": "Emitting"},
                      "tex": {"RGB": [0.5, 0.5, 0.5], "TYPE": "Diffuse", "TEXTURE": "tex.png"}},
        "Objects": [
            {"MATERIAL": "light", "ROTAT": [0.0, 0.0, 0.0], "SCALE": [3.0, 0.3, 3.0], "TRANS": [0.0, 10.0, 0.0], "TYPE": "cube"},
            {"MATERIAL": "white", "ROTAT": [0.0, 0.0, 0.0], "SCALE": [10.0, 0.01, 10.0], "TRANS": [0.0, 0.0, 0.0], "TYPE": "cube"},
            {"MATERIAL": "tex", "PATH": "/cube.obj", "ROTAT": [20.0, 30.0, 0.0], "SCALE": [2.0, 2.0, 2.0],
             "TRANS": [0.0, 4.0, 0.0], "TYPE": "obj"}]}
    (tmp_path / "scene.json").write_text(json.dumps(scene))
    sc = ptamd.SceneFile(str(tmp_path / "scene.json"))
    assert len(sc.textures) == 1 and sc.textures[0].shape == (4, 4, 4)
    tr = ptamd.PathTracer(sc)
    g = tr.capture_gbuffer(3)
    rec = tr.test_intersect(tr.test_camera(3))
    tr.free()
    am = g["albedo_mat"].reshape(-1, 4)
    tex_id = sc.material_names.index("tex")
    on = (rec["t"] > 0) & (rec["materialId"] == tex_id)
    assert on.sum() > 50
    assert len(np.unique(rec["uv"][on], axis=0)) > 20           # real interpolated uvs, not one corner
    # expected texels: pt_texture.h itself, compiled for the host, at the record's uv (v flipped
    # as the shader flips it)
    exe = tmp_path / "texprobe"
    (tmp_path / "texprobe.cpp").write_text(_TEX_PROBE)
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-I", os.path.join(REPO, "include"),
                    str(tmp_path / "texprobe.cpp"), "-o", str(exe)], check=True)
    texels = sc.textures[0].reshape(-1, 4).astype(np.uint32)
    packed = texels[:, 0] | texels[:, 1] << 8 | texels[:, 2] << 16 | texels[:, 3] << 24
    u = rec["uv"][on, 0].astype(np.float32)
    v = np.float32(1.0) - rec["uv"][on, 1].astype(np.float32)
    text = "4 4 %d\n%s\n%s\n" % (on.sum(), " ".join("%x" % t for t in packed),
                                 "\n".join("%x %x" % (a, b) for a, b in zip(u.view(np.uint32), v.view(np.uint32))))
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
    want = np.array([int(x, 16) for x in out], np.uint32).reshape(-1, 3)
    assert np.array_equal(am[on, :3].view(np.uint32), want)
    # untextured materials of the same scene keep their colour
    off = (rec["t"] > 0) & (rec["materialId"] != tex_id)
    assert off.any() and _eq(am[off, :3], sc.materials["color"][rec["materialId"][off]])


# ---- 3. the filter against its definition ---------------------------------------------------------
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def atrous_reference(image, samples, g, p, f):
    """include/pt/pt_denoise.h's definition, every operation in dtype `f`.  image (h, w, 3)."""
    h, w = image.shape[:2]
    n = g["normal_t"][..., :3].astype(f)
    x = g["position"][..., :3].astype(f)
    hit = g["position"][..., 3] > 0.5
    alb = np.maximum(g["albedo_mat"][..., :3], np.float32(1e-3)).astype(f)
    sc, sn, sp = (f(np.float32(p[k])) for k in ("sigma_color", "sigma_normal", "sigma_position"))
    with np.errstate(all="ignore"):
        c = image.astype(f) / f(samples)
        if p["demodulate_albedo"]:
            c = np.where(hit[..., None], c / alb, c)
        for l in range(p["levels"]):
            s = 1 << l
            scl = sc * f(2.0 ** -l)
            fin = np.isfinite(c).all(-1)
            num, den = np.zeros((h, w, 3), f), np.zeros((h, w), f)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    ys, xs = np.arange(h) + s * j, np.arange(w) + s * i
                    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                    yc, xc = np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]
                    cq, nq, xq, hq, finq = c[yc, xc], n[yc, xc], x[yc, xc], hit[yc, xc], fin[yc, xc]
                    cq = np.where(finq[..., None], cq, f(0))
                    dc = np.where(fin, ((c - cq) ** 2).sum(-1), f(0))       # non-finite centre: colour term 1
                    dn = np.where(hit, ((n - nq) ** 2).sum(-1), f(0))       # two misses: the terms are 1
                    dx = np.where(hit, ((x - xq) ** 2).sum(-1), f(0))
                    wt = (f(H5[i + 2]) * f(H5[j + 2])) * np.exp(-dc / (scl * scl)) * np.exp(-dn / (sn * sn)) \
                        * np.exp(-dx / (sp * sp))
                    wt = np.where(inside & (hq == hit) & finq, wt, f(0)).astype(f)
                    num += wt[..., None] * cq
                    den += wt
            c = np.where(den[..., None] != 0, num / np.where(den == 0, f(1), den)[..., None], f(0))
        if p["demodulate_albedo"]:
            c = np.where(hit[..., None], c * alb, c)
    assert c.dtype == f
    return c, den


# The NaN pixel with all 24 neighbours in range.  48 x 40: the image centre, on the back wall, whose
# taps are weighted by normal and position.  17 x 9: pixels are ~3 scene units apart there, so
# around any interior HIT pixel every tap's position term is below e^-100: with a non-finite centre
# (no centre tap) the weight sum is ~1e-92 in float64 and underflows to 0 in float32, and the
# definition's two branches (sum / 0) then differ by the number format alone.  The interior pixel
# of that size is therefore one whose neighbourhood is all misses (the terms are 1 there).
NAN_INTERIOR = {(48, 40): (20, 24), (17, 9): (4, 2)}


def _synthetic_image(w, h, samples):
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.15 + 0.5 * xx / w + 0.25 * yy / h                               # smooth gradient
    img = np.stack([base, 0.8 * base + 0.1, 1.0 - base], -1)
    img = img + 0.6 * (xx >= w // 2)[..., None] * np.array([0.2, 0.5, 0.1])   # vertical step edge
    img = img + rng.normal(0, 0.08, (h, w, 3))                               # noise
    img = (np.maximum(img, 0) * samples).astype(np.float32)                  # accumulated, not averaged
    img[NAN_INTERIOR[(w, h)]] = np.nan       # all 24 neighbours in range
    img[0, 0] = np.nan                       # a corner
    img[h // 2 - 1, 3, 1] = np.inf           # one channel only
    img[h - 2, w - 3] = -np.inf
    return img


FILTER_SIZES = [(48, 40), (17, 9)]          # no multiple of the 16 x 16 tile; step 16 passes every border of 17 x 9
FILTER_LEVELS = [1, 2, 5]
FILTER_SAMPLES = 4
# The tolerance is 8 x the float32 floor: the largest |float32 - float64| of the restatement above
# over all of these inputs (both sizes, levels 1 / 2 / 5, demodulation on and off), computed by
# the fixture below.  Measured floor 3.8e-07 (so the tolerance is 3.0e-06); the factor covers the
# kernel's tap-order, reciprocal-sigma and hardware-exp rounding, which the float32 run only
# partly shows (measured on the GPU: 3.9e-07 at most).
TOL_FACTOR = 8.0


@pytest.fixture(scope="module")
def filter_cases(ptamd):
    """per size: the tracer's feature planes (captured once), the image, and the float64 / float32
    restatements for every (levels, demodulate) -- shared and never modified"""
    cases, floor = {}, 0.0
    for (w, h) in FILTER_SIZES:
        sc = ptamd.SceneFile(scene_path("cornell"), res=(w, h))
        tr = ptamd.PathTracer(sc)
        g = tr.capture_gbuffer(1)
        tr.free()
        img = _synthetic_image(w, h, FILTER_SAMPLES)
        for lv in FILTER_LEVELS:
            for demod in (1, 0):
                p = dict(levels=lv, sigma_color=0.45, sigma_normal=0.35, sigma_position=0.20, demodulate_albedo=demod)
                r64, den = atrous_reference(img, FILTER_SAMPLES, g, p, np.float64)
                r32, _ = atrous_reference(img, FILTER_SAMPLES, g, p, np.float32)
                assert np.isfinite(r64).all()
                floor = max(floor, float(np.abs(r32.astype(np.float64) - r64).max()))
                cases[(w, h, lv, demod)] = (img, p, r64, den)
    print(f"float32 floor of the restatement: {floor:.3e}; tolerance {TOL_FACTOR * floor:.3e}")
    assert 0 < floor < 1e-4
    return cases, TOL_FACTOR * floor


@pytest.mark.parametrize("demod", [1, 0])
@pytest.mark.parametrize("levels", FILTER_LEVELS)
@pytest.mark.parametrize("size", FILTER_SIZES)
def test_filter_matches_definition(size, levels, demod, filter_cases, ptamd):
    cases, tol = filter_cases
    w, h = size
    img, p, ref, den = cases[(w, h, levels, demod)]
    sc = ptamd.SceneFile(scene_path("cornell"), res=size)
    tr = ptamd.PathTracer(sc)
    tr.capture_gbuffer(1)
    tr.set_image(img.reshape(-1, 3))
    got = tr.denoise(FILTER_SAMPLES, **p)
    back = tr.image()
    tr.free()
    assert got.shape == (h, w, 3)
    assert np.isfinite(got).all()                       # non-finite inputs never reach the output
    zero = den == 0                                     # (last level) no tap with weight: the definition yields 0
    assert (got[zero] == 0).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{w}x{h} levels {levels} demod {demod}: max |gpu - ref| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert back.tobytes() == img.reshape(-1, 3).tobytes()    # the accumulated image is never written


# ---- 4. PBO ---------------------------------------------------------------------------------------
def test_denoise_pbo(ptamd):
    sc = ptamd.SceneFile(scene_path("cornell"), res=(48, 40))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 3)
    tr.capture_gbuffer(1)
    dev = ctypes.c_void_p()
    assert ptamd.lib.pt_device_alloc(tr.pixels * 4, ctypes.byref(dev)) == 0
    try:
        host = tr.denoise(3, pbo_device_ptr=dev.value)
        pbo = np.zeros((tr.pixels, 4), np.uint8)
        assert ptamd.lib.pt_device_read(pbo.ctypes.data, dev, pbo.size) == 0
    finally:
        ptamd.lib.pt_device_free(dev)
    tr.free()
    assert pbo.tobytes() == ptamd.image_to_pbo(host.reshape(-1, 3), 1).tobytes()
    assert pbo[:, :3].max() > 0 and (pbo[:, 3] == 0).all()


# ---- 5. determinism, non-interference ----------------------------------------------------------------
def test_denoise_deterministic(ptamd):
    sc = ptamd.SceneFile(scene_path("cornell_glass_test"), res=(48, 40))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 2)
    tr.capture_gbuffer(1)
    a = tr.denoise(2)
    b = tr.denoise(2)
    tr.free()
    assert a.tobytes() == b.tobytes()


def test_denoise_leaves_speculated_frames_alone(ptamd, monkeypatch):
    monkeypatch.delenv("PT_SPECULATE", raising=False)
    sc = ptamd.SceneFile(scene_path("cornell"), res=(48, 40))
    tr = ptamd.PathTracer(sc)
    for it in range(1, 5):
        img = tr.trace(it, copy_image=True)
        if it < 4:
            tr.capture_gbuffer(1)
            assert np.isfinite(tr.denoise(it)).any()
    with_denoise = img.copy()
    assert tr.image().tobytes() == with_denoise.tobytes()
    launched, adopted = tr.spec_counts()
    tr.free()
    assert adopted >= 3                       # frames 2..4 were traced ahead and taken over
    t2 = ptamd.PathTracer(sc)
    for it in range(1, 5):
        img = t2.trace(it, copy_image=True)
    plain = img.copy()
    t2.free()
    assert with_denoise.tobytes() == plain.tobytes()


# ---- 6. errors ------------------------------------------------------------------------------------
def test_denoise_errors(ptamd):
    L = ptamd.lib
    sc = ptamd.SceneFile(scene_path("cornell"), res=(32, 24))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 1)
    out = np.zeros((tr.pixels, 3), np.float32)
    P = ptamd.denoise_default_params
    assert L.pt_denoise(ctypes.byref(P()), 1, None, out.ctypes.data) == PT_E_STATE     # nothing captured
    assert L.pt_gbuffer_get(None, None, None, tr.pixels) == PT_E_STATE
    tr.capture_gbuffer(1)
    assert L.pt_denoise(ctypes.byref(P()), 1, None, out.ctypes.data) == 0
    assert L.pt_denoise(None, 1, None, out.ctypes.data) == 0                           # NULL: the defaults
    assert L.pt_set_camera(sc.camera.ctypes.data) == 0                                 # the same camera: kept
    assert L.pt_denoise(ctypes.byref(P()), 1, None, out.ctypes.data) == 0
    for bad in (dict(levels=0), dict(levels=9), dict(sigma_color=0.0), dict(sigma_normal=-1.0),
                dict(sigma_position=float("nan")), dict(sigma_color=float("inf"))):
        assert L.pt_denoise(ctypes.byref(P(**bad)), 1, None, out.ctypes.data) == PT_E_INVALID, bad
        assert L.pt_last_error()
    assert L.pt_denoise(ctypes.byref(P()), 0, None, out.ctypes.data) == PT_E_INVALID   # samples
    assert L.pt_gbuffer_capture(0) == PT_E_INVALID
    tr.capture_gbuffer(1)
    cam = sc.camera.copy()
    cam["position"][0][1] += 0.25
    assert L.pt_set_camera(cam.ctypes.data) == 0                                       # moved: the planes are stale
    assert L.pt_denoise(ctypes.byref(P()), 1, None, out.ctypes.data) == PT_E_STATE
    tr.capture_gbuffer(1)
    assert L.pt_denoise(ctypes.byref(P()), 1, None, out.ctypes.data) == 0
    tr.free()


def test_denoise_unsupported_on_several_shards(ptamd):
    L = ptamd.lib
    sc = ptamd.SceneFile(scene_path("cornell"), res=(32, 32))
    tr = ptamd.PathTracer(sc, devices=[0, 0])           # num_devices = 2, device_ids = {0, 0}
    out = np.zeros((tr.pixels, 3), np.float32)
    assert L.pt_gbuffer_capture(1) == PT_E_UNSUPPORTED
    assert L.pt_gbuffer_get(None, None, None, tr.pixels) == PT_E_UNSUPPORTED
    assert L.pt_denoise(None, 1, None, out.ctypes.data) == PT_E_UNSUPPORTED
    tr.trace(1)
    img = tr.image()
    tr.free()
    t1 = ptamd.PathTracer(sc)
    t1.trace(1)
    assert img.tobytes() == t1.image().tobytes()        # and trace still works afterwards
    t1.free()
    t2 = ptamd.PathTracer(sc, shard_mode=ptamd.SHARD_PIXELS, shard_rank=0, shard_count=2)
    assert L.pt_gbuffer_capture(1) == PT_E_UNSUPPORTED
    t2.free()


# ---- 7. it denoises -------------------------------------------------------------------------------
def test_denoise_lowers_the_error(ptamd):
    sc = ptamd.SceneFile(scene_path("cornell"), res=(64, 64))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 4)
    noisy = tr.image().reshape(64, 64, 3) / np.float32(4)
    tr.capture_gbuffer(1)
    den = tr.denoise(4)
    tr.trace_frames(5, 508)
    truth = tr.image().reshape(64, 64, 3) / np.float32(512)
    tr.free()
    ok = np.isfinite(truth).all(-1) & np.isfinite(noisy).all(-1) & np.isfinite(den).all(-1)
    mse_noisy = float(((noisy[ok] - truth[ok]) ** 2).mean())
    mse_den = float(((den[ok] - truth[ok]) ** 2).mean())
    print(f"MSE against 512 spp: 4 spp {mse_noisy:.4e}, denoised {mse_den:.4e}")
    assert mse_den < mse_noisy


# ---- 9 (GPU half). pt_render --denoise ------------------------------------------------------------------
def test_pt_render_denoise_writes_both_images(tmp_path):
    base = [PT_RENDER, scene_path("cornell"), "--spp", "3", "--res", "40x32"]
    subprocess.run(base + ["--out", str(tmp_path / "plain")], check=True, capture_output=True, timeout=120)
    r = subprocess.run(base + ["--out", str(tmp_path / "den"), "--denoise", "3"], check=True, capture_output=True,
                       text=True, timeout=120)
    assert "den.denoised.png (3 levels)" in r.stdout
    plain, den = (tmp_path / "plain.png").read_bytes(), (tmp_path / "den.png").read_bytes()
    assert plain == den                                                   # the ordinary output is unchanged
    assert (tmp_path / "plain.pfm").read_bytes() == (tmp_path / "den.pfm").read_bytes()
    filtered = (tmp_path / "den.denoised.png").read_bytes()
    assert filtered[:8] == b"\x89PNG\r\n\x1a\n" and filtered != den
    assert not (tmp_path / "plain.denoised.png").exists()
