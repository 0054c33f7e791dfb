"""The denoiser's temporal stage on the GPU (include/pt/pt_denoise_temporal.h) against one numpy
restatement of the header's definition, a function per stage and dtype.  Each stage takes the GPU's
result of the stage before it as input (history planes -> reprojection, base planes -> integration),
so a tap decision on a float threshold in test 1 cannot spoil test 2.  Measured: max |gpu - float64|
is the restatement's float32 floor in every case but two (0.98 of it): at most base colour 2.0e-06,
base moments 5.8e-06, integrated colour 1.7e-07, moments 3.5e-06, filtered image 6.4e-06.
"""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, scene_path
from test_denoise import H5, _synthetic_image, c0_reference

pytestmark = pytest.mark.gpu

PT_E_INVALID, PT_E_STATE, PT_E_UNSUPPORTED = -1, -2, -5
PT_RENDER = os.path.join(REPO, "project3-cuda-path-tracer-2025_amd", "build", "pt_render")
SIZES = [(48, 40), (17, 9)]          # test_denoise.py's: no multiple of the 16 x 16 tile
SAMPLES = 4
TOL_FACTOR = 8.0                     # x the float32 floor of the restatement, as test_denoise.py
DENOISE = dict(sigma_color=0.45, sigma_normal=0.35, sigma_position=0.20)
TEMPORAL = dict(max_history=32, normal_cos_min=0.9, plane_tol=0.02, sigma_variance=4.0)
# camera B relative to A: (translation, pan in radians about `up`)
PAIRS = {"same": ((0, 0, 0), 0.0), "pan": ((0.3, 0.1, -0.2), 0.04), "disocclude": ((3.5, 1.0, -3.0), 0.45), "away": ((0, 0, 0), math.pi)}

def _camera(sc, move):
    cam, yaw = sc.camera.copy(), move[1]
    v, r = cam["view"][0].astype(np.float64), cam["right"][0].astype(np.float64)
    cam["position"][0] += np.float32(move[0])
    cam["view"][0] = math.cos(yaw) * v + math.sin(yaw) * r
    cam["right"][0] = math.cos(yaw) * r - math.sin(yaw) * v
    return cam

_dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
_luma = lambda c, f: _dot(c, np.float32([0.2126, 0.7152, 0.0722]).astype(f))

def reproject(hist, gh, cam, g, tp, f):
    """stage 1 -> (base colour | N_base, base moments, the discrete decisions per pixel)"""
    h, w = g["position"].shape[:2]
    X, n, t = g["position"][..., :3].astype(f), g["normal_t"][..., :3].astype(f), g["normal_t"][..., 3].astype(f)
    v = X - cam["position"][0].astype(f)
    d = _dot(v, cam["view"][0].astype(f)[None, None])
    ok = (g["position"][..., 3] > 0.5) & (d > f(1e-6))
    ds = np.where(ok, d, f(1))
    plx, ply = cam["pixelLength"][0].astype(f)
    u = np.clip((-_dot(v, cam["right"][0].astype(f)[None, None]) / (ds * plx) + f(w) * f(0.5)) - f(0.5), -2, w + 1)
    ww = np.clip((-_dot(v, cam["up"][0].astype(f)[None, None]) / (ds * ply) + f(h) * f(0.5)) - f(0.5), -2, h + 1)
    x0, y0 = np.floor(u), np.floor(ww)
    fx, fy = u - x0, ww - y0
    acc, W, decisions = np.zeros((h, w, 6), f), np.zeros((h, w), f), [ok, np.where(ok, x0, 0), np.where(ok, y0, 0)]
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0.astype(int) + i, y0.astype(int) + j
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
            hc = hist["color"][q].astype(f)
            valid = ok & inside & (gh["position"][q][..., 3] > 0.5) & (gh["albedo_mat"][q][..., 3] == g["albedo_mat"][..., 3]) \
                & (_dot(n, gh["normal_t"][q][..., :3].astype(f)) >= f(np.float32(tp["normal_cos_min"]))) \
                & (np.abs(_dot(gh["position"][q][..., :3].astype(f) - X, n)) <= f(np.float32(tp["plane_tol"])) * t) \
                & np.isfinite(hc[..., :3]).all(-1) & (hc[..., 3] > 0)
            bw = np.where(valid, (fx if i else f(1) - fx) * (fy if j else f(1) - fy), f(0))
            W += bw
            acc += bw[..., None] * np.concatenate([hc, hist["moments"][q][..., :2].astype(f)], -1)
            decisions.append(valid)
    has = W >= f(1e-3)
    decisions.append(has)
    acc = np.where(has[..., None], acc / np.where(has, W, f(1))[..., None], f(0))
    acc[..., 3] = np.minimum(acc[..., 3], f(tp["max_history"]))
    return acc[..., :4], acc[..., 4:], np.stack([np.asarray(x, np.float64) for x in decisions], -1)

def integrate(img, g, bcol, bmom, demod, var_hist_min, f):
    """stage 2 -> (colour | N, (mu1, mu2, variance))"""
    h, w = img.shape[:2]
    with np.errstate(all="ignore"):
        c0 = c0_reference(img, SAMPLES, g, demod, f)
        fin = np.isfinite(c0).all(-1)
        c0 = np.where(fin[..., None], c0, f(0))
        L = _luma(c0, f)
        nb = bcol[..., 3].astype(f)
        a = (f(SAMPLES) / (nb + f(SAMPLES)))[..., None]
        blend = lambda b, c: np.where(fin[..., None], (f(1) - a) * b.astype(f) + a * c, b.astype(f))
        col = np.concatenate([blend(bcol[..., :3], c0), np.where(fin, nb + f(SAMPLES), nb)[..., None]], -1)
        mu1, mu2 = blend(bmom[..., :2], np.stack([L, L * L], -1)).transpose(2, 0, 1)
        mat = np.where(fin, g["albedo_mat"][..., 3], -2).astype(np.int64)       # -2: not usable in a window
        pad = lambda x, v: np.pad(x, 3, constant_values=v)
        Lp, mp = pad(L, 0), pad(mat, -2)
        sl, sl2, cnt = np.zeros((h, w), f), np.zeros((h, w), f), np.zeros((h, w), f)
        for j in range(7):
            for i in range(7):
                on = mp[j:j + h, i:i + w] == g["albedo_mat"][..., 3].astype(np.int64)
                ql = np.where(on, Lp[j:j + h, i:i + w], f(0))
                sl, sl2, cnt = sl + ql, sl2 + ql * ql, cnt + on
        mean = sl / np.maximum(cnt, 1)
        spatial = np.where(cnt > 0, sl2 / np.maximum(cnt, 1) - mean * mean, f(0))
        var = np.maximum(np.where(nb >= f(var_hist_min), mu2 - mu1 * mu1, spatial), f(0))
    return col.astype(f), np.stack([mu1, mu2, var], -1).astype(f)

def levels(col, var, g, levels_, demod, tp, f):
    """stage 3: pt_denoise.h's levels with the variance-normalised colour term"""
    h, w = var.shape
    n, x, hit = g["normal_t"][..., :3].astype(f), g["position"][..., :3].astype(f), g["position"][..., 3] > 0.5
    sn, sp = f(np.float32(DENOISE["sigma_normal"])), f(np.float32(DENOISE["sigma_position"]))
    c, fin = col[..., :3], col[..., 3] > 0.5
    for l in range(levels_):
        sv = f(np.float32(tp["sigma_variance"])) * f(2.0 ** -l)
        kc = f(1) / (sv * sv * (var + f(1e-6)))
        num, den = np.zeros((h, w, 3), f), np.zeros((h, w), f)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ys, xs = np.arange(h) + (j << l), np.arange(w) + (i << l)
                inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                q = (np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :])
                cq = np.where(fin[q][..., None], c[q], f(0))
                e = np.where(fin, ((c - cq) ** 2).sum(-1), f(0)) * kc + np.where(hit, ((n - n[q]) ** 2).sum(-1), f(0)) \
                    / (sn * sn) + np.where(hit, ((x - x[q]) ** 2).sum(-1), f(0)) / (sp * sp)
                wt = np.where(inside & (hit[q] == hit) & fin[q], f(H5[i + 2]) * f(H5[j + 2]) * np.exp(-e), f(0)).astype(f)
                num, den = num + wt[..., None] * cq, den + wt
        c = np.where(den[..., None] != 0, num / np.where(den == 0, f(1), den)[..., None], f(0))
        fin = np.isfinite(c).all(-1)
    if demod:
        c = np.where(hit[..., None], c * np.maximum(g["albedo_mat"][..., :3], np.float32(1e-3)).astype(f), c)
    return c

@functools.lru_cache(maxsize=None)
def _case(size, pair, demod=1, nlevels=5, var_hist_min=0):
    """call under camera A, set_camera(B), capture, second call; restatements in float32 and float64"""
    import ptamd
    w, h = size
    sc = ptamd.SceneFile(scene_path("cornell"), res=size)
    tr = ptamd.PathTracer(sc)
    tp = dict(TEMPORAL, variance_history_min=var_hist_min)
    p = dict(DENOISE, levels=nlevels, demodulate_albedo=demod)
    img_b = _synthetic_image(w, h, SAMPLES)          # gradient + step edge + noise, NaN / inf pixels
    img_a = np.ascontiguousarray(img_b[::-1, ::-1])
    g_a = tr.capture_gbuffer(1)
    tr.set_image(img_a.reshape(-1, 3))
    tr.denoise_temporal(SAMPLES, temporal=tp, **p)
    hist = tr.temporal_planes()
    assert ptamd.lib.pt_set_camera(_camera(sc, PAIRS[pair]).ctypes.data) == 0
    g_b = tr.capture_gbuffer(2)
    tr.set_image(img_b.reshape(-1, 3))
    out = tr.denoise_temporal(SAMPLES, temporal=tp, **p)
    gpu = dict(tr.temporal_planes(), out=out, image_after=tr.image(), image_b=img_b)
    tr.free()
    ref = {}
    for f in (np.float32, np.float64):
        bcol, bmom, dec = reproject(hist, g_a, sc.camera, g_b, tp, f)
        col, mom = integrate(img_b, g_b, gpu["base_color"], gpu["base_moments"], demod, var_hist_min, f)
        ref[f] = dict(base_color=bcol, base_moments=bmom[..., :2], dec=dec, color=col, moments=mom,
                      out=levels(col, mom[..., 2], g_b, nlevels, demod, tp, f))
    keep = (ref[np.float32]["dec"] == ref[np.float64]["dec"]).all(-1)
    assert (~keep).mean() <= 0.02, f"{(~keep).sum()} pixels on a float threshold"
    return gpu, ref, keep, g_b

def _check(gpu, ref, keys, keep, what):
    for k in keys:
        r64, r32 = ref[np.float64][k], ref[np.float32][k].astype(np.float64)
        floor = float(np.abs(r32 - r64)[keep].max())
        err = float(np.abs(gpu[k][..., :r64.shape[-1]].astype(np.float64) - r64)[keep].max())
        print(f"{what} {k}: max |gpu - ref| {err:.3e}, float32 floor {floor:.3e}")
        assert floor < 1e-4 and np.isfinite(gpu[k]).all() and err <= TOL_FACTOR * floor

@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("size", SIZES)
def test_reprojection_matches_definition(size, pair):
    gpu, ref, keep, g_b = _case(size, pair)
    _check(gpu, ref, ("base_color", "base_moments"), keep, f"{size} {pair}")
    nb, hit = gpu["base_color"][..., 3], g_b["position"][..., 3] > 0.5
    assert (nb[~hit] == 0).all() and (gpu["base_color"][nb == 0] == 0).all()
    if pair == "away":
        assert not hit.any()
    elif size == (48, 40):
        assert (nb[hit] > 0).mean() > (0.0 if pair == "disocclude" else 0.9)
        if pair == "disocclude":                              # invalid taps and W < 1e-3 occur
            assert (ref[np.float64]["dec"][..., 3:7].sum(-1) % 4 != 0).any() and (hit & (nb == 0)).any()

@pytest.mark.parametrize("var_hist_min", [0, 1000])           # every pixel temporal / every pixel spatial
@pytest.mark.parametrize("demod", [1, 0])
@pytest.mark.parametrize("nlevels", [1, 5])
@pytest.mark.parametrize("size", SIZES)
def test_integration_variance_and_filter_match_definition(size, nlevels, demod, var_hist_min):
    gpu, ref, keep, _ = _case(size, "pan", demod, nlevels, var_hist_min)
    _check(gpu, ref, ("color", "moments", "out"), np.ones_like(keep), f"{size} levels {nlevels} demod {demod} vhm {var_hist_min}")
    assert gpu["image_after"].tobytes() == gpu["image_b"].reshape(-1, 3).tobytes()   # the image is never written

def test_state_machine(ptamd):
    w, h = 48, 40
    sc = ptamd.SceneFile(scene_path("cornell"), res=(w, h))
    tr = ptamd.PathTracer(sc)
    img = _synthetic_image(w, h, SAMPLES)
    tr.set_image(img.reshape(-1, 3))
    g = tr.capture_gbuffer(1)
    plain = tr.denoise(SAMPLES)
    first = tr.denoise_temporal(SAMPLES)
    pl = tr.temporal_planes()
    c0 = c0_reference(img, SAMPLES, g, 1, np.float32)
    fin = np.isfinite(c0).all(-1)
    assert np.array_equal(pl["color"][fin][:, :3], c0[fin]) and (pl["color"][fin][:, 3] == SAMPLES).all()
    assert (pl["color"][~fin] == 0).all() and (pl["base_color"] == 0).all()           # without history
    assert tr.denoise_temporal(SAMPLES).tobytes() == first.tobytes()                  # nothing is counted twice
    tr.capture_gbuffer(1)
    second = tr.denoise_temporal(SAMPLES)
    n2 = tr.temporal_planes()["color"][..., 3][fin & (g["position"][..., 3] > 0.5)]
    assert n2.max() == 2 * SAMPLES and (n2 == 2 * SAMPLES).mean() > 0.9 and second.tobytes() != first.tobytes()
    assert tr.denoise_temporal(SAMPLES).tobytes() == second.tobytes()
    assert tr.denoise_temporal(SAMPLES, demodulate_albedo=0).tobytes() != second.tobytes()   # drops the history
    assert (tr.temporal_planes()["base_color"] == 0).all()
    tr.temporal_reset()
    tr.capture_gbuffer(1)
    assert tr.denoise_temporal(SAMPLES).tobytes() == first.tobytes()                  # as a first call
    assert tr.image().tobytes() == img.reshape(-1, 3).tobytes()
    assert tr.denoise(SAMPLES).tobytes() == plain.tobytes()                           # pt_denoise is undisturbed
    tr.free()

def test_errors(ptamd):
    L = ptamd.lib
    sc = ptamd.SceneFile(scene_path("cornell"), res=(32, 24))
    tr = ptamd.PathTracer(sc)
    assert L.pt_denoise_temporal(None, None, 1, None, None) == PT_E_STATE                 # nothing captured
    assert L.pt_temporal_get(None, None, None, None, tr.pixels) == PT_E_STATE
    tr.capture_gbuffer(1)
    assert L.pt_denoise_temporal(None, None, 1, None, None) == 0                          # NULL: the defaults
    T = ptamd.temporal_default_params
    for bad in (dict(max_history=0), dict(normal_cos_min=1.5), dict(normal_cos_min=float("nan")), dict(plane_tol=0.0),
                dict(plane_tol=float("inf")), dict(sigma_variance=-1.0), dict(variance_history_min=-1)):
        assert L.pt_denoise_temporal(None, ctypes.byref(T(**bad)), 1, None, None) == PT_E_INVALID, bad
    bad = ptamd.denoise_default_params(levels=9)                                          # pt_denoise's conditions
    assert L.pt_denoise_temporal(ctypes.byref(bad), None, 1, None, None) == PT_E_INVALID
    assert L.pt_denoise_temporal(None, None, 0, None, None) == PT_E_INVALID and L.pt_last_error()
    assert L.pt_set_camera(_camera(sc, PAIRS["pan"]).ctypes.data) == 0                    # moved: the planes are stale
    assert L.pt_denoise_temporal(None, None, 1, None, None) == PT_E_STATE
    tr.free()
    tr = ptamd.PathTracer(sc, devices=[0, 0])
    assert L.pt_denoise_temporal(None, None, 1, None, None) == PT_E_UNSUPPORTED
    assert L.pt_temporal_reset() == PT_E_UNSUPPORTED
    tr.free()

def test_history_lowers_the_error(ptamd):
    sc = ptamd.SceneFile(scene_path("cornell"), res=(64, 64))
    tr = ptamd.PathTracer(sc)
    for k in range(6):                                   # a short arc around the box, 1 spp per camera
        assert ptamd.lib.pt_set_camera(_camera(sc, ((0.25 * (k - 5), 0, 0), 0.02 * (k - 5))).ctypes.data) == 0
        tr.set_image(np.zeros((tr.pixels, 3), np.float32))
        tr.trace_frames(1, 1)
        tr.capture_gbuffer(1)
        temporal = tr.denoise_temporal(1)
    spatial = tr.denoise(1)
    tr.trace_frames(2, 511)
    truth = tr.image().reshape(64, 64, 3) / np.float32(512)
    tr.free()
    ok = np.isfinite(truth).all(-1)
    mse_t, mse_s = (float(((x[ok] - truth[ok]) ** 2).mean()) for x in (temporal, spatial))
    print(f"MSE against 512 spp: denoise {mse_s:.4e}, denoise_temporal {mse_t:.4e}")
    assert mse_t < mse_s

def test_pt_render_events_denoise_temporal(tmp_path):
    (tmp_path / "ev.txt").write_text("frame 2\nkey 83\nbutton 0 1\ncursor 10 0\ncursor 40 5\nbutton 0 0\n"
                                     "frame 2\nkey 83\nframe 1\nkey 256\n")
    base = [PT_RENDER, scene_path("cornell"), "--res", "40x32"]
    r = subprocess.run(base + ["--events", str(tmp_path / "ev.txt"), "--img-dir", str(tmp_path), "--time-tag", "T",
                               "--denoise-temporal", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for n in (2, 2, 3):
        png, den = ((tmp_path / f"cornell.T.{n}samp{e}.png").read_bytes() for e in ("", ".denoised"))
        assert den[:8] == b"\x89PNG\r\n\x1a\n" and den != png
    assert subprocess.run(base + ["--denoise-temporal"], capture_output=True, timeout=60).returncode == 2
