"""The blockwise feature regression on the GPU (include/pt/pt_denoise_regress.h) against one numpy
restatement of the header's definition with the dtype as a parameter: the block table and the output
image against float64, the pass-through pixels, blocks without a sample, determinism, the PBO,
errors, that it denoises, and pt_render --denoise-regress.

Measured on the GPU: see the docstring of test_fit_and_output_match_definition.
"""
import ctypes
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

from conftest import REPO, scene_path
from test_denoise import NAN_INTERIOR, _eq, _synthetic_image, c0_reference

pytestmark = pytest.mark.gpu

PT_E_INVALID, PT_E_STATE, PT_E_UNSUPPORTED = -1, -2, -5
PT_RENDER = os.path.join(REPO, "project3-cuda-path-tracer-2025_amd", "build", "pt_render")
NAN_33x50 = (25, 16)     # the third size's interior NaN pixel (row, column): the image centre, on the back wall -- a surface pixel
SIZES = [(48, 40), (17, 9), (33, 50)]         # (17, 9): every block clipped; (33, 50): a one-pixel block column, three block rows
SAMPLES = 4
RIDGE = 1e-3
TOL_FACTOR = 8.0                               # x the float32 floor of the restatement, as test_denoise.py
# (scene, size, demodulate, through K); the last: guides behind the glass
CASES = [(s, size, d, 0) for s in ("cornell", "cornell_glass_test") for size in SIZES for d in (1, 0)] \
    + [("cornell_glass_test", (48, 40), 1, 4)]


def regress_reference(image, g, emittance, ridge, demod, f):
    """include/pt/pt_denoise_regress.h's definition, every operation in dtype `f`.  image (h, w, 3).
    -> (block table (nby, nbx, 37), output (h, w, 3), surface mask, {(j, i): the block's sample rows F})"""
    h, w = image.shape[:2]
    n, X = g["normal_t"][..., :3].astype(f), g["position"][..., :3].astype(f)
    hit = g["position"][..., 3] > 0.5
    alb = np.maximum(g["albedo_mat"][..., :3], np.float32(1e-3)).astype(f)
    surface = hit & ~(emittance[np.maximum(g["albedo_mat"][..., 3].astype(int), 0)] > 0)
    c = c0_reference(image, SAMPLES, g, demod, f)
    fin = np.isfinite(c).all(-1)
    sample = surface & fin
    nby, nbx = -(-h // 16) + 1, -(-w // 16) + 1
    blocks, num, den, rows = np.zeros((nby, nbx, 37), f), np.zeros((h, w, 3), f), np.zeros((h, w), f), {}
    for j in range(nby):
        for i in range(nbx):
            ys, xs = slice(max(16 * j - 16, 0), min(16 * j + 16, h)), slice(max(16 * i - 16, 0), min(16 * i + 16, w))
            s = sample[ys, xs]
            if not s.any():
                continue                                               # n = 0: no fit
            P = X[ys, xs]
            lo, hi = P[s].min(0), P[s].max(0)
            d = hi - lo
            xh = np.where(d > 0, (P - lo) / np.where(d > 0, d, f(1)), f(0))
            F = np.concatenate([np.ones(s.shape + (1,), f), n[ys, xs], xh, xh * xh], -1)
            Fs, Cs, cnt = F[s], c[ys, xs][s], f(s.sum())
            A = Fs.T @ Fs + np.diag([f(0)] + [f(np.float32(ridge)) * cnt] * 9).astype(f)
            L = np.linalg.cholesky(A)
            beta = np.linalg.solve(L.T, np.linalg.solve(L, Fs.T @ Cs)).astype(f)
            blocks[j, i], rows[j, i] = np.concatenate([[cnt], lo, hi, beta.ravel()]), Fs
            wx = f(1) - np.abs(np.arange(xs.start, xs.stop) - (16 * i - 0.5)).astype(f) / f(16)
            wy = f(1) - np.abs(np.arange(ys.start, ys.stop) - (16 * j - 0.5)).astype(f) / f(16)
            ww = wy[:, None] * wx[None, :]
            num[ys, xs] += ww[..., None] * np.maximum(F @ beta, f(0))
            den[ys, xs] += ww
    out = np.where(den[..., None] > 0, num / np.where(den > 0, den, f(1))[..., None], f(0))
    out = np.where(surface[..., None], out, np.where(fin[..., None], c, f(0)))    # misses and emitters pass through
    if demod:
        out = np.where(hit[..., None], out * alb, out)
    assert out.dtype == f and blocks.dtype == f
    return blocks, out, surface, rows


def _tracer(ptamd, scene, size, through=0, **kw):
    sc = ptamd.SceneFile(scene_path(scene), res=size)
    tr = ptamd.PathTracer(sc, **kw)
    return sc, tr, (tr.capture_gbuffer(1, through=through) if not kw else None)


def _image(w, h):
    """test_denoise.py's synthetic image; its table of interior NaN pixels gets the third size's entry
    for the duration of the call only"""
    with mock.patch.dict(NAN_INTERIOR, {(33, 50): NAN_33x50}):
        return _synthetic_image(w, h, SAMPLES)


def _residual(beta, b64, rows):
    """max over the blocks of |A (beta - beta64)| / n with A = F^T F + ridge n D in float64: the
    coefficients' error as the normal equations see it, per sample -- free of the conditioning of A"""
    worst = 0.0
    for (j, i), Fs in rows.items():
        A = Fs.T @ Fs + np.diag([0.0] + [float(np.float32(RIDGE)) * len(Fs)] * 9)
        d = (beta[j, i, 7:].astype(np.float64) - b64[j, i, 7:]).reshape(10, 3)
        worst = max(worst, float(np.abs(A @ d).max()) / len(Fs))
    return worst


@pytest.fixture(scope="module")
def regress_cases(ptamd):
    """per case: the image and the float64 / float32 restatements on the tracer's own planes --
    shared and never modified -- and the tolerances, 8 x the float32 floor over all cases, each floor
    asserted below 1e-4: one of the image, one of the coefficients' residual (_residual).  The raw
    coefficients cannot meet that bound even in the float32 restatement: the condition number of A
    (~5e3, a flat wall's normal repeats the constant column) enlarges their rounding error along
    directions neither the fitted colour nor the residual depends on.  They are compared too, at
    8 x a floor of their own that is capped at 5e-3."""
    cases, floor, floor_res, floor_beta = {}, 0.0, 0.0, 0.0
    for case in CASES:
        scene, (w, h), demod, through = case
        sc, tr, g = _tracer(ptamd, scene, (w, h), through)
        tr.free()
        img = _image(w, h)
        b64, o64, surface, rows = regress_reference(img, g, sc.materials["emittance"], RIDGE, demod, np.float64)
        b32, o32, _, _ = regress_reference(img, g, sc.materials["emittance"], RIDGE, demod, np.float32)
        assert np.isfinite(o64).all() and surface.any() and (b64[..., 0] > 0).any()
        # a surface pixel with a non-finite colour is filled from the fit (17 x 9: its interior NaN pixel is a miss)
        assert (w, h) == (17, 9) or (surface & ~np.isfinite(img).all(-1)).any()
        assert (w, h) != (33, 50) or surface[NAN_33x50]
        fo, fr, fb = float(np.abs(o32 - o64).max()), _residual(b32, b64, rows), float(np.abs(b32 - b64)[..., 7:].max())
        print(f"{case}: float32 floor image {fo:.3e} residual {fr:.3e} beta {fb:.3e}")
        floor, floor_res, floor_beta = max(floor, fo), max(floor_res, fr), max(floor_beta, fb)
        cases[case] = (img, b64, o64, o32, surface, rows)
    print(f"float32 floors of the restatement: image {floor:.3e}, residual {floor_res:.3e}, beta {floor_beta:.3e}")
    assert 0 < floor < 1e-4 and 0 < floor_res < 1e-4 and 0 < floor_beta < 5e-3
    return cases, TOL_FACTOR * floor, TOL_FACTOR * floor_res, TOL_FACTOR * floor_beta


# ---- 1. fit and output against float64 ------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-demod{c[2]}-K{c[3]}")
def test_fit_and_output_match_definition(case, regress_cases, ptamd):
    """Measured on the GPU, max over the cases against float64 (float32 floor of the restatement,
    tolerance): image 3.0e-05 (6.0e-05, 4.8e-04), residual 2.4e-06 (3.9e-06, 3.1e-05), beta 5.8e-04
    (2.0e-03, 1.6e-02)."""
    cases, tol, tol_res, tol_beta = regress_cases
    scene, (w, h), demod, through = case
    img, b64, o64, o32, surface, rows = cases[case]
    sc, tr, _ = _tracer(ptamd, scene, (w, h), through)
    tr.set_image(img.reshape(-1, 3))
    got = tr.denoise_regress(SAMPLES, ridge=RIDGE, demodulate_albedo=demod)
    blocks = tr.regress_blocks()
    back = tr.image()
    tr.free()
    assert got.shape == (h, w, 3) and blocks.shape == b64.shape
    assert np.isfinite(got).all() and np.isfinite(blocks).all()        # non-finite inputs never reach the output
    assert np.array_equal(blocks[..., :7], b64[..., :7].astype(np.float32))   # n, lo, hi: exact
    eo, er = float(np.abs(got - o64).max()), _residual(blocks, b64, rows)
    eb = float(np.abs(blocks[..., 7:] - b64[..., 7:]).max())
    print(f"{case}: max |gpu - ref| image {eo:.3e} (tolerance {tol:.3e}) residual {er:.3e} ({tol_res:.3e}) "
          f"beta {eb:.3e} ({tol_beta:.3e})")
    assert eo <= tol and er <= tol_res and eb <= tol_beta
    assert (~surface).any() and _eq(got[~surface], o32[~surface])      # misses and emitters: c0, or 0 where it is not finite
    assert back.tobytes() == img.reshape(-1, 3).tobytes()              # the accumulated image is never written


# ---- 2. blocks without a sample ---------------------------------------------------------------------
def test_no_sample_in_any_block(ptamd):
    sc = ptamd.SceneFile(scene_path("cornell"), res=(48, 40))
    tr = ptamd.PathTracer(sc)
    cam = sc.camera.copy()
    cam["view"][0] = -cam["view"][0]                                   # out of the box's open side
    assert ptamd.lib.pt_set_camera(cam.ctypes.data) == 0
    tr.capture_gbuffer(1)
    img = _image(48, 40)
    tr.set_image(img.reshape(-1, 3))
    got = tr.denoise_regress(SAMPLES)
    blocks = tr.regress_blocks()
    tr.free()
    assert blocks.shape == (4, 4, 37) and (blocks == 0).all()          # n = 0 everywhere: no fit
    with np.errstate(all="ignore"):
        c0 = img / np.float32(SAMPLES)
    assert _eq(got, np.where(np.isfinite(c0).all(-1)[..., None], c0, np.float32(0)))


# ---- 3. determinism, PBO ----------------------------------------------------------------------------
def test_deterministic_and_pbo(ptamd):
    sc, tr, _ = _tracer(ptamd, "cornell_glass_test", (48, 40))
    tr.trace_frames(1, 3)
    dev = ctypes.c_void_p()
    assert ptamd.lib.pt_device_alloc(tr.pixels * 4, ctypes.byref(dev)) == 0
    try:
        a = tr.denoise_regress(3, pbo_device_ptr=dev.value)
        pbo = np.zeros((tr.pixels, 4), np.uint8)
        assert ptamd.lib.pt_device_read(pbo.ctypes.data, dev, pbo.size) == 0
    finally:
        ptamd.lib.pt_device_free(dev)
    ta = tr.regress_blocks()
    b = tr.denoise_regress(3)
    tb = tr.regress_blocks()
    assert np.isfinite(tr.denoise_regress(3, ridge=1e-30)).all()       # the pivots keep their lower bound
    tr.free()
    assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes()
    assert pbo.tobytes() == ptamd.image_to_pbo(a.reshape(-1, 3), 1).tobytes()
    assert pbo[:, :3].max() > 0 and (pbo[:, 3] == 0).all()


# ---- 4. errors ----------------------------------------------------------------------------------------
def test_errors(ptamd):
    L, P = ptamd.lib, ptamd.regress_default_params
    sc = ptamd.SceneFile(scene_path("cornell"), res=(32, 24))
    tr = ptamd.PathTracer(sc)
    tr.trace_frames(1, 1)
    out = np.zeros((tr.pixels, 3), np.float32)
    tab = np.zeros((3 * 3, 37), np.float32)
    assert L.pt_denoise_regress(None, 1, None, out.ctypes.data) == PT_E_STATE          # nothing captured
    tr.capture_gbuffer(1)
    assert L.pt_regress_get(tab.ctypes.data, 9) == PT_E_STATE                          # no call yet
    assert L.pt_denoise_regress(None, 1, None, out.ctypes.data) == 0                   # NULL: the defaults
    assert L.pt_regress_get(tab.ctypes.data, 9) == 0 and L.pt_regress_get(tab.ctypes.data, 8) == PT_E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.pt_denoise_regress(ctypes.byref(P(ridge=bad)), 1, None, out.ctypes.data) == PT_E_INVALID, bad
        assert L.pt_last_error()
    assert L.pt_denoise_regress(ctypes.byref(P()), 0, None, out.ctypes.data) == PT_E_INVALID   # samples
    tr.free()
    for kw in (dict(devices=[0, 0]), dict(shard_mode=ptamd.SHARD_PIXELS, shard_rank=0, shard_count=2), dict(naive_mesh=True)):
        sc, tr, _ = _tracer(ptamd, "cornell", (32, 32), **kw)
        assert L.pt_denoise_regress(None, 1, None, out.ctypes.data) == PT_E_UNSUPPORTED, kw
        tr.free()


# ---- 5. it denoises -----------------------------------------------------------------------------------
def test_regression_lowers_the_error(ptamd):
    sc, tr, _ = _tracer(ptamd, "cornell", (64, 64))
    tr.trace_frames(1, 4)
    noisy = tr.image().reshape(64, 64, 3) / np.float32(4)
    reg, atrous = tr.denoise_regress(4), tr.denoise(4)
    tr.trace_frames(5, 508)
    truth = tr.image().reshape(64, 64, 3) / np.float32(512)
    tr.free()
    ok = np.isfinite(truth).all(-1) & np.isfinite(noisy).all(-1)
    mse = [float(((x[ok] - truth[ok]) ** 2).mean()) for x in (noisy, reg, atrous)]
    print(f"MSE against 512 spp: 4 spp {mse[0]:.4e}, regressed {mse[1]:.4e}, a-trous {mse[2]:.4e}")
    assert mse[1] < mse[0]


# ---- 6. pt_render --denoise-regress -------------------------------------------------------------------
def test_pt_render_denoise_regress_writes_both_images(tmp_path):
    base = [PT_RENDER, scene_path("cornell"), "--spp", "3", "--res", "40x32"]
    subprocess.run(base + ["--out", str(tmp_path / "plain")], check=True, capture_output=True, timeout=120)
    r = subprocess.run(base + ["--out", str(tmp_path / "reg"), "--denoise-regress"], check=True, capture_output=True,
                       text=True, timeout=120)
    assert "reg.regressed.png (ridge 0.001)" in r.stdout
    for ext in (".png", ".pfm"):                                       # the ordinary output is unchanged
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("reg" + ext)).read_bytes()
    fitted = (tmp_path / "reg.regressed.png").read_bytes()
    assert fitted[:8] == b"\x89PNG\r\n\x1a\n" and fitted != (tmp_path / "reg.png").read_bytes()
    assert not (tmp_path / "plain.regressed.png").exists()
