"""Time of the denoiser's kernels (include/pt/pt_denoise.h) on cornell at 800^2 and 1600^2.

    python tools/denoise_probe.py [out.json]        (default profiles/denoise_probe.json)
    python tools/denoise_probe.py --temporal [out.json]   (default profiles/denoise_temporal_probe.json)
    python tools/denoise_probe.py --through [out.json]    (default profiles/gbuffer_through_probe.json)
    python tools/denoise_probe.py --regress [out.json]    (default profiles/denoise_regress_probe.json)

8 spp are accumulated, then 5 warm-up and 20 timed calls each of pt_gbuffer_capture and of
pt_denoise without the host copy (default parameters: 5 levels), timed by HIP events on the
library's stream (pt_debug_denoise_timing).  Per level the record holds the median time, the
unique bytes of the traffic model (16 B colour read + 32 B guides read + 16 B
written per pixel) and the fraction of 8 TB/s that makes.

--temporal: the temporal stage (include/pt/pt_denoise_temporal.h) at 800^2, 5 levels.  Every
iteration moves the camera (two cameras in turn), captures, and runs pt_denoise_temporal (which
reprojects, the capture being new) and pt_denoise on the same image, interleaved in one process;
the record holds the medians of reprojection, integration + variance and the levels, and
pt_denoise's time beside them.

--through: the through-capture (include/pt/pt_gbuffer_through.h) at 800^2 on cornell (no delta
surface) and cornell_glass_test: every iteration times pt_gbuffer_capture and
pt_gbuffer_capture_through with K = 0 and K = 4 in turn, interleaved in one process; the record holds
the medians, and the pixels that followed 1..4 delta surfaces.

--regress: the feature regression (include/pt/pt_denoise_regress.h) at 800^2 on cornell and
cornell_glass_test, default parameters: every iteration runs pt_denoise_regress and pt_denoise on the
same image and capture, interleaved in one process; the record holds the medians of k_regress_fit,
k_regress_apply and pt_denoise's five levels.
"""
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "project3-cuda-path-tracer-2025_amd"))
import ptamd  # noqa: E402

WARMUP, CALLS, SPP = 5, 20, 8
BYTES_PER_PIXEL_LEVEL = 16 + 32 + 16
HBM_BYTES_PER_S = 8e12


def probe(res):
    sc = ptamd.SceneFile(os.path.join(REPO, "scenes", "cornell.json"), res=(res, res))
    tr = ptamd.PathTracer(sc)
    L = ptamd.lib
    tr.trace_frames(1, SPP)
    tr.synchronize()
    p = ptamd.denoise_default_params()
    assert L.pt_debug_denoise_timing(1) == 0
    cap, den, lev = [], [], []
    c, d, lv = ctypes.c_float(), ctypes.c_float(), (ctypes.c_float * 8)()
    for k in range(WARMUP + CALLS):
        assert L.pt_gbuffer_capture(1) == 0, L.pt_last_error()
        assert L.pt_denoise(ctypes.byref(p), SPP, None, None) == 0, L.pt_last_error()
        assert L.pt_debug_denoise_times(ctypes.byref(c), ctypes.byref(d), lv) == 0
        if k >= WARMUP:
            cap.append(c.value)
            den.append(d.value)
            lev.append([lv[i] for i in range(p.levels)])
    L.pt_debug_denoise_timing(0)
    tr.free()
    med = statistics.median
    level_ms = [med([r[i] for r in lev]) for i in range(p.levels)]
    nbytes = BYTES_PER_PIXEL_LEVEL * res * res
    return {
        "scene": "cornell", "res": [res, res], "spp": SPP, "levels": p.levels, "warmup": WARMUP, "calls": CALLS,
        "capture_ms": med(cap), "capture_ms_min_max": [min(cap), max(cap)],
        "denoise_ms": med(den), "denoise_ms_min_max": [min(den), max(den)],
        "level_ms": level_ms,
        "level_kernel": ["k_atrous_lds<1>", "k_atrous_lds<2>"] + ["k_atrous_direct"] * (p.levels - 2),
        "level_unique_bytes": nbytes,
        "level_fraction_of_8TBps": [nbytes / (ms * 1e-3) / HBM_BYTES_PER_S if ms > 0 else None for ms in level_ms],
    }


def probe_temporal(res):
    sc = ptamd.SceneFile(os.path.join(REPO, "scenes", "cornell.json"), res=(res, res))
    tr = ptamd.PathTracer(sc)
    L = ptamd.lib
    tr.trace_frames(1, SPP)
    tr.synchronize()
    cams = [sc.camera.copy(), sc.camera.copy()]
    cams[1]["position"][0][0] += 0.25
    p = ptamd.denoise_default_params()
    assert L.pt_debug_denoise_timing(1) == 0
    rows = []
    r, i, lv, d = (ctypes.c_float() for _ in range(4))
    for k in range(WARMUP + CALLS):
        assert L.pt_set_camera(cams[k & 1].ctypes.data) == 0
        assert L.pt_gbuffer_capture(1) == 0, L.pt_last_error()
        assert L.pt_denoise_temporal(ctypes.byref(p), None, SPP, None, None) == 0, L.pt_last_error()
        assert L.pt_debug_temporal_times(ctypes.byref(r), ctypes.byref(i), ctypes.byref(lv)) == 0
        assert L.pt_denoise(ctypes.byref(p), SPP, None, None) == 0, L.pt_last_error()
        assert L.pt_debug_denoise_times(None, ctypes.byref(d), None) == 0
        if k >= WARMUP:
            rows.append((r.value, i.value, lv.value, d.value))
    L.pt_debug_denoise_timing(0)
    tr.free()
    med = [statistics.median(c) for c in zip(*rows)]
    return {"scene": "cornell", "res": [res, res], "spp": SPP, "levels": p.levels, "warmup": WARMUP, "calls": CALLS,
            "reproject_ms": med[0], "integrate_variance_ms": med[1], "levels_ms": med[2],
            "temporal_total_ms": med[0] + med[1] + med[2], "pt_denoise_ms": med[3],
            "min_max": [[min(c), max(c)] for c in zip(*rows)]}


def probe_through(scene, res):
    sc = ptamd.SceneFile(os.path.join(REPO, "scenes", scene + ".json"), res=(res, res))
    tr = ptamd.PathTracer(sc)
    L = ptamd.lib
    followed = tr.capture_gbuffer(1, through=4)["followed"]
    assert L.pt_debug_denoise_timing(1) == 0
    calls = {"pt_gbuffer_capture": lambda: L.pt_gbuffer_capture(1),
             "through_K0": lambda: L.pt_gbuffer_capture_through(1, 0),
             "through_K4": lambda: L.pt_gbuffer_capture_through(1, 4)}
    rows = {k: [] for k in calls}
    c = ctypes.c_float()
    for k in range(WARMUP + CALLS):
        for name, call in calls.items():
            assert call() == 0, L.pt_last_error()
            assert L.pt_debug_denoise_times(ctypes.byref(c), None, None) == 0
            if k >= WARMUP:
                rows[name].append(c.value)
    L.pt_debug_denoise_timing(0)
    tr.free()
    return {"scene": scene, "res": [res, res], "warmup": WARMUP, "calls": CALLS,
            "pixels_by_followed": [int((followed == k).sum()) for k in range(5)],
            "capture_ms": {k: statistics.median(v) for k, v in rows.items()},
            "capture_ms_min_max": {k: [min(v), max(v)] for k, v in rows.items()}}


def probe_regress(scene, res):
    sc = ptamd.SceneFile(os.path.join(REPO, "scenes", scene + ".json"), res=(res, res))
    tr = ptamd.PathTracer(sc)
    L = ptamd.lib
    tr.trace_frames(1, SPP)
    tr.synchronize()
    tr.capture_gbuffer(1)
    assert L.pt_debug_denoise_timing(1) == 0
    rows = []
    fit, app, d = (ctypes.c_float() for _ in range(3))
    for k in range(WARMUP + CALLS):
        assert L.pt_denoise_regress(None, SPP, None, None) == 0, L.pt_last_error()
        assert L.pt_debug_regress_times(ctypes.byref(fit), ctypes.byref(app)) == 0
        assert L.pt_denoise(None, SPP, None, None) == 0, L.pt_last_error()
        assert L.pt_debug_denoise_times(None, ctypes.byref(d), None) == 0
        if k >= WARMUP:
            rows.append((fit.value, app.value, fit.value + app.value, d.value))
    L.pt_debug_denoise_timing(0)
    blocks = tr.regress_blocks()
    tr.free()
    med = [statistics.median(c) for c in zip(*rows)]
    return {"scene": scene, "res": [res, res], "spp": SPP, "warmup": WARMUP, "calls": CALLS,
            "blocks": [blocks.shape[1], blocks.shape[0]], "blocks_with_fit": int((blocks[..., 0] > 0).sum()),
            "fit_ms": med[0], "apply_ms": med[1], "regress_total_ms": med[2], "pt_denoise_ms": med[3],
            "min_max": [[min(c), max(c)] for c in zip(*rows)]}


def main():
    modes = {"--temporal": "denoise_temporal_probe.json", "--through": "gbuffer_through_probe.json",
             "--regress": "denoise_regress_probe.json"}
    args = [a for a in sys.argv[1:] if a not in modes]
    mode = next((a for a in sys.argv[1:] if a in modes), "")
    out = args[0] if args else os.path.join(REPO, "profiles", modes.get(mode, "denoise_probe.json"))
    runs = {"--temporal": lambda: [probe_temporal(800)],
            "--through": lambda: [probe_through("cornell", 800), probe_through("cornell_glass_test", 800)],
            "--regress": lambda: [probe_regress("cornell", 800), probe_regress("cornell_glass_test", 800)],
            "": lambda: [probe(800), probe(1600)]}[mode]()
    rec = {"tool": ("tools/denoise_probe.py " + mode).strip(),
           "timer": "HIP events on the context's stream, no host copy",
           "runs": runs}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
