"""Time of the denoiser's kernels (include/pt/pt_denoise.h) on cornell at 800^2 and 1600^2.

    python tools/denoise_probe.py [out.json]        (default profiles/denoise_probe.json)

8 spp are accumulated, then 5 warm-up and 20 timed calls each of pt_gbuffer_capture and of
pt_denoise without the host copy (default parameters: 5 levels), timed by HIP events on the
library's stream (pt_debug_denoise_timing).  Per level the record holds the median time, the
unique bytes of the traffic model (16 B colour read + 32 B guides read + 16 B
written per pixel) and the fraction of 8 TB/s that makes.
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


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "denoise_probe.json")
    rec = {"tool": "tools/denoise_probe.py", "timer": "HIP events on the context's stream, no host copy",
           "runs": [probe(800), probe(1600)]}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
