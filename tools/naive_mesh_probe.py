"""Frame time of the naive mesh mode (include/pt/pt_naive_mesh.h) against the BVH, same scene.

    python tools/naive_mesh_probe.py [out.json]        (default profiles/naive_mesh_probe.json)

Workload: the 5,040-triangle bunny stand-in scene of BASELINE configs[3]
(scenes/cornell_obj_bnnuy.json) at 800^2, depth 8, staged pipeline.  A = naive mode (k_naive_mesh,
no BVH), B = the staged pipeline with the BVH.  The library's state is process-global, so the two
are timed in one process in the order A B A B ..., each round a fresh pt_init, the pass graph
prepared, WARMUP frames, then FRAMES frames timed from the host around pt_trace_frames +
pt_synchronize (the run is far longer than a launch).  The record holds the median over the rounds
and their min / max, the ratio of the medians, the triangle count, and k_naive_mesh's per-bounce
launch times from pt_profile_frames (pt_kernel_times.bvh_ms in this mode).
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "project3-cuda-path-tracer-2025_amd"))
import ptamd  # noqa: E402

SCENE, RES, DEPTH = "cornell_obj_bnnuy", 800, 8
ROUNDS, WARMUP = 5, 2
FRAMES = {"naive": 4, "bvh": 32}          # per timed run: both run for tens of milliseconds at least


def timed(scene, mode):
    n = FRAMES[mode]
    tr = ptamd.PathTracer(scene, naive_mesh=(mode == "naive"), pipeline=ptamd.PIPELINE_STAGED, frames_per_pass=n)
    assert ptamd.get_naive_mesh()[1] == (mode == "naive")
    tr.prepare_frames(n)
    tr.trace_frames(1, WARMUP)
    tr.synchronize()
    t0 = time.perf_counter()
    tr.trace_frames(1 + WARMUP, n)
    tr.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n
    tr.free()
    return ms


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "naive_mesh_probe.json")
    scene = ptamd.SceneFile(os.path.join(REPO, "scenes", SCENE + ".json"), res=(RES, RES), depth=DEPTH)
    times = {"naive": [], "bvh": []}
    for _ in range(ROUNDS):
        for mode in ("naive", "bvh"):       # A B A B ...
            times[mode].append(timed(scene, mode))
    tr = ptamd.PathTracer(scene, naive_mesh=True, frames_per_pass=1)
    tr.trace_frames(1, WARMUP)
    prof = tr.profile(1 + WARMUP, 4)
    tr.free()
    med = {m: statistics.median(v) for m, v in times.items()}
    rec = {
        "tool": "tools/naive_mesh_probe.py", "scene": SCENE, "res": [RES, RES], "depth": DEPTH,
        "pipeline": "staged", "triangles": int(len(scene.triangles)), "tile": ptamd.naive_mesh_tile(),
        "timer": "host clock around pt_trace_frames + pt_synchronize, graph prepared, per frame",
        "rounds": ROUNDS, "warmup_frames": WARMUP, "timed_frames": FRAMES, "order": "naive, bvh, naive, bvh, ...",
        "naive_ms_per_frame": med["naive"], "naive_ms_min_max": [min(times["naive"]), max(times["naive"])],
        "bvh_ms_per_frame": med["bvh"], "bvh_ms_min_max": [min(times["bvh"]), max(times["bvh"])],
        "naive_over_bvh": med["naive"] / med["bvh"],
        "k_naive_mesh_ms_per_bounce": prof["bvh_ms"], "profiled_frame_ms": prof["frame_ms"],
        "profiled_intersect_ms": prof["intersect_ms"], "profiled_shade_ms": prof["shade_ms"],
        "reference_readme_row_ms": {"no_bvh": 732.9, "bvh": 99.4,
                                    "note": "other hardware and the reference's own OBJ, not this stand-in"},
    }
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
