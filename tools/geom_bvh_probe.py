"""Frame time with the hierarchy over the geoms (include/pt/pt_geom_bvh.h) against the flat loop.

    python tools/geom_bvh_probe.py [out.json]        (default profiles/geom_bvh_probe.json)

Scenes: cornell.json (7 geoms) plus n random cubes and spheres inside the room, sized so that they
fill about the same volume at every n, for totals of 72, 300, 1000 and 4000 geoms; 800^2, depth 8;
fused and staged pipelines.  A = mode off (the flat loop of intersect_scene: with the mode off the
kernels are the ones the library had before the mode existed), B = mode on.  The library's state is
process-global, so A and B are timed in one process in the order A B A B ..., each round a fresh
pt_init, the pass graph prepared, WARMUP frames, then FRAMES frames timed with the host clock around
pt_trace_frames + pt_synchronize (the timed window ends in a device synchronise and is tens of
milliseconds at least).  Before timing, the images of A and B after the warm-up are compared bit for
bit.  The record holds, per scene and pipeline, the median over the rounds with min / max for A and B,
the ratio of the medians, the tree's shape, and the staged intersection stage alone (k_intersect
against k_intersect_gbvh, pt_profile_frames' intersect_ms per frame).
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "project3-cuda-path-tracer-2025_amd"))
import ptamd  # noqa: E402

RES, DEPTH = 800, 8
TOTALS = [72, 300, 1000, 4000]
ROUNDS, WARMUP, FRAMES = 5, 2, 64
PIPELINES = {"fused": ptamd.PIPELINE_FUSED, "staged": ptamd.PIPELINE_STAGED}


def write_scene(path, total):
    with open(os.path.join(REPO, "scenes", "cornell.json")) as f:
        d = json.load(f)
    d["Materials"]["mirror"] = {"RGB": [0.9, 0.9, 0.9], "TYPE": "Specular"}
    d["Materials"]["glass"] = {"RGB": [0.95, 0.95, 0.95], "TYPE": "Refractive", "IOR": 1.5}
    mats = ["diffuse_red", "diffuse_green", "diffuse_white", "mirror", "glass"]
    n = total - len(d["Objects"])
    size = 0.9 * (65.0 / n) ** (1.0 / 3.0)
    rng = np.random.default_rng(7)
    for i in range(n):
        d["Objects"].append({"TYPE": "cube" if i % 2 else "sphere", "MATERIAL": mats[i % len(mats)],
                             "TRANS": [float(x) for x in rng.uniform([-4, 0.5, -4], [4, 9, 3])],
                             "ROTAT": [float(x) for x in rng.uniform(0, 90, 3)],
                             "SCALE": [float(x) for x in rng.uniform(0.25 * size, size, 3)]})
    with open(path, "w") as f:
        json.dump(d, f)


def tracer(scene, on, pipeline, fpp):
    tr = ptamd.PathTracer(scene, geom_bvh=on, pipeline=PIPELINES[pipeline], frames_per_pass=fpp)
    assert ptamd.get_geom_bvh()[2] == on
    return tr


def timed(scene, on, pipeline):
    tr = tracer(scene, on, pipeline, FRAMES)
    tr.prepare_frames(FRAMES)
    tr.trace_frames(1, WARMUP)
    tr.synchronize()
    img = tr.image().copy()
    t0 = time.perf_counter()
    tr.trace_frames(1 + WARMUP, FRAMES)
    tr.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / FRAMES
    info = ptamd.geom_bvh_info()
    tr.free()
    return ms, img, info


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "geom_bvh_probe.json")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for total in TOTALS:
            path = os.path.join(tmp, "g%d.json" % total)
            write_scene(path, total)
            scene = ptamd.SceneFile(path, res=(RES, RES), depth=DEPTH)
            for pipeline in PIPELINES:
                t = {False: [], True: []}
                same, info = True, None
                for _ in range(ROUNDS):
                    ms_a, img_a, _ = timed(scene, False, pipeline)     # A B A B ...
                    ms_b, img_b, info = timed(scene, True, pipeline)
                    t[False].append(ms_a)
                    t[True].append(ms_b)
                    same = same and img_a.tobytes() == img_b.tobytes()
                row = {"geoms": int(len(scene.geoms)), "pipeline": pipeline, "images_bit_identical": same, "tree": info}
                for on, key in ((False, "off"), (True, "on")):
                    row[key + "_ms_per_frame"] = statistics.median(t[on])
                    row[key + "_ms_min_max"] = [min(t[on]), max(t[on])]
                row["off_over_on"] = row["off_ms_per_frame"] / row["on_ms_per_frame"]
                if pipeline == "staged":                            # the intersection stage alone
                    for on, key in ((False, "k_intersect_ms_per_frame"), (True, "k_intersect_gbvh_ms_per_frame")):
                        tr = tracer(scene, on, pipeline, 1)
                        tr.trace_frames(1, WARMUP)
                        row[key] = tr.profile(1 + WARMUP, 4)["intersect_ms"]
                        tr.free()
                rows.append(row)
                print(json.dumps(row), flush=True)
    rec = {"tool": "tools/geom_bvh_probe.py", "res": [RES, RES], "depth": DEPTH,
           "timer": "host clock around pt_trace_frames + pt_synchronize, graph prepared, per frame",
           "rounds": ROUNDS, "warmup_frames": WARMUP, "timed_frames": FRAMES, "order": "off, on, off, on, ...",
           "traversal": "immediate form (the parked-leaf form has not been built)", "rows": rows}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
