"""Frame time with the traversal kernels on the 8-wide quantised records (include/pt/pt_bvh_wide.h)
against the 4-wide records they walk otherwise.

    python tools/bvh_wide_probe.py [out.json] [scene ...]     (default profiles/bvh_wide_probe.json)

Scenes: the two trees past the L2 (cornell_obj_cyrene, 262k triangles; cornell_obj_phainon, 1.0M) and the
two L2-resident ones (cornell_obj_bnnuy, cornell_obj_khaslana); 800^2, depth 8, fused pipeline.  A = mode off
(with the mode off the kernels and buffers are the ones the library had before the mode existed), B =
mode on with min_refs = 1, so the small trees are measured too.  The library's state is process-global,
so A and B are timed in one process in the order A B A B ..., each round a fresh pt_init, the pass graph
prepared, WARMUP frames, then FRAMES frames timed with the host clock around pt_trace_frames +
pt_synchronize (the window ends in a device synchronise and is tens of milliseconds at least).  Before
timing, the images of A and B after the warm-up are compared bit for bit.  The record holds, per scene,
the median over the rounds with min / max for A and B, the ratio of the medians, the share of queued
rays handed over to k_bvh_tail_trav, and the layout's shape.
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "project3-cuda-path-tracer-2025_amd"))
import ptamd  # noqa: E402

RES, DEPTH = 800, 8
SCENES = ["cornell_obj_cyrene", "cornell_obj_phainon", "cornell_obj_bnnuy", "cornell_obj_khaslana"]
ROUNDS, WARMUP, FRAMES = 3, 2, 16


def timed(scene, on):
    tr = ptamd.PathTracer(scene, bvh_wide=1 if on else False, frames_per_pass=FRAMES)
    assert ptamd.get_bvh_wide()[2] == on
    info = ptamd.bvh_wide_info()
    tr.prepare_frames(FRAMES)
    tr.trace_frames(1, WARMUP)
    tr.synchronize()
    img = tr.image().copy()
    tr.reset_stats()
    t0 = time.perf_counter()
    tr.trace_frames(1 + WARMUP, FRAMES)
    tr.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / FRAMES
    st = tr.stats()
    tr.free()
    share = sum(st["handed_total"]) / max(1, sum(st["queued_total"]))
    return ms, img, info, share


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "bvh_wide_probe.json")
    rows = []
    for name in sys.argv[2:] or SCENES:
        scene = ptamd.SceneFile(os.path.join(REPO, "scenes", name + ".json"), res=(RES, RES), depth=DEPTH)
        t, share = {False: [], True: []}, {}
        same, info = True, None
        for _ in range(ROUNDS):
            ms_a, img_a, _, share["off"] = timed(scene, False)     # A B A B ...
            ms_b, img_b, info, share["on"] = timed(scene, True)
            t[False].append(ms_a)
            t[True].append(ms_b)
            same = same and img_a.tobytes() == img_b.tobytes()
        row = {"scene": name, "triangles": int(len(scene.triangles)), "images_bit_identical": same, "layout": info,
               "handed_share": share}
        for on, key in ((False, "off"), (True, "on")):
            row[key + "_ms_per_frame"] = statistics.median(t[on])
            row[key + "_ms_min_max"] = [min(t[on]), max(t[on])]
        row["off_over_on"] = row["off_ms_per_frame"] / row["on_ms_per_frame"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bvh_wide_probe.py", "res": [RES, RES], "depth": DEPTH,
           "timer": "host clock around pt_trace_frames + pt_synchronize, graph prepared, per frame",
           "rounds": ROUNDS, "warmup_frames": WARMUP, "timed_frames": FRAMES, "order": "off, on, off, on, ...",
           "off": "the 4-wide records (PT_BVH_QUAD default), as without the mode",
           "rows": rows}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
