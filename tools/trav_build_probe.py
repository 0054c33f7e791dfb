"""Host vs device build of the SAH traversal hierarchy (include/pt/pt_trav_build.h).

1. pt_trav_build on synthetic leaf boxes on a sphere, host against device, over leaf counts from 1 k to
   the 1.0 M-triangle stand-in's (334 k): median of 3, the two interleaved, after one warm-up of each;
   the trees are compared byte for byte.  The device time is the whole call (upload, kernels,
   download, the host's O(n) box fold and numbering); every call ends in a blocking download.
2. Whole pt_init (PathTracer construction, 64^2) with the mode off and on, interleaved, median of 3.

Writes profiles/trav_build_probe.json and prints it.  Needs a GPU.  Tools only.
  python tools/trav_build_probe.py [--skip-init] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "project3-cuda-path-tracer-2025_amd"))

COUNTS = [1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16, 87_000, 1 << 17, 1 << 18, 334_000]
SCENES = ["cornell_obj_bnnuy", "cornell_obj_khaslana", "cornell_obj_cyrene", "cornell_obj_phainon"]


def sphere_leaves(n, seed=1):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    c = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    r = (g.random((n, 3)) * 4.0 / np.sqrt(n)).astype(np.float32)
    return c - r, c + r, g.random(n).astype(np.float32)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    import ptamd
    out_path = os.path.join(REPO, "profiles", "trav_build_probe.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    res = {"build": [], "pt_init": [], "bfs_levels": 12, "max_height": 21}
    for n in COUNTS:
        lo, hi, s = sphere_leaves(n)
        run = {w: (lambda w=w: ptamd.trav_build(lo, hi, s, w, 12, 21)) for w in ("host", "gpu")}
        trees = {w: run[w]() for w in run}      # warm-up, and the identity check
        same = trees["host"][0].tobytes() == trees["gpu"][0].tobytes() and trees["host"][1] == trees["gpu"][1]
        ms = {"host": [], "gpu": []}
        for _ in range(3):
            for w in ("host", "gpu"):
                ms[w].append(timed(run[w])[0])
        res["build"].append({"leaves": n, "host_ms": round(statistics.median(ms["host"]), 2),
                             "device_ms": round(statistics.median(ms["gpu"]), 2), "height": trees["gpu"][1],
                             "identical": bool(same)})
        print(res["build"][-1], flush=True)
    if "--skip-init" not in sys.argv:
        for name in SCENES:
            sc = ptamd.SceneFile(os.path.join(REPO, "scenes", name + ".json"), res=(64, 64))
            ms, active = {False: [], True: []}, False
            for rep in range(4):                # the first round is the warm-up
                for on in (False, True):
                    t, tr = timed(lambda: ptamd.PathTracer(sc, trav_build=2 if on else False))
                    active = active or (on and ptamd.get_trav_build()[2])
                    tr.free()
                    if rep:
                        ms[on].append(t)
            res["pt_init"].append({"scene": name, "triangles": int(len(sc.triangles)),
                                   "host_tree_ms": round(statistics.median(ms[False]), 1),
                                   "device_tree_ms": round(statistics.median(ms[True]), 1), "active": bool(active)})
            print(res["pt_init"][-1], flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
