"""The hierarchy over the geoms (host/geom_bvh.cpp, include/pt/pt_geom_bvh.h) without a GPU: the node
array `ingest_check geom-bvh FILE.json [min=N] [out=PATH]` writes, from both drivers `make asan` builds
(the sanitized one and the host-flags one), read back with numpy; and the setter's state rules.

Scenes: cornell.json has 7 geoms; `_scene(path, total)` is test_gpu_parity._many_geoms_scene with
total - 7 extras (for 6, cornell without its sphere).  6: a root with leaf and inner children and an
empty slot; 16 / 17: around a full second level; 65 / 72: the default threshold and above; 306: a
larger tree.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from test_gpu_parity import _many_geoms_scene
from test_scene_layout import drivers, run_layout  # noqa: F401  (drivers: the fixture that builds them)

NODE = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("ref", "<i4", (4,)), ("spare", "<f4", (4,))])
TOTALS = [6, 16, 17, 65, 72, 306]


def _scene(path, total, edit=None):
    _many_geoms_scene(path, max(0, total - 7))
    with open(path) as f:
        d = json.load(f)
    if total < 7:
        d["Objects"] = d["Objects"][:total]
    if edit:
        edit(d)
    with open(path, "w") as f:
        json.dump(d, f)
    return str(path)


def _tree(exe, scene, out, *args):
    res = run_layout(exe, ["geom-bvh", scene, "out=%s" % out] + list(args))
    assert res["rc"] == 0 and res["err"] == "", res
    return res, np.fromfile(out, NODE)


@pytest.mark.parametrize("total", TOTALS)
def test_tree_invariants(total, drivers, tmp_path):
    assert NODE.itemsize == 128
    scene = _scene(tmp_path / "s.json", total)
    runs = [_tree(exe, scene, str(tmp_path / ("%s%d.bin" % (b, k)))) for b, exe in sorted(drivers.items()) for k in (0, 1)]
    res, nodes = runs[0]
    for other, raw in runs[1:]:                         # two runs, both builds: the same bytes
        assert raw.tobytes() == nodes.tobytes() and other == res
    assert res["bufs"]["geoms"][0] == total and res["bufs"]["geom_bvh"][0] == len(nodes) >= 1
    valid = nodes["lo"][:, 0, :] <= nodes["hi"][:, 0, :]
    assert np.all(np.isposinf(nodes["lo"].transpose(0, 2, 1)[~valid])) and np.all(np.isneginf(nodes["hi"].transpose(0, 2, 1)[~valid]))
    assert np.all(nodes["ref"][~valid] == -2 ** 31) and np.all(valid.sum(1) >= (2 if total > 1 else 1))
    if total == 6:
        assert not valid.all() and (nodes["ref"][0][valid[0]] < 0).any() and (nodes["ref"][0][valid[0]] >= 0).any()
    refs = nodes["ref"][valid]
    assert sorted(~refs[refs < 0]) == list(range(total))            # every geom in exactly one leaf
    assert sorted(refs[refs >= 0]) == list(range(1, len(nodes)))    # every node but the root has one parent
    height = {0: 1}
    for k in range(len(nodes)):                                     # breadth-first: parents come first
        for c in np.flatnonzero(valid[k] & (nodes["ref"][k] >= 0)):
            ch = nodes["ref"][k][c]
            assert ch > k
            height[ch] = height[k] + 1
            # the slot box is the exact min / max union of the child's slot boxes
            assert np.array_equal(nodes["lo"][ch][:, valid[ch]].min(1), nodes["lo"][k][:, c])
            assert np.array_equal(nodes["hi"][ch][:, valid[ch]].max(1), nodes["hi"][k][:, c])
    h = max(height.values())
    assert res["scalars"]["geom_bvh_height"] == str(h) and res["scalars"]["geom_bvh_stack"] == str(3 * h + 1)
    assert 4 ** h >= total


def test_no_tree_where_the_mode_cannot_apply(drivers, tmp_path):
    """Below the threshold, past the stack budget, and for a geom whose box is not finite (a SCALE that
    overflows the box arithmetic): no tree, no error.  Coincident geoms: the builder ends."""
    exe = drivers["asan"]
    scene = _scene(tmp_path / "s.json", 17)
    for args in (["min=18"], ["geom_bvh_stack_budget=3"]):
        res, nodes = _tree(exe, scene, str(tmp_path / "none.bin"), *args)
        assert len(nodes) == 0 and "geom_bvh" not in res["bufs"] and "geom_bvh_height" not in res["scalars"]
    assert len(_tree(exe, scene, str(tmp_path / "at.bin"), "min=17")[1]) > 0
    huge = _scene(tmp_path / "huge.json", 17, lambda d: d["Objects"][9].update(SCALE=[1e30, 1e30, 1e30]))
    res, nodes = _tree(exe, huge, str(tmp_path / "huge.bin"))
    assert len(nodes) == 0 and "geom_bvh" not in res["bufs"]
    dup = _scene(tmp_path / "dup.json", 7, lambda d: d["Objects"].extend([dict(d["Objects"][3])] * 9))
    res, nodes = _tree(exe, dup, str(tmp_path / "dup.bin"))
    valid = nodes["lo"][:, 0, :] <= nodes["hi"][:, 0, :]
    refs = nodes["ref"][valid]
    assert sorted(~refs[refs < 0]) == list(range(16))


def test_setter_state_rules_and_environment(ptamd):
    L = ptamd.lib
    L.pt_free()
    prev = ptamd.get_geom_bvh()[:2]
    try:
        ptamd.set_geom_bvh(True)
        assert ptamd.get_geom_bvh() == (True, 65, False)            # default threshold; no context: inactive
        ptamd.set_geom_bvh(True, 12)
        L.pt_free()
        assert ptamd.get_geom_bvh() == (True, 12, False)            # sticky
        assert L.pt_get_geom_bvh(None, None, None) == 0 and ptamd.geom_bvh_info() == dict(num_nodes=0, height=0, stack_entries=0)
        ptamd.set_geom_bvh(False, -3)
        assert ptamd.get_geom_bvh() == (False, 65, False)
    finally:
        ptamd.set_geom_bvh(*prev)
    code = "import sys; sys.path.insert(0, %r); import ptamd; print(*map(int, ptamd.get_geom_bvh()))" % PKG
    for value, want in ((None, "0 65 0"), ("0", "0 65 0"), ("1", "1 65 0"), ("300", "1 300 0")):
        env = {k: v for k, v in os.environ.items() if k != "PT_GEOM_BVH"}
        if value is not None:
            env["PT_GEOM_BVH"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-2000:])
