"""The 8-wide quantised record layout (host/trav_tree.cpp, include/pt/pt_bvh_wide.h) without a GPU:
what `ingest_check wide8 FILE.json OUT` writes, from both drivers `make asan` builds (the sanitized one
and the host-flags one), checked in numpy float32; and the setter's state rules.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO, scene_path
from test_gpu_parity import _skewed_mesh_scene
from test_scene_layout import drivers, run_layout  # noqa: F401  (drivers: the fixture that builds them)

WIDE8 = np.dtype([("origin", "<f4", (3,)), ("exp", "u1", (3,)), ("count", "u1"), ("qlo", "u1", (3, 8)),
                  ("qhi", "u1", (3, 8)), ("ref", "<i4", (8,)), ("cull", "<u4", (8,))])
LEAF8 = np.dtype([("lo", "<f4", (3,)), ("cull", "<u4"), ("hi", "<f4", (3,)), ("count", "<i4"),
                  ("tri", "<f4", (9, 4)), ("spare", "<f4", (4,))])
HOT = np.dtype([("pos", "<f4", (9,)), ("tri", "<i4"), ("pad", "<i4", (2,))])   # DevTriHot: v0 v1 v2 | index


def _dump(exe, scene, out, *args):
    res = run_layout(exe, ["wide8", scene, out] + list(args))
    assert res["rc"] == 0 and res["err"] == "", res
    raw = open(out, "rb").read()
    W, L, stack, height = np.frombuffer(raw, "<i4", 4)
    rec = np.frombuffer(raw, WIDE8, W, 16)
    leaf = np.frombuffer(raw, LEAF8, L if W else 0, 16 + 128 * W)
    hot4 = np.frombuffer(raw, HOT, 4 * L if W else 0, 16 + 128 * W + 192 * L).reshape(-1, 4)
    return res, raw, rec, leaf, hot4, int(stack), int(height)


def _decode(rec, q):
    """origin + float(q) * 2^(exp - 127), the product and the sum in float32 as the kernels form them"""
    scale = (rec["exp"].astype(np.uint32) << 23).view(np.float32)
    return rec["origin"][:, :, None] + q.astype(np.float32) * scale[:, :, None]


@pytest.mark.parametrize("name", ["cornell_obj_bnnuy", "cornell_obj_khaslana", "@skewed"])
def test_record_invariants(name, drivers, tmp_path):
    assert WIDE8.itemsize == 128 and LEAF8.itemsize == 192 and HOT.itemsize == 48
    scene = _skewed_mesh_scene(tmp_path, 1.002, n=30000) if name == "@skewed" else scene_path(name)
    runs = [_dump(exe, scene, str(tmp_path / (b + ".bin"))) for b, exe in sorted(drivers.items())]
    res, raw, rec, leaf, hot4, stack, height = runs[0]
    assert runs[1][1] == raw and runs[1][0] == res                  # both builds: the same bytes
    W, L = len(rec), len(leaf)
    assert W >= 1 and L >= 2 and res["bufs"]["wide8"][0] == W and res["bufs"]["leaf8"][0] == L
    assert res["scalars"]["wide8_stack"] == str(stack) and res["scalars"]["wide8_height"] == str(height)
    used = np.arange(8)[None, :] < rec["count"][:, None]
    assert np.all((rec["ref"] >= 0) == used) and np.all(rec["ref"][~used] == -1) and np.all(rec["count"] >= 2)
    refs = rec["ref"][used]
    assert sorted(refs[refs >= W] - W) == list(range(L))            # every leaf referenced exactly once
    assert sorted(refs[refs < W]) == list(range(1, W))              # every record but the root exactly once
    # a leaf record's box is the min / max of its triangles, bit for bit
    pos = hot4["pos"].reshape(L, 4, 3, 3)
    live = (np.arange(4)[None, :] < leaf["count"][:, None])[:, :, None, None]
    assert np.all((leaf["count"] >= 1) & (leaf["count"] <= 4))
    lo = np.where(live, pos, np.float32(np.inf)).min((1, 2))
    hi = np.where(live, pos, np.float32(-np.inf)).max((1, 2))
    assert lo.tobytes() == leaf["lo"].tobytes() and hi.tobytes() == leaf["hi"].tobytes()
    # decoded child boxes are finite and contain the boxes of all leaves below; stack need; height
    dlo, dhi = _decode(rec, rec["qlo"]), _decode(rec, rec["qhi"])
    assert np.all(np.isfinite(dlo)) and np.all(np.isfinite(dhi))
    ulo, uhi = np.empty((W, 3), np.float32), np.empty((W, 3), np.float32)   # union of the leaves below a record
    need, lev = np.zeros(W, np.int64), np.ones(W, np.int64)
    for w in range(W - 1, -1, -1):                                  # children are numbered after their parent
        n, r = rec["count"][w], rec["ref"][w][:rec["count"][w]]
        assert np.all(r[r < W] > w)
        inner = r < W
        clo = np.where(inner[:, None], ulo[np.where(inner, r, 0)], leaf["lo"][np.where(inner, 0, r - W)])
        chi = np.where(inner[:, None], uhi[np.where(inner, r, 0)], leaf["hi"][np.where(inner, 0, r - W)])
        assert np.all(dlo[w][:, :n].T <= clo) and np.all(dhi[w][:, :n].T >= chi), w
        ulo[w], uhi[w] = clo.min(0), chi.max(0)
        assert np.array_equal(rec["origin"][w], ulo[w])
        flat = ulo[w] == uhi[w]                                     # a zero-extent axis decodes exactly
        assert np.all(dlo[w][flat, :n] == ulo[w][flat, None]) and np.all(dhi[w][flat, :n] == ulo[w][flat, None])
        need[w] = n - 1 + max([need[c] for c in r[inner]], default=0)
        lev[w] = 1 + max([lev[c] for c in r[inner]], default=1)
    assert stack == need[0] + 1 and height == lev[0]
    for a in range(9):                                              # the triangle part is the 4-slot group's
        v = pos[:, :, a // 3, a % 3] - pos[:, :, 0, a % 3] if a >= 3 else pos[:, :, 0, a]
        assert np.array_equal(leaf["tri"][:, a, :], v)


def test_off_by_default_and_below_the_threshold(drivers, tmp_path):
    exe = drivers["asan"]
    scene = scene_path("cornell_obj_bnnuy")
    res = run_layout(exe, ["layout", scene])
    assert not {"wide8", "leaf8"} & set(res["bufs"]) and not {"wide8_stack", "wide8_height"} & set(res["scalars"])
    on = run_layout(exe, ["layout", scene, "bvh_wide_min=1"])
    assert on["bufs"]["wide8"][0] > 0 and {k: v for k, v in on["bufs"].items() if k not in ("wide8", "leaf8")} == res["bufs"]
    refs = res["bufs"]["pairs"][0] + res["bufs"]["leaf9"][0] // 9
    assert len(_dump(exe, scene, str(tmp_path / "a.bin"), "min=%d" % refs)[2]) > 0
    none = _dump(exe, scene, str(tmp_path / "b.bin"), "min=%d" % (refs + 1))
    assert len(none[2]) == 0 and "wide8" not in none[0]["bufs"]
    assert len(_dump(exe, scene, str(tmp_path / "c.bin"), "bvh_tree_ref=1")[2]) == 0   # no SAH tree: inactive


def test_names_setter_state_rules_and_environment(ptamd):
    header = open(os.path.join(REPO, "include", "pt", "pt_bvh_wide.h")).read()
    names = re.findall(r"^int32_t (pt_\w+)\(", header, re.M)
    assert names == ptamd.BVH_WIDE_SYMBOLS and all(hasattr(ptamd.lib, n) for n in names)
    L = ptamd.lib
    L.pt_free()
    prev = ptamd.get_bvh_wide()[:2]
    try:
        ptamd.set_bvh_wide(True)
        assert ptamd.get_bvh_wide() == (True, 65536, False)         # default threshold; no context: inactive
        ptamd.set_bvh_wide(True, 12)
        L.pt_free()
        assert ptamd.get_bvh_wide() == (True, 12, False)            # sticky
        assert L.pt_get_bvh_wide(None, None, None) == 0
        assert ptamd.bvh_wide_info() == dict(num_records=0, height=0, stack_entries=0, leaf_bytes=0)
        ptamd.set_bvh_wide(False, -3)
        assert ptamd.get_bvh_wide() == (False, 65536, False)
    finally:
        ptamd.set_bvh_wide(*prev)
    code = "import sys; sys.path.insert(0, %r); import ptamd; print(*map(int, ptamd.get_bvh_wide()))" % PKG
    for value, want in ((None, "0 65536 0"), ("0", "0 65536 0"), ("1", "1 65536 0"), ("300", "1 300 0")):
        env = {k: v for k, v in os.environ.items() if k != "PT_BVH_WIDE"}
        if value is not None:
            env["PT_BVH_WIDE"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-2000:])
