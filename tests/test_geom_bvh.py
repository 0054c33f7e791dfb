"""Primitive intersection through the hierarchy over the geoms (include/pt/pt_geom_bvh.h) against the
plain-C oracle, bit for bit (tolerance zero: the wavefront's rule) -- needs an MI355X.

Every test asserts that the mode is really active where it should apply.  Scenes as in
test_geom_bvh_layout (cornell.json has 7 geoms; totals are cornell + extras of
test_gpu_parity._many_geoms_scene).
"""
import json
import os

import numpy as np
import pytest

from conftest import scene_path
from test_geom_bvh_layout import _scene
from test_gpu_parity import BIT, _eq, _oracle_isects, _oracle_pair, _random_paths

pytestmark = pytest.mark.gpu


def _hard_paths(oracle, scene_json, cam):
    """_random_paths (axis-parallel, NaN and tiny directions), camera rays, origins outside the room,
    origins inside geoms, a zero direction, NaN and inf components."""
    with open(scene_json) as f:
        centres = np.array([o["TRANS"] for o in json.load(f)["Objects"]], np.float32)
    inside = _random_paths(len(centres) + 64, 3)[:len(centres)]   # (their first sixteenth: axis-parallel)
    inside["origin"] = centres
    odd = _random_paths(64, 4)[40:48]
    odd["direction"][0] = 0
    odd["direction"][1] = [np.inf, 0, 0]
    odd["direction"][2] = [0.6, -np.inf, 0.8]
    odd["origin"][3] = [np.inf, 1, 1]
    odd["origin"][4] = [np.nan, 1, 1]
    odd["origin"][5] = [-np.inf, -np.inf, -np.inf]
    odd["direction"][6] = [np.nan, 0.6, 0.8]
    return np.concatenate([x.astype(oracle.PATH) for x in
                           (_random_paths(1500, 11), cam, _random_paths(400, 5, box=12.0), inside, odd)])


def _records_equal(oracle, tr, a, paths):
    gpu, ref = tr.test_intersect(paths), _oracle_isects(oracle, a, paths)
    for f in ("t", "surfaceNormal", "materialId"):
        assert _eq(gpu[f], ref[f]), (f, np.where(gpu[f].view(np.uint32) != ref[f].view(np.uint32))[0][:10])
    return ref


@pytest.mark.parametrize("total", [6, 16, 17, 65, 72, 306])
def test_records_bitexact(total, tmp_path, oracle, ptamd):
    path = _scene(tmp_path / "s.json", total)
    a, b = _oracle_pair(oracle, ptamd, path, (96, 96))
    assert len(b.geoms) == total
    tr = ptamd.PathTracer(b, geom_bvh=1)
    info = ptamd.geom_bvh_info()
    assert ptamd.get_geom_bvh()[2] and info["num_nodes"] >= 1 and info["stack_entries"] == 3 * info["height"] + 1
    ref = _records_equal(oracle, tr, a, _hard_paths(oracle, path, tr.test_camera(3)[:1500]))
    assert (ref["t"] > 0).mean() > 0.3
    tr.free()


def test_ties_go_to_the_first_copy(tmp_path, oracle, ptamd):
    """The last objects repeat objects 0..5 with another material: every hit on them carries the first
    copy's material (smallest index among equal t), and the builder ends on coincident boxes."""
    def dup(d):
        d["Objects"] += [dict(o, MATERIAL="mirror") for o in d["Objects"][:6]]
    path = _scene(tmp_path / "s.json", 17, dup)
    a, b = _oracle_pair(oracle, ptamd, path, (96, 96))
    tr = ptamd.PathTracer(b, geom_bvh=1)
    assert ptamd.get_geom_bvh()[2]
    ref = _records_equal(oracle, tr, a, _hard_paths(oracle, path, tr.test_camera(3)[:1500]))
    first = {int(g["materialid"]) for g in b.geoms[:6]}
    on_walls = np.isin(ref["materialId"], list(first)) & (ref["t"] > 0)
    assert on_walls.mean() > 0.3 and int(b.geoms[-1]["materialid"]) not in first
    tr.free()


def _mesh_scene(tmp_path):
    with open(scene_path("cornell_obj_bnnuy")) as f:
        d = json.load(f)
    with open(_scene(tmp_path / "x.json", 7 + 66)) as f:
        x = json.load(f)
    d["Materials"].update(x["Materials"])
    d["Objects"] += x["Objects"][7:]
    for o in d["Objects"]:                               # the OBJ path is relative to the scene's directory
        if "PATH" in o:
            o["PATH"] = "/" + os.path.relpath(os.path.dirname(scene_path("cornell")) + o["PATH"], tmp_path)
    (tmp_path / "mesh.json").write_text(json.dumps(d))
    return str(tmp_path / "mesh.json")


FRAME_OPTS = [{}, {"pipeline": 1}, {"pipeline": 1, "material_sort": 1}, {"stream_compaction": 0, "pipeline": 1}]


@pytest.mark.parametrize("case,mode", [(17, 1), (72, True), ("mesh", True)])
@pytest.mark.parametrize("opts", FRAME_OPTS, ids=["fused", "staged", "staged_sort", "no_compaction"])
def test_frames_bitexact(case, mode, opts, tmp_path, oracle, ptamd):
    """Image and per-bounce live counts over 2 iterations at 48^2, then trace_frames of 4 more.
    (Compaction off exists on the staged pipeline only.)  `mesh`: cornell_obj_bnnuy plus 66 geoms --
    both traversal stacks in one kernel."""
    path = _mesh_scene(tmp_path) if case == "mesh" else _scene(tmp_path / "s.json", case)
    a, b = _oracle_pair(oracle, ptamd, path, (48, 48))
    tr = ptamd.PathTracer(b, geom_bvh=mode, **opts)
    assert ptamd.get_geom_bvh()[2] and len(b.geoms) >= (65 if mode is True else 1)
    r = oracle.Renderer(a, oracle.options(stream_compaction=opts.get("stream_compaction", 1),
                                          material_sort=opts.get("material_sort", 0), **BIT))
    for it in (1, 2):
        live = r.trace(it)
        tr.trace(it)
        if opts.get("stream_compaction", 1):
            assert tr.stats()["live"] == [int(x) if x >= 0 else 0 for x in live]
        assert _eq(tr.image(), r.image), it
    tr.trace_frames(3, 4)
    for it in range(3, 7):
        r.trace(it)
    assert _eq(tr.image(), r.image)
    tr.free()


@pytest.mark.parametrize("total,kw", [(6, dict(geom_bvh=True)), (72, dict(geom_bvh=True, variant=10)), (72, {})])
def test_fallback_is_the_flat_path(total, kw, tmp_path, oracle, ptamd):
    """Too few geoms for the default threshold, a variant without a geom-BVH instantiation, the mode
    off: pt_init succeeds, active is 0, the image is the oracle's; the constructor puts the process
    setting back."""
    ptamd.set_geom_bvh(False)
    path = _scene(tmp_path / "s.json", total)
    a, b = _oracle_pair(oracle, ptamd, path, (48, 48))
    tr = ptamd.PathTracer(b, **kw)
    assert ptamd.get_geom_bvh() == (False, 65, False)    # the setting restored, the live context inactive
    assert ptamd.geom_bvh_info() == dict(num_nodes=0, height=0, stack_entries=0)
    r = oracle.Renderer(a, oracle.options(**BIT))
    for it in (1, 2):
        r.trace(it)
        tr.trace(it)
    assert _eq(tr.image(), r.image)
    tr.free()
    ptamd.set_geom_bvh(True, 9)
    ptamd.PathTracer(b).free()
    assert ptamd.get_geom_bvh()[:2] == (True, 9)
    ptamd.set_geom_bvh(False)
