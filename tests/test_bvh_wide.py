"""The traversal kernels on the 8-wide quantised records (include/pt/pt_bvh_wide.h) against the oracle:
frames and live counts bit for bit, adversarial rays through the kernels per path, and the cases in
which the mode must report inactive and change nothing."""
import numpy as np
import pytest

from conftest import scene_path
from test_fused_bounce import ITERS, assert_honest, expected, grid_of, make_case, run, scenes  # noqa: F401  (scenes: a fixture)
from test_gpu_parity import _skewed_mesh_scene

pytestmark = pytest.mark.gpu
BIT = dict(trig_mode=1, arg_order=0)


def _eq(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.fixture(scope="module")
def skewed(tmp_path_factory):
    return _skewed_mesh_scene(tmp_path_factory.mktemp("wide_skewed"), 1.002, n=30000)


@pytest.mark.parametrize("lds", [None, 2])
@pytest.mark.parametrize("name,res,depth,lanes", [("cornell_obj_bnnuy", (96, 96), None, 40),
                                                   ("cornell_obj_khaslana", (64, 64), 12, 56),
                                                   ("cornell_obj_cyrene", (48, 48), None, 8),
                                                   ("@skewed", (32, 32), None, 32)])
def test_wide_records_bitexact(name, res, depth, lanes, lds, skewed, oracle, ptamd, monkeypatch):
    """Multi-frame passes and API frames, live counts and segments_total included; with PT_BVH_STACK_LDS=2
    the up to seven pushes per record cross into the spill row and through the hand-over."""
    monkeypatch.setenv("PT_BVH_TAIL_LANES", str(lanes))
    if lds is not None:
        monkeypatch.setenv("PT_BVH_STACK_LDS", str(lds))
    path = skewed if name == "@skewed" else scene_path(name)
    a = oracle.load_scene(path, res=res, depth=depth)
    b = ptamd.SceneFile(path, res=res, depth=depth)
    r = oracle.Renderer(a, oracle.options(**BIT))
    tr = ptamd.PathTracer(b, bvh_wide=1)
    try:
        info = ptamd.bvh_wide_info()
        assert ptamd.get_bvh_wide()[2] and info["num_records"] > 0 and info["leaf_bytes"] == 192, info
        assert info["stack_entries"] > 2 and info["height"] >= 2
        segs = 0
        for it in range(1, 5):
            segs += int(np.maximum(r.trace(it), 0).sum())
        tr.trace_frames(1, 4)
        st = tr.stats()
        assert sum(st["queued_total"]) > 0
        assert _eq(tr.image(), r.image), name
        assert st["segments_total"] == segs
        for it in (5, 6):
            live = r.trace(it)
            tr.trace(it, copy_image=True)
            assert tr.stats()["live"][:a.trace_depth] == [int(x) if x >= 0 else 0 for x in live][:a.trace_depth]
        assert _eq(tr.image(), r.image), name
    finally:
        tr.free()
    assert ptamd.get_bvh_wide()[0] is False     # the process-wide setting was put back


@pytest.mark.parametrize("name,n", [("cornell_obj_bnnuy", 6000), ("cornell_obj_cyrene", 2048)])
def test_adversarial_rays_through_the_kernels(name, n, scenes, oracle, ptamd):
    """refpins.rays and _random_paths (NaN / inf / axis-parallel directions, vertex and edge ties) through
    k_bvh_bounce and k_bvh_tail_trav with the mode on, per path against the oracle."""
    a, b = scenes(name)
    tr = ptamd.PathTracer(b, bvh_wide=1)
    try:
        assert ptamd.get_bvh_wide()[2] and tr.bounce_variant()[1]
        c = make_case(oracle, a, name, grid_of(tr, a), n=n)
        for it in ITERS:
            assert_honest(c, expected(c, it), True)
            run(tr, c, it, name + "-wide8")
    finally:
        tr.free()


@pytest.mark.parametrize("kw", [dict(bvh_wide=1, pipeline=1), dict(bvh_wide=1, variant=154),
                                dict(bvh_wide=1, naive_mesh=True), dict(bvh_wide=10 ** 7)],
                         ids=["staged", "no-split", "naive-mesh", "below-min"])
def test_inactive_cases_trace_as_without_the_mode(kw, oracle, ptamd):
    a = oracle.load_scene(scene_path("cornell_obj_bnnuy"), res=(48, 48))
    b = ptamd.SceneFile(scene_path("cornell_obj_bnnuy"), res=(48, 48))
    r = oracle.Renderer(a, oracle.options(**BIT))
    tr = ptamd.PathTracer(b, **kw)
    try:
        assert ptamd.get_bvh_wide()[2] is False
        assert ptamd.bvh_wide_info() == dict(num_records=0, height=0, stack_entries=0, leaf_bytes=0)
        for it in (1, 2):
            r.trace(it)
            tr.trace(it)
        assert _eq(tr.image(), r.image), kw
    finally:
        tr.free()
