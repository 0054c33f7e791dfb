"""k_head: the camera bounce and bounce 1 of a primitive-only scene in one launch (PT_HEAD_FUSE).

Every case runs the same calls three times -- the oracle, the library with PT_HEAD_FUSE=0 (two
k_bounce launches, as before) and the library with the fused launch -- and requires the image bit
for bit and stats()["live_total"] for every bounce to be equal at every checkpoint.  Which launch a
tracer took is read from the profiler: a multi-frame pass (no k_tail) has a bounce-1 entry of 0.0
exactly when k_head traced bounce 1 (its duration is in entry 0).

Shapes: 36x20 = 720 pixels = 3 blocks of 256 with the last block and its last wave partial; 720 is
a multiple of neither 64 nor 256, so in a pass of F frames the frame slots change inside a wave and
inside a block.
"""
import json

import numpy as np
import pytest

from conftest import scene_path

BIT = dict(trig_mode=1, arg_order=0)
RES = (36, 20)
pytestmark = pytest.mark.gpu


def _eq(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


class _Oracle:
    """The oracle behind the tracer's calls: image and summed per-bounce live counts."""

    def __init__(self, oracle, scene, **opts):
        self.r = oracle.Renderer(scene, oracle.options(**opts, **BIT))
        self.depth = scene.trace_depth
        self.tot = np.zeros(max(1, self.depth), np.int64)

    def trace(self, it, copy_image=False):
        live = np.maximum(self.r.trace(it), 0)
        self.tot[:len(live)] += live[:len(self.tot)]

    def trace_frames(self, first, count):
        for it in range(first, first + count):
            self.trace(it)

    def prepare_frames(self, count):
        pass

    def snapshot(self):
        return self.r.image.copy(), self.tot.tolist()[:self.depth]


class _Gpu:
    def __init__(self, tr, depth):
        self.tr, self.depth = tr, depth
        self.trace, self.trace_frames, self.prepare_frames = tr.trace, tr.trace_frames, tr.prepare_frames

    def snapshot(self):
        return self.tr.image(), self.tr.stats()["live_total"][:self.depth]


def _took_head(tr, it):
    """a profiled pass of two frames (no k_tail): bounce 1 has no launch of its own"""
    p = tr.profile(it, 2)
    assert p["bounce_ms"][0] > 0.0
    return len(p["bounce_ms"]) > 1 and p["bounce_ms"][1] == 0.0


def _run(calls, target):
    shots = []
    for name, *args in calls:
        kw = args.pop() if args and isinstance(args[-1], dict) else {}
        getattr(target, name)(*args, **kw)
        shots.append(target.snapshot())
    return shots


def _check(oracle, ptamd, monkeypatch, a, b, calls, opts=None, expect_head=True, oracle_opts=None, mask=None,
           last_iteration=100):
    """oracle == PT_HEAD_FUSE=0 == fused at every checkpoint; the fused tracer took k_head iff expected"""
    opts = opts or {}
    want = _run(calls, _Oracle(oracle, a, **(oracle_opts or {})))
    got = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("PT_HEAD_FUSE", fuse)
        tr = ptamd.PathTracer(b, **opts)
        try:
            got[fuse] = _run(calls, _Gpu(tr, a.trace_depth))
            head = _took_head(tr, last_iteration) if opts.get("pipeline", 0) == 0 else False
            assert head == (expect_head and fuse == "1"), (fuse, head)
        finally:
            tr.free()
    for k, (w, g0, g1) in enumerate(zip(want, got["0"], got["1"])):
        wi = w[0] if mask is None else np.where(mask[:, None], w[0], np.float32(0))
        assert _eq(g1[0], g0[0]), (k, int(np.sum(g1[0].view(np.uint32) != g0[0].view(np.uint32))))
        assert _eq(g1[0], wi), (k, int(np.sum(g1[0].view(np.uint32) != wi.view(np.uint32))))
        assert g1[1] == g0[1], (k, g1[1], g0[1])
        if mask is None:
            assert g1[1] == w[1], (k, g1[1], w[1])


def _pair(oracle, ptamd, name, res=RES, depth=None):
    return (oracle.load_scene(scene_path(name), res=res, depth=depth),
            ptamd.SceneFile(scene_path(name), res=res, depth=depth))


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 8])
def test_single_frames_and_passes(depth, oracle, ptamd, monkeypatch):
    """depth 1: no fusion; 2: k_head is the whole pass; 3: k_head meets k_tail (which then starts at
    bounce 2); consecutive single frames, then passes of 2, 3 and 5 frames from prepared graphs"""
    a, b = _pair(oracle, ptamd, "cornell", depth=depth)
    calls = [("trace", 1), ("trace", 2), ("trace", 3), ("prepare_frames", 2), ("trace_frames", 4, 2),
             ("prepare_frames", 3), ("trace_frames", 6, 3), ("prepare_frames", 5), ("trace_frames", 9, 5),
             ("trace", 14)]
    for fpp in (0, 2):   # one pass of F frames; passes of 2 and a remainder
        _check(oracle, ptamd, monkeypatch, a, b, calls, opts={"frames_per_pass": fpp}, expect_head=depth >= 2)


def test_speculated_frames(oracle, ptamd, monkeypatch):
    """single frames that copy the image out: frames 2.. are traced by the speculated-frame graph,
    which takes the fused launch too; equal to the same calls with PT_SPECULATE=0"""
    a, b = _pair(oracle, ptamd, "cornell")
    calls = [("trace", it, {"copy_image": True}) for it in (1, 2, 3, 4, 6, 7)]
    want = _run(calls, _Oracle(oracle, a))
    got = {}
    for fuse, spec in (("0", "1"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("PT_HEAD_FUSE", fuse)
        monkeypatch.setenv("PT_SPECULATE", spec)
        tr = ptamd.PathTracer(b)
        try:
            got[fuse, spec] = _run(calls, _Gpu(tr, a.trace_depth))
            if spec == "1":
                launched, adopted = tr.spec_counts()
                assert adopted == 4 and launched >= adopted, (launched, adopted)   # frames 2, 3, 4 and 7
            assert _took_head(tr, 100) == (fuse == "1")
        finally:
            tr.free()
    for k, w in enumerate(want):
        for key, g in got.items():
            assert _eq(g[k][0], w[0]), (k, key)
            assert g[k][1] == w[1], (k, key, g[k][1], w[1])


def test_glass_scene(oracle, ptamd, monkeypatch):
    """refraction and specular paths through bounce 1 (depth 8, sort off)"""
    a, b = _pair(oracle, ptamd, "cornell_glass_test")
    calls = [("trace", 1), ("trace", 2), ("trace_frames", 3, 3), ("trace", 6)]
    _check(oracle, ptamd, monkeypatch, a, b, calls)


def test_all_camera_rays_miss(tmp_path, oracle, ptamd, monkeypatch):
    """cornell's geometry, the camera turned away from it: every block dies at bounce 0"""
    with open(scene_path("cornell")) as f:
        sc = json.load(f)
    sc["Camera"]["LOOKAT"] = [0.0, 5.0, 30.0]
    path = str(tmp_path / "cornell_all_miss.json")
    with open(path, "w") as f:
        json.dump(sc, f)
    a, b = oracle.load_scene(path, res=RES), ptamd.SceneFile(path, res=RES)
    calls = [("trace", 1), ("trace_frames", 2, 3), ("trace", 5)]
    _check(oracle, ptamd, monkeypatch, a, b, calls)
    monkeypatch.setenv("PT_HEAD_FUSE", "1")
    tr = ptamd.PathTracer(b)
    tr.trace_frames(1, 3)
    st = tr.stats()
    tr.free()
    assert st["live_total"][0] == 3 * RES[0] * RES[1] and st["live_total"][1] == 0, st["live_total"]


@pytest.mark.parametrize("rank", [0, 1])
def test_pixel_shard(rank, oracle, ptamd, monkeypatch):
    """shard_pixel in the fused launch: row bands of 4 of a 36x40 frame, both ranks"""
    from ptamd import dist as D
    w, h = 36, 40
    a, b = _pair(oracle, ptamd, "cornell", res=(w, h))
    rows = np.zeros(h, bool)
    rows[D.owned_rows(h, 4, 2, rank)] = True
    calls = [("trace", 1), ("trace", 2), ("trace_frames", 3, 3)]
    _check(oracle, ptamd, monkeypatch, a, b, calls, mask=np.repeat(rows, w),
           opts={"shard_mode": ptamd.SHARD_PIXELS, "shard_rank": rank, "shard_count": 2, "shard_rows": 4})


@pytest.mark.parametrize("name,res,opts", [
    ("cornell_glass_test", RES, {"material_sort": 1}),       # material grouping
    ("cornell_obj_bnnuy", (32, 32), {}),                     # a mesh scene
    ("cornell", RES, {"pipeline": 1}),                       # the staged pipeline
    ("cornell", RES, {"variant": 10}),                       # another kernel variant
])
def test_other_configurations_keep_their_launches(name, res, opts, oracle, ptamd, monkeypatch):
    a, b = _pair(oracle, ptamd, name, res=res)
    calls = [("trace", 1), ("trace", 2), ("trace_frames", 3, 3)]
    _check(oracle, ptamd, monkeypatch, a, b, calls, opts=opts, expect_head=False,
           oracle_opts={"material_sort": opts.get("material_sort", 0)})
