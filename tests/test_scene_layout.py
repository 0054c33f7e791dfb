"""The device scene layout (host/scene_layout.cpp: pt_scene_view -> the byte images of the device
buffers) through the standalone driver host/ingest_check.cpp, no GPU and nothing loaded into Python.

`make asan` builds the driver twice: build/asan/ingest_check (g++, AddressSanitizer + UBSan) and
build/hostcheck/ingest_check (the library's own host compiler and flags, i.e. the objects that go
into libptamd.so).  `ingest_check layout FILE.json [key=value ...]` prints, per buffer, its element
count and a 64-bit FNV-1a digest of its bytes, then every scalar of the layout, then rc and the
error text.

Byte identity: tests/golden/scene_layout_digests.json holds what pt_init of the commit named in its
"parent" field uploaded for each case below, when the layout was still part of init_one: captured
there by hashing at init_one's upload() call sites and printing the scalars of its SceneDev fill
(a throwaway patch, one pt_init per case with the PT_* environment the keys stand for).  Both driver
builds must reproduce every digest and scalar.

Corrupt trees: `ingest_check layout-mutate FILE.json KIND` corrupts a copy of cornell_obj_bnnuy's BVH
arrays in one way and runs the builder: a layout or an error, never a sanitizer report.  From the
parent's code (init_one, then):
  refused  child_past_end  "BVH node N child out of range"  (the node loop's range check)
           tri_index_end   "triIndices[0] out of range"     (the hot-triangle loop)
           leaf_past_end   "BVH leaf N indexes past triIndices"  (the node loop)
  accepted, on the reference-order traversal (VAR_BVH_FAST | VAR_BVH_SPLIT cleared; pt_init then
  refuses the remaining variant on the fused pipeline, which has no kernels for it, and runs it on
  the staged one -- the runtime's check, after the layout, as before):
           same_child, child_root   bvh_height() = -1 (a node reached twice); the pair walk stops too
           leaf5                    the 5th triangle is outside the leaf's box (bvh_boxes_nested), and
                                    a leaf of more than 4 triangles has no 4-slot group
           unnested, nan_box        bvh_boxes_nested() fails
For unnested and nan_box the parent cleared the bits but still filled a pair layout that no kernel
reads without VAR_BVH_FAST; the builder leaves it empty for a tree whose boxes are not nested, so
`pairs` is empty for every accepted kind.  Layouts of valid input are unchanged (the cases above).
"""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG, scene_path
from test_gpu_parity import _many_geoms_scene, _skewed_mesh_scene

DRIVERS = {"asan": os.path.join(PKG, "build", "asan", "ingest_check"),
           "host": os.path.join(PKG, "build", "hostcheck", "ingest_check")}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0:allocator_may_return_null=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ for the sanitizer build")

VAR_BVH_FAST, VAR_BVH_SPLIT, VAR_BVH_NODES = 16, 32, 64
VAR_DEFAULT = 2 | 8 | 16 | 32 | 128            # pt_default_options

# case -> (scene, LayoutParams keys).  "@geoms33": test_candidate_table_scenes_bitexact's generator
# with n = 33; "@skewed": test_deep_skewed_bvh_intersections's, base 1.002.  The host loader's tree over
# that mesh is 26 levels high (100761 nodes), not past the 64-entry stack: it takes the SAH pair layout
# like any mesh, with more refs than 16 bits hold (ref_shift 15); the too-deep fallback shares its one
# condition with the malformed trees of the corrupt-tree test below.
CASES = {
    "cornell": ("cornell", {}),                                   # no BVH, no table
    "cornell_grid": ("cornell", {"grid": 1}),                     # + candidate table, origin, scale
    "geoms33": ("@geoms33", {}),
    "bnnuy": ("cornell_obj_bnnuy", {}),                           # SAH pairs, 4-wide records, hot4, leaf9
    "bnnuy_tree_ref": ("cornell_obj_bnnuy", {"bvh_tree_ref": 1}),
    "bnnuy_h19_bfs0": ("cornell_obj_bnnuy", {"sah_max_height": 19, "bvh_bfs_levels": 0}),
    "bnnuy_h19_bfs8": ("cornell_obj_bnnuy", {"sah_max_height": 19, "bvh_bfs_levels": 8}),
    "bnnuy_no_quad": ("cornell_obj_bnnuy", {"bvh_quad": 0}),
    "bnnuy_nodes": ("cornell_obj_bnnuy", {"variant": VAR_DEFAULT | VAR_BVH_NODES}),   # pair layout empty
    "bnnuy_naive": ("cornell_obj_bnnuy", {"naive": 1}),
    "skewed": ("@skewed", {}),
}
REFUSED = ("child_past_end", "tri_index_end", "leaf_past_end")
ACCEPTED = ("unnested", "same_child", "child_root", "leaf5", "nan_box")


@pytest.fixture(scope="module")
def drivers():
    subprocess.run(["make", "-C", PKG, "asan"], check=True, capture_output=True, timeout=600)
    return DRIVERS


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "scene_layout_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    made = {}

    def get(name):
        if not name.startswith("@"):
            return scene_path(name)
        if name not in made:
            d = tmp_path_factory.mktemp(name[1:])
            made[name] = (_many_geoms_scene(d / "grid.json", 33) if name == "@geoms33"
                          else _skewed_mesh_scene(d, 1.002))
        return made[name]
    return get


def parse_layout(text):
    """driver output -> {"bufs": {name: [count, digest]}, "scalars": {name: "v ..."}, "rc": n, "err": s}"""
    res = {"bufs": {}, "scalars": {}}
    for line in text.splitlines():
        w = line.split()
        if line.startswith("buf "):
            res["bufs"][w[1]] = [int(w[2]), w[3]]
        elif line.startswith("scalar "):
            res["scalars"][w[1]] = " ".join(w[2:])
        elif line.startswith("rc="):
            res["rc"] = int(w[0][3:])
            res["err"] = line.split(" err=", 1)[1]
    return res


def run_layout(exe, args):
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=ENV)
    out = p.stdout + p.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
    res = parse_layout(p.stdout)
    assert "rc" in res, out[-4000:]
    return res


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_bytes_equal_parent(case, drivers, golden, scenes):
    scene, params = CASES[case]
    want = golden["cases"][case]
    assert want["rc"] == 0 and want["params"] == params
    for build, exe in drivers.items():
        got = run_layout(exe, ["layout", scenes(scene)] + ["%s=%d" % kv for kv in sorted(params.items())])
        assert got["rc"] == 0 and got["err"] == "", (build, got)
        assert got["scalars"] == want["scalars"], (build, got["scalars"], want["scalars"])
        assert got["bufs"] == want["bufs"], (build, got["bufs"], want["bufs"])


def test_cases_cover_the_layout_branches(golden):
    """The recorded layouts are the ones the case list means to pin (counts from the parent)."""
    c = golden["cases"]
    n = lambda case, buf: c[case]["bufs"][buf][0]
    assert n("cornell", "grid") == 0 and n("cornell", "nodes") == 0 and n("cornell_grid", "grid") > 0
    assert n("geoms33", "geoms") == 40 and n("geoms33", "grid") > 0
    assert n("bnnuy", "pairs") > 1 and n("bnnuy", "quads") > 0 and n("bnnuy", "hot4") > 0 and n("bnnuy", "leaf9") > 0
    assert n("bnnuy_tree_ref", "pairs") > 1 and n("bnnuy_tree_ref", "quads") == 0
    assert c["bnnuy_tree_ref"]["bufs"]["pairs"] != c["bnnuy"]["bufs"]["pairs"]
    assert c["bnnuy_h19_bfs0"]["bufs"]["pairs"] != c["bnnuy_h19_bfs8"]["bufs"]["pairs"]
    assert n("bnnuy_no_quad", "quads") == 0 and c["bnnuy_no_quad"]["bufs"]["pairs"] == c["bnnuy"]["bufs"]["pairs"]
    assert n("bnnuy_nodes", "pairs") == 0 and n("bnnuy_nodes", "nodes") == n("bnnuy", "nodes")
    assert n("bnnuy_naive", "naive_hot") > 0 and n("bnnuy_naive", "nodes") == 0 and n("bnnuy_naive", "cold") > 0
    assert n("skewed", "nodes") > 65535 and n("skewed", "pairs") > 1 and c["skewed"]["scalars"]["ref_shift"] == "15"


@pytest.mark.parametrize("kind", REFUSED + ACCEPTED)
def test_corrupt_tree_is_refused_or_falls_back(kind, drivers, golden):
    want = golden["mutations"][kind]
    for build, exe in drivers.items():
        got = run_layout(exe, ["layout-mutate", scene_path("cornell_obj_bnnuy"), kind])
        if kind in REFUSED:
            assert want["rc"] != 0
            assert (got["rc"], got["err"]) == (want["rc"], want["err"]), (build, got)
        else:
            assert want["rc"] == 0 and got["rc"] == 0, (build, got)
            variant = int(got["scalars"]["variant"])
            assert variant == int(want["scalars"]["variant"]) == VAR_DEFAULT & ~(VAR_BVH_FAST | VAR_BVH_SPLIT)
            assert got["bufs"]["pairs"][0] == 0 and got["scalars"]["pair_count"] == "0", (build, got)
            for buf in ("nodes", "node_aux", "hot", "cold"):      # the node-array traversal's buffers: the parent's
                assert got["bufs"][buf] == want["bufs"][buf], (build, buf)
