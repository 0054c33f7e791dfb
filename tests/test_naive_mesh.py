"""The reference's NAIVE_MESH_LOADING mode (include/pt/pt_naive_mesh.h, k_naive_mesh).

The reference in every comparison is the UNCHANGED oracle on a one-leaf tree: one root node with
start 0, triCount N, identity triIndices and the mesh bounds padded by 1e3 scene units, run with
bvh = 1 and trig_mode = 1.  bvhMeshIntersectionTest on that tree tests every triangle in array
order with the strict `<` of the naive loop, so it is that loop.  The GPU gets the same triangles,
the mode on and no BVH arrays.  Records (52 bytes) and images are compared bit for bit, NaN lanes
by their mask.
"""
import ctypes
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO, scene_path

sys.path.insert(0, os.path.join(REPO, "tools"))

BIT = dict(trig_mode=1, arg_order=0)
PAD = np.float32(1e3)
PATH_COUNTS = (1, 63, 64, 65, 33 * 17)


# ---- helpers -----------------------------------------------------------------------------------
def _one_leaf(oracle, a):
    """`a` with its tree replaced by ONE leaf over all triangles in array order."""
    n = len(a.triangles)
    if n == 0:
        return dataclasses.replace(a, bvh_nodes=np.zeros(0, oracle.BVHNODE), tri_indices=np.zeros(0, np.int32))
    p = np.concatenate([a.triangles[v]["position"] for v in ("v1", "v2", "v3")]).astype(np.float32)
    node = np.zeros(1, oracle.BVHNODE)
    node["min"], node["max"] = p.min(0) - PAD, p.max(0) + PAD
    node["left"], node["right"], node["start"], node["triCount"] = -1, -1, 0, n
    return dataclasses.replace(a, bvh_nodes=node, tri_indices=np.arange(n, dtype=np.int32))


def _oracle_records(oracle, a, paths, bvh=1):
    pa = np.ascontiguousarray(paths, oracle.PATH)
    out = np.zeros(len(pa), oracle.ISECT)
    oracle.lib().or_compute_intersections(ctypes.byref(a.c_struct()), ctypes.byref(oracle.options(bvh=bvh, **BIT)),
                                          pa.ctypes.data, len(pa), out.ctypes.data)
    return out


def _words(rec):
    r = np.ascontiguousarray(rec)
    assert r.dtype.itemsize == 52
    return r.view(np.uint32).reshape(len(r), 13)


def _same(got, want):
    """Bit-identical 52-byte records; NaN words must be NaN on both sides (the mask), any payload."""
    g, w = _words(got), _words(want)
    isf = np.ones(13, bool)
    isf[4] = False                                      # materialId is the one integer word
    gn, wn = np.isnan(g.view(np.float32)) & isf, np.isnan(w.view(np.float32)) & isf
    return np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn])


def _image_same(got, want):
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(g), np.isnan(w)
    return np.array_equal(gn, wn) and g[~gn].tobytes() == w[~wn].tobytes()


def _tri_array(oracle, pos, normals=None, uvs=None, mats=0, seed=0):
    """TRIANGLE records from (n, 3, 3) positions; tangents are arbitrary finite values (the hit
    record copies them)."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3, 3)
    n = len(pos)
    rng = np.random.default_rng(seed)
    t = np.zeros(n, oracle.TRIANGLE)
    for k, v in enumerate(("v1", "v2", "v3")):
        t[v]["position"] = pos[:, k]
        t[v]["normal"] = 0 if normals is None else np.asarray(normals, np.float32).reshape(n, 3, 3)[:, k]
        t[v]["uv"] = rng.random((n, 2), np.float32) if uvs is None else np.asarray(uvs, np.float32).reshape(n, 3, 2)[:, k]
        t[v]["materialID"] = mats
    t["materialID"] = mats
    t["centroid"] = ((pos[:, 0] + pos[:, 1] + pos[:, 2]) / np.float32(3)).astype(np.float32)
    t["dpdu"] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    t["dpdv"] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    return t


def _random_tris(oracle, n, num_mats, seed):
    """n small triangles inside the cornell box; a fifth with zero vertex normals (flat branch)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([-4, 1, -4], [4, 9, 4], (n, 1, 3))
    pos = (c + rng.uniform(-0.9, 0.9, (n, 3, 3))).astype(np.float32)
    nrm = rng.normal(size=(n, 3, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[rng.random(n) < 0.2] = 0
    return _tri_array(oracle, pos, nrm, None, rng.integers(0, num_mats, n).astype(np.int32), seed)


@pytest.fixture(scope="module")
def cornell(oracle):
    return oracle.load_scene(scene_path("cornell"), res=(48, 48))


def _scene(oracle, base, tris, geoms=None):
    a = dataclasses.replace(base, triangles=np.ascontiguousarray(tris, oracle.TRIANGLE),
                            geoms=base.geoms if geoms is None else geoms)
    return _one_leaf(oracle, a)


def _gpu_naive(ptamd, a, **opts):
    """A naive-mode tracer over a's geoms and triangles, no BVH arrays."""
    view = ptamd.scene_view_from_arrays(a.geoms, a.materials, a.camera, a.trace_depth, triangles=a.triangles)
    assert view.num_bvh_nodes == 0 and view.num_tri_indices == 0
    return ptamd.PathTracer(view, naive_mesh=True, **opts)


def _records_pair(oracle, ptamd, a, paths):
    tr = _gpu_naive(ptamd, a)
    try:
        assert ptamd.get_naive_mesh() == (False, True)  # active; the process-wide setting was put back
        got = tr.test_intersect(np.ascontiguousarray(paths, ptamd.PATH))
    finally:
        tr.free()
    return got, _oracle_records(oracle, a, paths)


def _aimed(oracle, org, dst):
    org, dst = np.atleast_2d(np.asarray(org, np.float32)), np.atleast_2d(np.asarray(dst, np.float32))
    org, dst = np.broadcast_arrays(org, dst)
    p = np.zeros(len(org), oracle.PATH)
    d = (dst - org).astype(np.float32)
    p["origin"] = org
    p["direction"] = (d / np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    p["color"] = 1
    p["remainingBounces"] = 4
    return p


# ---- the frames scene: cornell + four small meshes (diffuse, mirror, glass, textured + bump) -----
MESHES = [("diffuse_red", (-2.8, 2.0, 0.5), 1.7, 1.0), ("nm_mirror", (2.6, 2.6, -0.5), 2.0, 2.0),
          ("nm_glass", (0.1, 6.6, 1.0), 1.8, 3.1), ("nm_textured", (0.2, 1.7, 2.6), 1.4, 0.4)]


@pytest.fixture(scope="module")
def mesh_scene_path(tmp_path_factory):
    import make_synthetic_meshes as M
    d = tmp_path_factory.mktemp("naive_mesh")
    M.write_textures(str(d / "textures"))
    with open(scene_path("cornell")) as f:
        s = json.load(f)
    s["Materials"]["nm_mirror"] = {"RGB": [0.95, 0.95, 0.9], "TYPE": "Reflective"}
    s["Materials"]["nm_glass"] = {"RGB": [0.9, 0.95, 1.0], "TYPE": "Glass", "IOR": 1.5}
    s["Materials"]["nm_textured"] = {"RGB": [0.98, 0.98, 0.98], "TYPE": "Diffuse",
                                     "TEXTURE": "textures/phat_phuck_tex1_albedo.png",
                                     "BUMP_MAP": "textures/phat_phuck_tex2_albedo.png", "BUMP_SCALE": 0.3}
    assert "diffuse_red" in s["Materials"]
    for k, (mat, centre, radius, seed) in enumerate(MESHES):
        v, n, t, f = M.lumpy_sphere(11, 8, centre, (radius, radius * 0.9, radius), lump=0.15, seed=seed)
        M.write_obj(str(d / f"mesh{k}.obj"), v, f, n, t, "(naive mesh test)")
        s["Objects"].append({"TYPE": "obj", "PATH": f"/mesh{k}.obj", "MATERIAL": mat, "TRANS": [0, 0, 0],
                             "ROTAT": [0, 0, 0], "SCALE": [1, 1, 1]})
    s["Camera"]["DEPTH"] = 8
    path = d / "naive_mesh_scene.json"
    path.write_text(json.dumps(s))
    return str(path)


@pytest.fixture(scope="module")
def mesh_scene(oracle, mesh_scene_path):
    a = oracle.load_scene(mesh_scene_path, res=(48, 48), depth=8)
    assert 300 <= len(a.triangles) <= 900 and len(a.bvh_nodes) > 1 and len(a.textures) == 2
    return a


@pytest.fixture(scope="module")
def mesh_reference(oracle, mesh_scene):
    """Oracle on the one-leaf tree, 2 spp: {(compaction, sort): (image after it = 1, 2; live counts)}."""
    leaf = _one_leaf(oracle, mesh_scene)
    out = {}
    for comp, sort in ((1, 0), (0, 0), (1, 1)):
        r = oracle.Renderer(leaf, oracle.options(stream_compaction=comp, material_sort=sort, **BIT))
        images, lives = [], []
        for it in (1, 2):
            lives.append([int(x) if x >= 0 else 0 for x in r.trace(it)])
            images.append(r.image.copy())
        out[(comp, sort)] = (images, lives)
    return out


def _strip_bvh(ptamd, b):
    """b's scene view (textures included) without its BVH arrays."""
    v = ptamd._SceneView()
    ctypes.memmove(ctypes.byref(v), ctypes.byref(b.view()), ctypes.sizeof(v))
    v.bvh_nodes, v.num_bvh_nodes, v.tri_indices, v.num_tri_indices = None, 0, None, 0
    v._keep = b
    return v


def _camera_rays(oracle, a, iteration=1):
    rays = np.zeros(a.pixelcount, oracle.PATH)
    o = oracle.options(**BIT)
    for y in range(a.height):
        for x in range(a.width):
            oracle.lib().or_generate_ray(a.camera.ctypes.data, iteration, a.trace_depth, x, y, ctypes.byref(o),
                                         rays[x + y * a.width:].ctypes.data)
    return rays


# ---- CPU: the method itself -----------------------------------------------------------------------
def test_one_leaf_tree_equals_host_bvh_on_a_tie_free_mesh(oracle, mesh_scene_path):
    """1. Oracle with the one-leaf tree == oracle with the host-built BVH, all 52-byte records of a
    32 x 32 view.  The two visit orders can differ only at rays with two triangles at equal t; this
    mesh and camera have none, so nothing is excluded."""
    a = oracle.load_scene(mesh_scene_path, res=(32, 32), depth=8)
    rays = _camera_rays(oracle, a)
    tree, leaf = _oracle_records(oracle, a, rays), _oracle_records(oracle, _one_leaf(oracle, a), rays)
    tie = (tree["t"] == leaf["t"]) & (_words(tree) != _words(leaf)).any(1)
    assert tie.mean() == 0
    assert _same(tree, leaf)
    prim = _oracle_records(oracle, a, rays, bvh=0)
    mesh_hit = (_words(prim) != _words(leaf)).any(1)
    assert mesh_hit.sum() > 50                          # the meshes are in view; every such ray passed the padded root box
    # further bounces do not meet a tie either: the two trees render the same image
    img = []
    for s in (a, _one_leaf(oracle, a)):
        r = oracle.Renderer(s, oracle.options(**BIT))
        r.trace(1)
        img.append(r.image.copy())
    assert _image_same(img[0], img[1])


def test_frames_scene_is_tie_free_for_the_bvh_equivalence(oracle, mesh_scene, mesh_reference):
    """The precondition of the GPU equivalence test: at 48 x 48, depth 8, 2 spp the host BVH and the
    one-leaf tree give the oracle the same image and live counts."""
    r = oracle.Renderer(mesh_scene, oracle.options(**BIT))
    images, lives = mesh_reference[(1, 0)]
    for k, it in enumerate((1, 2)):
        live = [int(x) if x >= 0 else 0 for x in r.trace(it)]
        assert live == lives[k]
        assert _image_same(r.image, images[k])
    assert np.nansum(images[1]) > 0


# ---- GPU: records ---------------------------------------------------------------------------------
def _tile_counts(ptamd):
    T = ptamd.naive_mesh_tile()
    return [1, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(5))
def test_tile_and_block_edges(which, oracle, ptamd, cornell):
    """4. Triangle counts 1, T-1, T, T+1, 2T+3 (T from the library) x path counts 1, 63, 64, 65,
    33 x 17: every record equals the oracle's."""
    import refpins as R
    n_tris = _tile_counts(ptamd)[which]
    tris = _random_tris(oracle, n_tris, len(cornell.materials), seed=100 + which)
    a = _scene(oracle, cornell, tris)
    rays = R.rays(max(PATH_COUNTS), seed=7 + which, targets=R.scene_targets(a.geoms, a.triangles)).astype(oracle.PATH)
    want = _oracle_records(oracle, a, rays)
    prim = _oracle_records(oracle, a, rays, bvh=0)
    assert ((_words(want) != _words(prim)).any(1)).sum() >= (1 if n_tris == 1 else 20)   # triangles do win
    tr = _gpu_naive(ptamd, a)
    try:
        for n in PATH_COUNTS:
            got = tr.test_intersect(rays[:n].astype(ptamd.PATH))
            assert _same(got, want[:n]), (n_tris, n)
    finally:
        tr.free()


@pytest.mark.gpu
def test_last_triangle_of_the_last_tile_is_tested(oracle, ptamd, cornell):
    """Only the last triangle (index 2T + 2, alone in the third tile's tail) lies on the rays."""
    n = _tile_counts(ptamd)[4]
    pos = np.tile(np.array([[30, 30, 30], [31, 30, 30], [30, 31, 30]], np.float32), (n, 1, 1))
    pos[:, :, 0] += np.arange(n, dtype=np.float32)[:, None] * 2
    pos[-1] = [[-1, 4, 0], [1, 4, 0], [0, 6, 0]]
    mats = np.arange(n, dtype=np.int32) % len(cornell.materials)
    a = _scene(oracle, cornell, _tri_array(oracle, pos, mats=mats), geoms=cornell.geoms[:0])
    rays = _aimed(oracle, [[0, 5, 5], [0.2, 4.5, 3]], [[0, 5, 0], [0.1, 4.6, 0]])
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (got["t"] > 0).all() and (got["materialId"] == mats[-1]).all()


@pytest.mark.gpu
def test_order_and_ties(oracle, ptamd, cornell):
    """5. Duplicate at a later index, shared edge and vertices, primitive against a coplanar triangle
    at equal t, degenerate / edge-on / behind-the-origin triangles, zero vertex normals."""
    nm = len(cornell.materials)
    assert nm >= 3
    no_geoms = cornell.geoms[:0]
    tri = np.array([[-1, 4, 0], [1, 4, 0], [0, 6, 0]], np.float32)
    up = np.tile(np.array([0, 0, 1], np.float32), (3, 1))

    # a triangle duplicated at a later index with another material: the earlier one wins
    a = _scene(oracle, cornell, _tri_array(oracle, [tri, tri + [5, 0, 0], tri], [up] * 3, mats=np.array([1, 0, 2], np.int32)),
               geoms=no_geoms)
    rays = _aimed(oracle, [[0, 5, 5], [0.3, 4.4, 2], [0, 5, -3]], [[0, 5, 0], [0.1, 4.5, 0], [0, 4.8, 0]])
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (got["t"] > 0).all() and (got["materialId"] == 1).all()

    # two triangles sharing the edge (1,4,0)-(0,6,0): rays at its midpoint and at the shared vertices
    other = np.array([[1, 4, 0], [2, 6, 0], [0, 6, 0]], np.float32)
    a = _scene(oracle, cornell, _tri_array(oracle, [tri, other], [up] * 2, mats=np.array([1, 2], np.int32)), geoms=no_geoms)
    targets = np.array([[0.5, 5, 0], [1, 4, 0], [0, 6, 0]], np.float32)
    org = np.array([[0.5, 5, 4], [1, 4, 4], [0, 6, 4], [2, 3, 5], [-1, 7, 3], [0.5, 5, -4]], np.float32)
    rays = np.concatenate([_aimed(oracle, o, targets) for o in org])
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (want["t"] > 0).sum() >= 3

    # a triangle coplanar with a cube's top face at equal t: the primitive wins.  The box test
    # reports the face of the cube y in [0, 2] slightly early (t_p = 1.9998 from y = 4), so the
    # triangle lies in the plane y = 4 - t_p; its edges are 4 long and axis-aligned, which makes
    # intersectTriangle's t for a vertical ray the exact height difference, i.e. t_p again.
    cube = np.zeros(1, oracle.GEOM)
    oracle.lib().or_make_geom(oracle.PT_CUBE, 2, oracle.v3((0, 1, 0)), oracle.v3((0, 0, 0)), oracle.v3((2, 2, 2)),
                              cube.ctypes.data)
    xs = np.array([-0.5, -0.25, 0.0, 0.125, 0.5], np.float32)
    org = np.stack(np.meshgrid(xs, [4.0], xs), -1).reshape(-1, 3).astype(np.float32)
    rays = _aimed(oracle, org, org - np.array([0, 2, 0], np.float32))
    only_prim = _oracle_records(oracle, _scene(oracle, cornell, np.zeros(0, oracle.TRIANGLE), geoms=cube), rays, bvh=0)
    tp = only_prim["t"][0]
    assert tp > 1.9 and (only_prim["t"] == tp).all()
    y = np.float32(4) - tp
    assert np.float32(4) - y == tp
    face = np.array([[-1, y, -1], [-1, y, 3], [3, y, -1]], np.float32)
    nrm = np.tile(np.array([0, 1, 0], np.float32), (3, 1))
    a = _scene(oracle, cornell, _tri_array(oracle, [face], [nrm], mats=np.array([1], np.int32)), geoms=cube)
    only_tri = _oracle_records(oracle, dataclasses.replace(a, geoms=no_geoms), rays)
    assert (only_tri["t"] == tp).all() and (only_tri["materialId"] == 1).all()   # the tie is real
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (got["materialId"] == 2).all() and (got["t"] == tp).all()
    assert (got["uv"] == 0).all() and (got["dpdu"] == 0).all()       # the primitive's record, not the triangle's

    # rejected: a degenerate triangle, one edge-on to the ray (|det| < 1e-5), one behind the origin
    # and one at t <= 1e-5
    degenerate = np.array([[-1, 4, 0], [1, 4, 0], [1, 4, 0]], np.float32)
    a = _scene(oracle, cornell, _tri_array(oracle, [degenerate, tri + [0, 0, 8]], [up] * 2, mats=1), geoms=no_geoms)
    rays = np.concatenate([
        _aimed(oracle, [[0, 4, 5], [0.5, 4, 3]], [[0, 4, 0], [0.5, 4, 0]]),             # at the degenerate one
        _aimed(oracle, [[-3, 5, 8], [0, 2, 8]], [[3, 5, 8], [0, 9, 8]]),                # in the plane z = 8
        _aimed(oracle, [[0, 5, 9]], [[0, 5, 12]]),                                      # triangle behind
    ])
    close = _aimed(oracle, [[0, 5, 8]], [[0, 5, 7]])
    close["origin"][0, 2] = np.float32(8) + np.float32(4e-6)                            # 4e-6 in front of it
    rays = np.concatenate([rays, close])
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (got["t"] == -1).all() and (want["t"] == -1).all()

    # zero vertex normals (one vertex is enough) take the flat normal
    tilted = np.array([[0.6, 0, 0.8], [0.6, 0, 0.8], [0, 0, 0]], np.float32)
    a = _scene(oracle, cornell, _tri_array(oracle, [tri], [tilted], mats=1), geoms=no_geoms)
    rays = _aimed(oracle, [[0, 5, 5], [0.2, 4.5, -3]], [[0, 5, 0], [0, 5, 0]])
    got, want = _records_pair(oracle, ptamd, a, rays)
    assert _same(got, want) and (got["t"] > 0).all()
    assert np.allclose(np.abs(got["surfaceNormal"]), [0, 0, 1], atol=1e-6)
    assert got["surfaceNormal"][0, 2] > 0 > got["surfaceNormal"][1, 2]   # facing the ray


@pytest.mark.gpu
def test_empty_mesh_equals_primitives_only(oracle, ptamd, cornell):
    """6. num_triangles == 0 with the mode on: the primitives-only records and image."""
    import refpins as R
    a = _scene(oracle, cornell, np.zeros(0, oracle.TRIANGLE))
    rays = R.rays(600, seed=5, targets=R.scene_targets(a.geoms, a.triangles)).astype(oracle.PATH)
    want = _oracle_records(oracle, a, rays, bvh=0)
    tr = _gpu_naive(ptamd, a)
    try:
        assert _same(tr.test_intersect(rays.astype(ptamd.PATH)), want)
        r = oracle.Renderer(cornell, oracle.options(bvh=0, **BIT))
        for it in (1, 2):
            r.trace(it)
            tr.trace(it)
        assert _image_same(tr.image(), r.image)
    finally:
        tr.free()


# ---- GPU: frames -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("comp,sort", [(1, 0), (0, 0), (1, 1)])
def test_frames_bitexact(comp, sort, oracle, ptamd, mesh_scene_path, mesh_scene, mesh_reference):
    """7. cornell + diffuse, mirror, glass and textured + bump-mapped meshes, 48 x 48, depth 8, 2 spp:
    image and per-bounce live counts after every frame, then pt_trace_frames over the same frames."""
    images, lives = mesh_reference[(comp, sort)]
    b = ptamd.SceneFile(mesh_scene_path, res=(48, 48), depth=8)
    assert b.camera.tobytes() == mesh_scene.camera.tobytes() and b.triangles.tobytes() == mesh_scene.triangles.tobytes()
    view = _strip_bvh(ptamd, b)
    opts = dict(stream_compaction=comp, material_sort=sort)
    tr = ptamd.PathTracer(view, naive_mesh=True, **opts)
    try:
        assert tr.opts.pipeline == ptamd.PIPELINE_STAGED
        for k, it in enumerate((1, 2)):
            tr.trace(it)
            if comp:
                assert tr.stats()["live"] == lives[k], (it, tr.stats()["live"], lives[k])
            assert _image_same(tr.image(), images[k]), (comp, sort, it)
        tr = ptamd.PathTracer(view, naive_mesh=True, **opts)
        tr.trace_frames(1, 2)
        tr.synchronize()
        assert _image_same(tr.image(), images[1]), ("trace_frames", comp, sort)
        prof = ptamd.PathTracer(view, naive_mesh=True, **opts).profile(1, 2)   # the same passes, eagerly
        assert _image_same(ptamd.PathTracer._live.image(), images[1])
        assert all(ms > 0 for ms in prof["bvh_ms"][:2]) and prof["intersect_ms"] > 0   # k_naive_mesh's launches
    finally:
        ptamd.PathTracer._live.free()


@pytest.mark.gpu
def test_equivalence_with_the_bvh(oracle, ptamd, mesh_scene_path, mesh_reference):
    """8. On the tie-free scene the staged pipeline with the host BVH renders the naive image bit for
    bit, and both-on (bvh = 1, BVH arrays supplied, the mode on) equals naive-only."""
    images, _ = mesh_reference[(1, 0)]
    b = ptamd.SceneFile(mesh_scene_path, res=(48, 48), depth=8)
    assert len(b.bvh_nodes) > 1
    got = {}
    for name, scene, kw in (("bvh", b, dict(pipeline=ptamd.PIPELINE_STAGED)),
                            ("naive", _strip_bvh(ptamd, b), dict(naive_mesh=True)),
                            ("both", b, dict(naive_mesh=True, bvh=1))):
        tr = ptamd.PathTracer(scene, **kw)
        try:
            assert ptamd.get_naive_mesh()[1] == (name != "bvh")
            for it in (1, 2):
                tr.trace(it)
            got[name] = tr.image()
        finally:
            tr.free()
    assert _image_same(got["naive"], images[1])
    assert got["bvh"].tobytes() == got["naive"].tobytes()
    assert got["both"].tobytes() == got["naive"].tobytes()


@pytest.mark.gpu
def test_refusals_and_return_to_the_fused_default(oracle, ptamd, mesh_scene_path, cornell):
    """9. PT_E_UNSUPPORTED (-5) for an explicit fused pipeline, several devices, a shard mode and
    pt_gbuffer_capture; with the mode off again the fused default traces its bit-exact result."""
    b = ptamd.SceneFile(mesh_scene_path, res=(48, 48), depth=8)
    for kw, words in ((dict(pipeline=ptamd.PIPELINE_FUSED), ("naive mesh", "staged", "PT_PIPELINE_FUSED")),
                      (dict(devices=[0, 0]), ("naive mesh", "num_devices")),
                      (dict(shard_mode=ptamd.SHARD_PIXELS, shard_count=2, shard_rank=0), ("naive mesh", "shard_mode"))):
        with pytest.raises(ptamd.PtError) as e:
            ptamd.PathTracer(b, naive_mesh=True, **kw)
        assert "(code -5)" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert ptamd.get_naive_mesh() == (False, False)   # nothing live; the setting was put back
    tr = ptamd.PathTracer(b, naive_mesh=True)
    try:
        with pytest.raises(ptamd.PtError) as e:
            tr.capture_gbuffer(1)
        assert "(code -5)" in str(e.value) and "naive mesh" in str(e.value)
        tr.trace(1)                                       # the context is still usable
    finally:
        tr.free()
    # sticky setter, then off: a new pt_init takes the fused default and its bit-exact result
    ptamd.set_naive_mesh(True)
    try:
        assert ptamd.default_options().pipeline == ptamd.PIPELINE_STAGED
    finally:
        ptamd.set_naive_mesh(False)
    c = ptamd.SceneFile(scene_path("cornell"), res=(48, 48))
    tr = ptamd.PathTracer(c)
    try:
        assert tr.opts.pipeline == ptamd.PIPELINE_FUSED and ptamd.get_naive_mesh() == (False, False)
        r = oracle.Renderer(oracle.load_scene(scene_path("cornell"), res=(48, 48)), oracle.options(**BIT))
        for it in (1, 2):
            tr.trace(it)
            r.trace(it)
        assert tr.image().tobytes() == r.image.tobytes()
    finally:
        tr.free()


@pytest.mark.gpu
def test_pt_render_naive_mesh(tmp_path, ptamd, mesh_scene_path):
    """10. `pt_render --naive-mesh` at 32 x 32, 1 spp writes the PNG bytes of ptamd in naive mode."""
    exe = os.path.join(PKG, "build", "pt_render")
    out = str(tmp_path / "render")
    env = {k: v for k, v in os.environ.items() if k != "PT_NAIVE_MESH"}
    subprocess.run([exe, mesh_scene_path, "--naive-mesh", "--spp", "1", "--res", "32x32", "--out", out], check=True,
                   timeout=120, env=env)
    b = ptamd.SceneFile(mesh_scene_path, res=(32, 32))    # the viewer camera, as pt_render applies it
    tr = ptamd.PathTracer(b, naive_mesh=True)
    try:
        tr.trace(1)
        img = tr.image()
    finally:
        tr.free()
    ref = str(tmp_path / "ref")
    ptamd.save_png(img, 32, 32, 1, ref)
    with open(out + ".png", "rb") as f, open(ref + ".png", "rb") as g:
        png = f.read()
        assert png == g.read() and len(png) > 100
    assert np.nansum(img) > 0
