"""Ray-level probes of the FUSED pipeline's bounce kernels — needs an MI355X.

PathTracer.test_bounce (pt_test_bounce) lays caller paths into a bounce's input segments and runs
launch_bounce (csrc/rt_pass.h) exactly as a frame does: k_bounce with the context's variant (block_intersect /
wave_intersect / intersect_scene_q, the candidate table, material grouping) and, in mesh scenes,
k_bvh_bounce -> k_bvh_tail_trav -> k_bvh_tail_shade behind the split queue.  Frames only ever feed
these kernels rays that start at the camera or on a surface inside the room; here they get
adversarial ones.

Expected values: the oracle in the bit mode, or_compute_intersections + or_shade per path.  The
survivors (remainingBounces > 0 afterwards) are matched by their unique pixelIndex and compared in
all 11 words; a terminated path's pixel must hold 0 + colour, every other pixel 0.  NaN equals NaN
whatever the payload (tests/test_bsdf_pin.py::differing).

Ray sets: (a) refpins.rays, the mix that pins the staged kernel against the reference's own
intersections.cu; (b) test_gpu_parity._random_paths (NaN directions, components around geom_test's
shared-reciprocal bound); (c) rays built from PathTracer.grid_info() for the candidate table and
the pre-test: origins on / one float beside every cell boundary, outside the table, direction
ratios on / one float beside every bin boundary (raw and normalised), dominant-axis ties in every
sign combination, magnitudes on both sides of grid_superset's m > 1e-30f gate and of the away
drop's `bounded` (1e3), zero and infinite directions; half of their origins are oracle hit points
of (a) moved 1e-4 along the normal (rays that leave a surface).

The conditions that keep the cases honest (hit / terminate / survive / mesh-hit shares, class
sizes, a float64 restatement of the table lookup) are computed from the oracle and numpy only and
asserted in every case.
"""
import ctypes
import json

import numpy as np
import pytest

import refpins as R
from conftest import scene_path
from test_bsdf_pin import differing
from test_gpu_parity import _many_geoms_scene, _random_paths

pytestmark = pytest.mark.gpu

BIT = dict(trig_mode=1, arg_order=0)
RES = (96, 96)
PIX = RES[0] * RES[1]            # the one-frame wavefront capacity
N = 6000
ITERS = (2, 5000)
NSEG = 8
# kernel variant bits (csrc/pt_records.h)
VAR_BVH_SPLIT, VAR_MAT_GROUP, VAR_NO_TEX = 32, 512, 1024
VAR_DEFAULT = 2 | 8 | 16 | 32 | 128      # pt_default_options: candidate queue, block-wide exchange, split BVH
NO_TEX = {"cornell": True, "synthetic_textured_bump": False}
CLASSES = ("cell", "outside", "bin", "tie", "below_gate", "above_gate", "within_bounded", "beyond_bounded",
           "zero", "inf")
MIN_CLASS = ("cell", "outside", "bin", "tie", "below_gate", "above_gate", "beyond_bounded")
GATE = np.float32(1e-30)


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def _grid_scene(path, n, outside):
    """_many_geoms_scene(n), with the two objects outside the room of
    test_candidate_table_scenes_bitexact when `outside`."""
    path = _many_geoms_scene(path, n)
    if outside:
        with open(path) as f:
            d = json.load(f)
        d["Objects"] += [{"TYPE": "sphere", "MATERIAL": "mirror", "TRANS": [0, 5, 14], "ROTAT": [0, 0, 0],
                          "SCALE": [3, 3, 3]},
                         {"TYPE": "cube", "MATERIAL": "diffuse_white", "TRANS": [-9, 2, 0], "ROTAT": [10, 20, 30],
                          "SCALE": [1, 6, 2]}]
        with open(path, "w") as f:
            json.dump(d, f)
    return path


GENERATED = {"grid33": (33, True), "grid12": (12, False), "many72": (72, False)}
DEPTH = {"cornell_obj_khaslana": 12}
TABLE_SCENES = ("grid33", "grid12", "cornell_obj_khaslana", "cornell_obj_cyrene")   # 16 .. 64 geoms
MESH_SCENES = ("cornell_obj_bnnuy", "cornell_obj_khaslana", "synthetic_textured_bump", "cornell_obj_cyrene")


@pytest.fixture(scope="module")
def scenes(tmp_path_factory, oracle, ptamd):
    """name -> (oracle scene, SceneFile), loaded once per module."""
    cache = {}
    tmp = tmp_path_factory.mktemp("fused_bounce")

    def get(name):
        if name not in cache:
            path = scene_path(name)
            if name in GENERATED:
                path = _grid_scene(tmp / (name + ".json"), *GENERATED[name])
            a = oracle.load_scene(path, res=RES, depth=DEPTH.get(name))
            b = ptamd.SceneFile(path, res=RES, depth=DEPTH.get(name))
            assert a.camera.tobytes() == b.camera.tobytes()
            cache[name] = (a, b)
        return cache[name]
    return get


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def _isects(oracle, a, paths, bvh=1):
    out = np.zeros(len(paths), oracle.ISECT)
    pa = np.ascontiguousarray(paths, oracle.PATH)
    if len(pa):
        oracle.lib().or_compute_intersections(ctypes.byref(a.c_struct()), ctypes.byref(oracle.options(bvh=bvh, **BIT)),
                                              pa.ctypes.data, len(pa), out.ctypes.data)
    return out


def _shade(oracle, a, it, isects, paths):
    ref = np.array(paths, oracle.PATH)
    s, o = a.c_struct(), oracle.options(**BIT)
    for i in range(len(ref)):
        oracle.lib().or_shade(ctypes.byref(s), ctypes.byref(o), int(it), isects[i:].ctypes.data, ref[i:].ctypes.data)
    return ref


# ---------------------------------------------------------------------------------------------
# set (c)
# ---------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float32)


def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def _neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def set_c(grid, surface, targets, seed):
    """(origins, directions, class tag per ray, marked-inside flag per ray).  `surface`: origins on
    surfaces (oracle hit points of set (a) + 1e-4 * normal), used for every other ray whose origin is
    not its point; `targets`: aim points (refpins.scene_targets) for half the rays whose direction is not."""
    rng = np.random.default_rng(seed)
    lo, inv = grid["lo"].astype(np.float64), grid["inv"].astype(np.float64)
    G, B = grid["cells"], grid["bins"]
    hi = lo + G / inv
    org, drn, tag, inside = [], [], [], []
    count = [0]

    def in_table():
        return (lo + rng.uniform(0.02, 0.98, 3) * (hi - lo)).astype(np.float32)

    def base_origin():
        count[0] += 1
        if count[0] % 2 and len(surface):
            return surface[(count[0] // 2) % len(surface)]
        return rng.uniform([-4.9, 0.1, -4.9], [4.9, 9.9, 4.9]).astype(np.float32)

    def put(o, d, t, ins=True):
        org.append(_f32(o))
        drn.append(_f32(d))
        tag.append(CLASSES.index(t))
        inside.append(ins)

    def into_room(o):
        to = rng.uniform([-4, 1, -4], [4, 9, 4])
        if len(targets) and rng.random() < 0.5:
            to = targets[rng.integers(len(targets))].astype(np.float64)
        return _unit(to - np.asarray(o, np.float64) + 1e-9)

    # cell boundaries: lo + k / inv and its two float neighbours on one axis
    for a in range(3):
        for k in range(G + 1):
            for j, x in enumerate(_neighbours(lo[a] + k / inv[a])):
                o = in_table()
                o[a] = x
                put(o, into_room(o), "cell", ins=not ((k == 0 and j == 0) or k == G))
    # outside the table: one float below lo, at the upper edge, beyond it
    for a in range(3):
        for rep in range(4):
            for x in (np.nextafter(np.float32(lo[a]), np.float32(-np.inf)), np.float32(lo[a] - 2.5),
                      np.float32(hi[a]), np.nextafter(np.float32(hi[a]), np.float32(np.inf)), np.float32(hi[a] + 3.0)):
                o = in_table()
                o[a] = x
                # (the float just below a float32 lo is outside; f32(hi) may round inside: not marked)
                put(o, into_room(o), "outside", ins=False)
    # bin boundaries: dominant component +-1, one other on -1 + 2 b / B and its float neighbours
    for k in range(3):
        for which in (1, 2):
            for b in range(B + 1):
                for x in _neighbours(-1.0 + 2.0 * b / B):
                    d = np.zeros(3, np.float32)
                    d[k] = 1.0 if (b + which + k) % 2 else -1.0
                    d[(k + which) % 3] = x
                    d[(k + 3 - which) % 3] = np.float32(rng.uniform(-0.999, 0.999))
                    o = base_origin()
                    put(o, d, "bin")
                    put(o, _unit(d), "bin")
    # dominant-axis ties, every sign combination
    for pat in ((1.0, 1.0, 0.37), (1.0, 0.37, 1.0), (0.37, 1.0, 1.0), (1.0, 1.0, 1.0)):
        for s in range(8):
            sg = np.array([1 if s & 1 else -1, 1 if s & 2 else -1, 1 if s & 4 else -1], np.float64)
            d = np.array(pat) * sg
            put(base_origin(), d, "tie")
            put(base_origin(), _unit(d), "tie")
            put(base_origin(), d * 0.3, "tie")
    # magnitudes: the largest component on both sides of m > 1e-30f and of `bounded` (<= 1e3)
    below = [GATE, np.nextafter(GATE, np.float32(0)), np.float32(0.5e-30), np.float32(0.99e-30)]
    above = [np.nextafter(GATE, np.float32(1)), np.float32(1.01e-30), np.float32(2e-30), np.float32(1e-29)]
    within = [np.float32(1e3), np.nextafter(np.float32(1e3), np.float32(0)), np.float32(999.0)]
    beyond = [np.nextafter(np.float32(1e3), np.float32(1e4)), np.float32(2e3), np.float32(1001.0)]
    for mags, t, reps in ((below, "below_gate", 10), (above, "above_gate", 10), (within, "within_bounded", 12),
                          (beyond, "beyond_bounded", 12)):
        for m in mags:
            for rep in range(reps):
                o = base_origin()
                d = into_room(o).astype(np.float64) if rep % 2 else _unit(rng.normal(size=3)).astype(np.float64)
                k = int(np.argmax(np.abs(d)))
                d = (d / abs(d[k]) * np.float64(m)).astype(np.float32)
                d[k] = np.copysign(m, d[k])
                put(o, d, t, ins=t != "below_gate")
    # zero and infinite directions
    for s in range(8):
        put(base_origin(), [0.0 if s & 1 else -0.0, 0.0 if s & 2 else -0.0, 0.0 if s & 4 else -0.0], "zero", ins=False)
    for k in range(3):
        for sg in (1.0, -1.0):
            for rep in range(2):
                d = _unit(rng.normal(size=3))
                d[k] = sg * np.inf
                put(base_origin(), d, "inf", ins=False)
    return np.array(org, np.float32), np.array(drn, np.float32), np.array(tag, np.int32), np.array(inside, bool)


def table_lookup(grid, o, d):
    """grid_superset's index computation restated in float64: (indexes the table, within one float of
    a cell edge, within one float of a bin edge) per ray."""
    lo, inv = grid["lo"].astype(np.float64), grid["inv"].astype(np.float64)
    G, B = grid["cells"], grid["bins"]
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(all="ignore"):
        f = (o64 - lo) * inv
        in_cells = ((f >= 0) & (f < G)).all(axis=1)
        ad = np.abs(d64)
        kx = (ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2])
        ky = ~kx & (ad[:, 1] >= ad[:, 2])
        k = np.where(kx, 0, np.where(ky, 1, 2))
        rows = np.arange(len(o))
        m = ad[rows, k]
        ok = in_cells & np.isfinite(ad.sum(axis=1)) & (m > np.float64(GATE))
        cell_edge = (np.abs(f - np.rint(f)) / inv <= np.spacing(np.abs(o))).any(axis=1) & np.isfinite(f).all(axis=1)
        r = np.stack([d64[rows, (k + 1) % 3], d64[rows, (k + 2) % 3]], 1) / m[:, None]
        x = (r + 1.0) * (0.5 * B)
        bin_edge = ok & (np.abs(x - np.rint(x)) * (2.0 / B) <= np.spacing(np.abs(r).astype(np.float32))).any(axis=1)
    return ok, cell_edge, bin_edge


# ---------------------------------------------------------------------------------------------
# cases: paths + expectations, cached (the layout, size and variant tests share them)
# ---------------------------------------------------------------------------------------------
class Case:
    pass


_CASES = {}


def make_case(oracle, a, name, grid, n=N, seed=1):
    key = (name, n, seed, grid["lo"].tobytes(), grid["inv"].tobytes(), grid["cells"])
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed + 1000)
    targets = R.scene_targets(a.geoms, a.triangles)
    # hit points of a first batch of (a): origins on surfaces for set (c)
    probe = R.rays(512, seed + 7, targets)
    pi = _isects(oracle, a, R.pack(probe, R.P_PATH).astype(oracle.PATH))
    hit = (pi["t"] > 0) & np.isfinite(pi["t"]) & np.isfinite(probe["origin"]).all(axis=1)
    with np.errstate(all="ignore"):
        pts = probe["origin"] + pi["t"][:, None] * probe["direction"] + np.float32(1e-4) * pi["surfaceNormal"]
    surface = pts[hit & np.isfinite(pts).all(axis=1)].astype(np.float32)
    co, cd, ctag, cins = set_c(grid, surface, targets, seed + 3)
    if len(co) > n * 0.45:                       # small cases: thin (c) out evenly, every class kept
        keep = np.zeros(len(co), bool)
        step = int(np.ceil(len(co) / (n * 0.45)))
        for c in range(len(CLASSES)):
            idx = np.flatnonzero(ctag == c)
            keep[idx[::step]] = True
            keep[idx[:40]] = True
        co, cd, ctag, cins = co[keep], cd[keep], ctag[keep], cins[keep]
    nc = min(len(co), n)
    nb = min(n // 4, n - nc)
    na = n - nc - nb
    p = np.zeros(n, oracle.PATH)
    ra = R.rays(na, seed, targets)
    rb = _random_paths(nb, seed + 1)
    p["origin"][:na], p["direction"][:na] = ra["origin"], ra["direction"]
    p["origin"][na:na + nb], p["direction"][na:na + nb] = rb["origin"], rb["direction"]
    p["origin"][na + nb:], p["direction"][na + nb:] = co[:nc], cd[:nc]
    p["color"] = rng.uniform(0.1, 1.0, (n, 3)).astype(np.float32)
    p["remainingBounces"] = rng.integers(1, 9, n)
    dead = np.arange(n) % 29 == 5                # paths that were not alive: neither survive nor gather
    p["remainingBounces"][dead] = np.array([0, -1, -7], np.int32)[np.arange(dead.sum()) % 3]
    p["pixelIndex"] = rng.permutation(PIX)[:n]
    order = rng.permutation(n)                   # the sets interleaved: every wave sees every kind
    c = Case()
    c.name, c.n, c.grid = name, n, grid
    c.paths = p[order]
    tags = np.concatenate([np.full(na, -1), np.full(nb, -2), ctag[:nc]]).astype(np.int32)
    c.tag = tags[order]
    c.inside = np.concatenate([np.zeros(na + nb, bool), cins[:nc]])[order]
    c.live = c.paths["remainingBounces"] > 0
    c.isects = _isects(oracle, a, c.paths)
    c.hit = c.isects["t"] > 0
    c.mesh = np.zeros(n, bool)
    if len(a.triangles):                         # a mesh hit: the primitives alone give another record
        prim = _isects(oracle, a, c.paths, bvh=0)
        c.mesh = c.hit & (np.ascontiguousarray(c.isects).view(np.uint8).reshape(n, -1) !=
                          np.ascontiguousarray(prim).view(np.uint8).reshape(n, -1)).any(axis=1)
    c.expected = {}
    c.oracle, c.scene = oracle, a
    _CASES[key] = c
    return c


def expected(c, it):
    if it not in c.expected:
        e = Case()
        e.ref = _shade(c.oracle, c.scene, it, c.isects, c.paths)
        e.surv = c.live & (e.ref["remainingBounces"] > 0)
        e.term = c.live & ~e.surv
        e.image = np.zeros((PIX, 3), np.float32)
        with np.errstate(all="ignore"):
            e.image[c.paths["pixelIndex"][e.term]] = np.float32(0) + e.ref["color"][e.term]
        c.expected[it] = e
    return c.expected[it]


def tag_name(t):
    return {-1: "a", -2: "b"}.get(int(t)) or "c:" + CLASSES[int(t)]


def assert_honest(c, e, mesh):
    """The conditions of the issue, from the oracle and numpy only."""
    live = c.live
    share = {"hit": c.hit[live].mean(), "term": e.term[live].mean(), "surv": e.surv[live].mean(),
             "mesh": c.mesh[live & c.hit].mean() if (live & c.hit).any() else 0.0}
    print(f"{c.name} n={c.n}: " + " ".join(f"{k}={v:.3f}" for k, v in share.items()))
    assert c.hit.mean() >= 0.30 and e.term.mean() >= 0.10 and e.surv.mean() >= 0.30, share
    if mesh:
        assert c.mesh[c.hit].mean() >= 0.20, share
    assert len(np.unique(c.paths["pixelIndex"])) == c.n and c.paths["pixelIndex"].max() < PIX
    assert (~live).sum() >= 32 or c.n < 1000
    if c.n < 1000:
        return
    for name in MIN_CLASS:
        assert (c.tag == CLASSES.index(name)).sum() >= 32, name
    isc = c.tag >= 0
    ok, cell_edge, bin_edge = table_lookup(c.grid, c.paths["origin"][isc], c.paths["direction"][isc])
    assert ok[c.inside[isc]].mean() >= 0.90, ok[c.inside[isc]].mean()
    assert cell_edge.sum() >= 32 and bin_edge.sum() >= 32, (cell_edge.sum(), bin_edge.sum())


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def _words(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(len(x), -1)


def _image_diff(got, want):
    """Pixels that differ; NaN against NaN is equal, NaN against a number is not."""
    ne = _words(got) != _words(want)
    ne &= ~(np.isnan(got) & np.isnan(want))
    return np.flatnonzero(ne.any(axis=1))


def oracle_geom(c, i):
    """Index of the geom the oracle's primitive loop picks for path i (first minimum of the box /
    sphere tests, or_prim_probe), -1 for none.  For a mesh hit this is the geom the triangle beat:
    the oracle's intersection record (ShadeableIntersection) carries no triangle index."""
    ng = len(c.scene.geoms)
    if ng == 0:
        return -1
    out = np.zeros((ng, 8), np.float32)
    pa = np.ascontiguousarray(c.paths[i:i + 1], c.oracle.PATH)
    c.oracle.lib().or_prim_probe(c.scene.geoms.ctypes.data, ng, pa.ctypes.data, 1, out.ctypes.data)
    best, t_min = -1, np.inf
    for g in range(ng):
        if out[g, 0] > 0 and t_min > out[g, 0]:
            best, t_min = g, out[g, 0]
    return best


def check(c, e, surv, seg_out, img, label):
    by_pix = np.full(PIX, -1, np.int64)
    by_pix[c.paths["pixelIndex"]] = np.arange(c.n)
    bad = {}

    def note(idx, what):
        for i in idx:
            bad.setdefault(int(i), what)

    want = e.ref[e.surv]
    gp, wp = surv["pixelIndex"].astype(np.int64), want["pixelIndex"].astype(np.int64)
    valid = (gp >= 0) & (gp < PIX)
    assert valid.all(), (label, "survivor with a pixelIndex outside the image", gp[~valid][:8])
    seen = np.bincount(gp, minlength=PIX)
    exp_seen = np.bincount(wp, minlength=PIX)
    unknown = np.flatnonzero((seen > 0) & (by_pix < 0))
    assert len(unknown) == 0, (label, "survivors of pixels no path was given for", unknown[:8])
    note(by_pix[np.flatnonzero((exp_seen == 1) & (seen == 0))], "survivor missing")
    note(by_pix[np.flatnonzero((exp_seen == 0) & (seen > 0))], "must not survive")
    note(by_pix[np.flatnonzero(seen > 1)], "survivor more than once")
    if not bad:
        g, w = surv[np.argsort(gp, kind="stable")], want[np.argsort(wp, kind="stable")]
        note(by_pix[w["pixelIndex"][differing(g, w)]], "survivor record differs")
    pix = _image_diff(img, e.image)
    note([by_pix[p] for p in pix if by_pix[p] >= 0], "pixel differs")
    stray = [int(p) for p in pix if by_pix[p] < 0]
    first = [(i, what, tag_name(c.tag[i]), f"t={c.isects['t'][i]!r}", f"mat={int(c.isects['materialId'][i])}",
              ("mesh hit, nearest geom " if c.mesh[i] else "geom ") + str(oracle_geom(c, i)),
              f"rb={int(c.paths['remainingBounces'][i])}")
             for i, what in sorted(bad.items())[:8]]
    assert not bad and not stray, (label, len(bad), "first failing paths:", first, "pixels without a path:", stray[:8])
    assert int(np.sum(seg_out)) == int(e.surv.sum()) == len(surv), (label, seg_out, int(e.surv.sum()), len(surv))


def run(tr, c, it, label, seg_counts=None, bounce=1):
    e = expected(c, it)
    tr.set_image(np.zeros((PIX, 3), np.float32))
    surv, seg_out = tr.test_bounce(it, c.paths, bounce=bounce, seg_counts=seg_counts)
    img = tr.image()
    check(c, e, surv, seg_out, img, (label, it))
    return surv, img


def room_grid(a):
    """For scenes without a table: a grid over the geoms' world boxes and the camera, so set (c)
    probes the flat pre-test with the same kinds of rays."""
    corners = np.array([[x, y, z, 1] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)], np.float64)
    pts = [np.asarray(a.camera["position"], np.float64).reshape(1, 3)]
    for g in a.geoms:                            # glm matrices are stored column by column
        pts.append((corners @ np.asarray(g["transform"], np.float64))[:, :3])
    pts = np.concatenate(pts)
    lo, hi = pts.min(0) - 0.01, pts.max(0) + 0.01
    return {"lo": lo.astype(np.float32), "inv": (12 / (hi - lo)).astype(np.float32), "cells": 12, "bins": 16}


def grid_of(tr, a):
    g = tr.grid_info()
    return g if g["cells"] > 0 else room_grid(a)


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
CASES = [
    ("cornell", {}, None, N),                                  # block_intersect, flat cull_candidates, away drop
    ("cornell", {"variant": 58}, None, N),                     # wave_intersect
    ("cornell", {"variant": 2}, None, N),                      # intersect_scene_q / prim_intersect_q, index order
    ("cornell_glass_test", {"material_sort": 1}, None, N),     # group_by_material after the exchange
    ("grid33", {}, None, N),                                   # grid_superset, cull_candidates_grid
    ("grid33", {"variant": 58}, None, N),
    ("grid12", {}, None, N),                                   # 19 geoms: the smallest table
    ("many72", {}, None, N),                                   # > LDS_GEOMS: global-table intersect_scene
    ("cornell_obj_bnnuy", {}, None, N),                        # prim_intersect_q + root test + queue + hand-over
    ("cornell_obj_bnnuy", {}, 0, N),
    ("cornell_obj_bnnuy", {}, 56, N),
    ("cornell_obj_khaslana", {}, None, N),                     # table + split queue together
    ("cornell_obj_khaslana", {"material_sort": 1}, None, N),
    ("synthetic_textured_bump", {}, None, N),                  # hit_attr and the tail shade's texture reads
    ("cornell_obj_cyrene", {}, None, 2048),                    # the 4-wide records, vertex / edge-midpoint rays
]


def _id(v):
    name, opts, lanes, n = v
    s = name + "".join(f"-{k}{x}" for k, x in opts.items())
    return s + (f"-lanes{lanes}" if lanes is not None else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bounce_matches_oracle(case, scenes, oracle, ptamd, monkeypatch):
    name, opts, lanes, n = case
    if lanes is not None:
        monkeypatch.setenv("PT_BVH_TAIL_LANES", str(lanes))
    a, b = scenes(name)
    tr = ptamd.PathTracer(b, **opts)
    try:
        # what the context really launches (launch_bounce's effective variant), not what was asked for:
        # pt_init drops material grouping, and the layout drops the fast / split traversal, silently
        mesh = name in MESH_SCENES
        want = opts.get("variant", VAR_DEFAULT) | (VAR_MAT_GROUP if opts.get("material_sort") else 0)
        if not mesh:
            want &= ~VAR_BVH_SPLIT             # nothing to queue without a mesh
        got, split = tr.bounce_variant()
        assert got & ~VAR_NO_TEX == want and split == mesh, (_id(case), got, want, split)
        if name in NO_TEX and "variant" not in opts:   # the texture-free build exists for the default variants
            assert bool(got & VAR_NO_TEX) == NO_TEX[name], (name, got)
        c = make_case(oracle, a, name, grid_of(tr, a), n=n)
        assert (tr.grid_info()["cells"] > 0) == (name in TABLE_SCENES)
        for it in ITERS:
            assert_honest(c, expected(c, it), name in MESH_SCENES)
            run(tr, c, it, _id(case))
        run(tr, c, ITERS[0], _id(case) + "-bounce4", bounce=4)     # the other path buffer, later counter rows
    finally:
        tr.free()


@pytest.mark.parametrize("name", ["cornell", "cornell_obj_bnnuy"])
def test_segment_layouts(name, scenes, oracle, ptamd):
    """The same paths in one segment, spread evenly, and split so that waves and blocks straddle
    segment boundaries (segment_slot): the same survivors, the same image, the oracle's."""
    a, b = scenes(name)
    tr = ptamd.PathTracer(b)
    try:
        c = make_case(oracle, a, name, grid_of(tr, a))
        head = [1, 63, 64, 65, 255, 257, 0]
        # "edge63": a segment that ends on a wave's last lane (segment_slot's `w0 + 63 < hi`)
        layouts = {"one": None, "even": [N // NSEG] * NSEG, "straddle": head + [N - sum(head)],
                   "edge63": [63, 128, 1, 0, 0, 0, 0, N - 192]}
        assert all(sum(v) == N for v in layouts.values() if v)
        it = ITERS[0]
        got = {}
        scrub = c.paths[::-1].copy()             # what a slot read past a segment's end would find:
        scrub["remainingBounces"] = 0            # another path, not the stale copy of the right one
        for key, seg in layouts.items():
            assert len(tr.test_bounce(it, scrub)[0]) == 0
            surv, img = run(tr, c, it, (name, key), seg_counts=seg)
            got[key] = (surv[np.argsort(surv["pixelIndex"], kind="stable")], img)
        for key in ("even", "straddle", "edge63"):
            assert len(differing(got[key][0], got["one"][0])) == 0, key
            assert len(_image_diff(got[key][1], got["one"][1])) == 0, key
    finally:
        tr.free()


@pytest.mark.parametrize("name", ["cornell", "grid33"])
def test_partial_blocks_and_waves(name, scenes, oracle, ptamd):
    """n around the wave and block sizes: every lane of a partial wave still takes part in the
    exchange, and n = 0 launches nothing."""
    a, b = scenes(name)
    tr = ptamd.PathTracer(b)
    try:
        full = make_case(oracle, a, name, grid_of(tr, a))
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            c = Case()
            c.name, c.n, c.grid, c.oracle, c.scene, c.expected = name, n, full.grid, oracle, a, {}
            for f in ("paths", "tag", "inside", "live", "isects", "hit", "mesh"):
                setattr(c, f, getattr(full, f)[:n])
            run(tr, c, ITERS[1], (name, n))
    finally:
        tr.free()


@pytest.mark.parametrize("name", ["cornell", "cornell_obj_bnnuy"])
def test_no_side_effect_on_later_frames(name, scenes, oracle, ptamd):
    """A frame traced after a test_bounce is the oracle's, bit for bit (cornell: k_head + k_tail)."""
    a, b = scenes(name)
    tr = ptamd.PathTracer(b)
    try:
        c = make_case(oracle, a, name, grid_of(tr, a))
        run(tr, c, ITERS[0], name, seg_counts=[N // NSEG] * NSEG, bounce=3)
        tr.set_image(np.zeros((PIX, 3), np.float32))
        r = oracle.Renderer(a, oracle.options(**BIT))
        for it in (1, 2):
            live = r.trace(it)
            tr.trace(it)
            assert tr.stats()["live"] == [int(x) if x >= 0 else 0 for x in live]
        assert tr.image().tobytes() == np.asarray(r.image).tobytes()
    finally:
        tr.free()


def test_refusals(scenes, oracle, ptamd):
    """Every refusal is PT_E_INVALID with a message, and refuses before anything is launched."""
    a, b = scenes("cornell")
    p = np.zeros(PIX + 1, ptamd.PATH)
    p["pixelIndex"] = np.arange(PIX + 1) % PIX
    p["remainingBounces"] = 1
    p["direction"] = (0, 0, -1)
    p["origin"] = (0, 5, 0)

    def refused(tr, word, paths, **kw):
        with pytest.raises(ptamd.PtError) as ei:
            tr.test_bounce(1, paths, **kw)
        msg = str(ei.value)
        assert "(code -1)" in msg and word in msg and len(msg) > 30, msg

    tr = ptamd.PathTracer(b, frames_per_pass=1)      # buffers of one frame: a segment holds 5 blocks
    try:
        stride = -(-(PIX // 256) // NSEG) * 256
        refused(tr, "wavefront", p)                                  # n above one frame's paths
        refused(tr, "segment", p[:stride + 1], seg_counts=[stride + 1] + [0] * 7)
        refused(tr, "segment", p[:8], seg_counts=[9, -1, 0, 0, 0, 0, 0, 0])
        refused(tr, "add up", p[:8], seg_counts=[1] * 7 + [2])
        refused(tr, "bounce", p[:8], bounce=64)
        refused(tr, "bounce", p[:8], bounce=0)                       # the camera bounce makes its own rays
        surv, seg_out = tr.test_bounce(1, p[:stride], seg_counts=[stride] + [0] * 7)   # exactly full: accepted
        assert len(surv) == seg_out.sum()
    finally:
        tr.free()
    tr = ptamd.PathTracer(b, pipeline=ptamd.PIPELINE_STAGED)
    try:
        refused(tr, "staged", p[:8])
    finally:
        tr.free()
