"""scatterRay and the BSDFs, bit for bit against the reference's own code.

tests/golden/bsdf_pin.npz holds inputs on the edges of the shading code and what the reference's
src/interactions.cu computed for them (oracle/ref_pins/bsdf_pin.cpp, compiled from the reference in
place; generator oracle/ref_pins/make_bsdf_fixtures.py).  These tests read only tests/golden/.

* the stand-in thrust/random.h that build uses reproduces tests/golden/rng_pin.json (rocThrust);
* the oracle in glibc mode (trig_mode=0, arg_order=0) equals the fixture on every record;
* the fixture still holds the branches it was built to reach;
* the oracle's portable trig (trig_mode=1, what the GPU is bit-exact with) stays within a bound
  measured once against the fixture;
* (GPU) k_shade equals the fixture byte for byte on the classes that call no sin / cos / powf, and
  equals or_shade(trig_mode=1) on the rest.

Comparison rule.  Finite values, infinities, integers: by bits.  A component that is NaN on both
sides counts as equal whatever its sign and payload: g++ (the harness), gcc (the oracle) and the
GPU pick different ones for the same operation (x86 SSE produces the negative default NaN, 0 * inf
folded by a compiler the positive one; 14 scatter records of the fixture, all with a NaN normal
component, differ from the oracle in nothing else).  NaN against non-NaN is a difference.
"""
import ctypes
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import refpins as R
from conftest import GOLDEN, REPO

SCENE = os.path.join(GOLDEN, "bsdf_pin_scene.json")
TRIG_FREE = (R.REFLECTIVE, R.TRANSMISSIVE, R.GLASS)      # no sin / cos / powf on their path

# trig_mode=1 against the fixture, measured on this fixture (deterministic: the fixture is fixed and
# pt_libm is exact arithmetic on floats); the tests assert twice the measured figures.  Unit: ulps of
# the fixture vector's largest component (a component near 0 is the difference of rounded products,
# so its own ulp says nothing).  Scatter and shade records measure the same.
#   plain records (1860 diffuse + microfacet): direction 10.875, colour 25, origin 0, lobe flips 0
#   rim records (294): direction 5016.6; colour: 24 records finite on one side only
# A rim record is one whose seed was searched so that a draw is exactly 0 or 1.  There the
# concentric map's radius is exactly 1 and z = sqrt(1 - cos^2 - sin^2) turns a trig rounding of
# ~1e-7 into ~3e-4; the reference gets z == 0 (pdf 0, colour inf / NaN or left alone), pt_libm a
# small positive z (finite colour).  Their colour is c / pdf with pdf = z / PI: no bound means anything.
MEASURED_DIR_ULPS = 10.875
MEASURED_COLOR_ULPS = 25.0
MEASURED_RIM_DIR_ULPS = 5016.6
MEASURED_RIM_COLOR_KIND_MISMATCHES = 24
FLIP_CAP = 0.01                                           # of the diffuse + microfacet records
FLIP_DIRECTION_DELTA = 1e-3                               # another lobe samples another direction


@functools.lru_cache(maxsize=None)
def fixture():
    fx = dict(np.load(os.path.join(GOLDEN, "bsdf_pin.npz")))
    fx["shade_in"] = R.bsdf_shade_inputs(fx)
    fx["scatter_class"] = R.bsdf_class(fx["scatter_in"]["material"])
    fx["shade_class"] = R.bsdf_class(fx["materials"][fx["shade_material"]])
    fx["shade_tag"] = fx["scatter_tag"][fx["shade_index"]]
    return fx


def _words(paths):
    return np.ascontiguousarray(paths).view(np.uint32).reshape(len(paths), 11)


def differing(got, want):
    """Record indices that differ under the module's comparison rule."""
    a, b = _words(got), _words(want)
    af, bf = a.view(np.float32)[:, :9], b.view(np.float32)[:, :9]
    ne = a != b
    ne[:, :9] &= ~(np.isnan(af) & np.isnan(bf))
    return np.flatnonzero(ne.any(axis=1))


def report(bad, cls, tags, fx):
    """First differing record indices per class, with the case they came from."""
    out = {}
    for c, name in enumerate(R.BSDF_CLASSES):
        idx = bad[cls[bad] == c][:8]
        if len(idx):
            out[name] = [(int(i), str(fx["tags"][tags[i]])) for i in idx]
    return out


def _oracle_material(oracle, row):
    m = np.zeros(1, oracle.MATERIAL)
    m["color"] = row[0:3]
    for k, f in enumerate(("hasReflective", "hasRefractive", "roughness", "metallic", "indexOfRefraction",
                           "emittance")):
        m[f] = row[3 + k]
    m["textureID"], m["bumpID"] = -1, -1
    return m


@functools.lru_cache(maxsize=None)
def oracle_scatter(trig_mode):
    import oracle
    fx = fixture()
    sc = fx["scatter_in"]
    o = oracle.options(trig_mode=trig_mode, arg_order=0)
    out = np.ascontiguousarray(sc["path"]).astype(oracle.PATH)
    L = oracle.lib()
    for i in range(len(sc)):
        m = _oracle_material(oracle, sc["material"][i])
        L.or_scatter(ctypes.byref(o), out[i:].ctypes.data, oracle.v3(sc["intersect"][i]), oracle.v3(sc["normal"][i]),
                     m.ctypes.data, int(sc["iter"][i]))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_shade(trig_mode):
    import oracle
    fx = fixture()
    sh = fx["shade_in"]
    scene = oracle.load_scene(SCENE)
    mm = scene.materials                      # the oracle's ingest of this scene == the reference's scene.cpp
    rows = np.column_stack([mm["color"]] + [mm[f] for f in ("hasReflective", "hasRefractive", "roughness", "metallic",
                                                            "indexOfRefraction", "emittance")]).astype(np.float32)
    assert rows.tobytes() == np.ascontiguousarray(fx["materials"]).tobytes()
    s = scene.c_struct()
    o = oracle.options(trig_mode=trig_mode, arg_order=0)
    out = np.ascontiguousarray(sh["path"]).astype(oracle.PATH)
    isect = np.ascontiguousarray(sh["isect"]).astype(oracle.ISECT)
    L = oracle.lib()
    for i in range(len(sh)):
        L.or_shade(ctypes.byref(s), ctypes.byref(o), int(sh["iter"][i]), isect[i:].ctypes.data, out[i:].ctypes.data)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# the stand-in RNG header
# ---------------------------------------------------------------------------------------------
STANDIN_PROGRAM = r'''
#include <thrust/random.h>
#include <cstdio>
#include <cstring>
int main() {   // "d <seed>": 8 u01 draws as u32 bits; "e <seed>": 4 raw engine values
    char mode; unsigned seed;
    while (std::scanf(" %c %u", &mode, &seed) == 2) {
        thrust::default_random_engine rng((int)seed);
        thrust::uniform_real_distribution<float> u01(0, 1);
        for (int j = 0; j < (mode == 'd' ? 8 : 4); ++j) {
            unsigned b; float f;
            if (mode == 'd') { f = u01(rng); std::memcpy(&b, &f, 4); } else b = rng();
            std::printf("%u ", b);
        }
        std::printf("\n");
    }
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_standin_rng_reproduces_rocthrust(tmp_path):
    """oracle/ref_pins/thrust_standin/thrust/random.h == rocThrust on every entry of rng_pin.json:
    all seeded cases (pathtrace.cu:51-56's hash as the seed, 8 draws, u32 bits) and the engine's edge
    seeds (0, m, 2m, 1, m - 1, 2^32 - 1; raw engine outputs)."""
    with open(os.path.join(GOLDEN, "rng_pin.json")) as f:
        pin = json.load(f)
    src = tmp_path / "standin.cpp"
    src.write_text(STANDIN_PROGRAM)
    exe = str(tmp_path / "standin")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(REPO, "oracle", "ref_pins", "thrust_standin"),
                    "-o", exe, str(src)], check=True)
    # the seed the reference computes is this hash (restated in refpins.utilhash, checked here too)
    for it, idx, d, h, _ in pin["cases"][::37]:
        key = np.array([0x80000000 | (d << 22) | it], np.uint32)
        assert int(R.utilhash(key)[0] ^ R.utilhash(np.array([idx], np.uint32))[0]) == h
    lines = ["d %d" % c[3] for c in pin["cases"]] + ["e %d" % e[0] for e in pin["engine"]]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    got = [[int(v) for v in ln.split()] for ln in out.splitlines()]
    want = [c[4] for c in pin["cases"]] + [e[1] for e in pin["engine"]]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:10], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------
# CPU: oracle against the reference fixture
# ---------------------------------------------------------------------------------------------
def test_oracle_scatter_matches_reference():
    """or_scatter(trig_mode=0, arg_order=0) == the reference's scatterRay on every record of every
    class (comparison rule in the module docstring)."""
    fx = fixture()
    bad = differing(oracle_scatter(0), fx["scatter_out"])
    assert len(bad) == 0, (len(bad), report(bad, fx["scatter_class"], fx["scatter_tag"], fx))


def test_oracle_shade_matches_reference():
    """or_shade(trig_mode=0, arg_order=0) on the scene loaded by the oracle == the reference's
    scatterRay behind its own scene.cpp and `intersect = origin + direction * t`."""
    fx = fixture()
    bad = differing(oracle_shade(0), fx["shade_out"])
    assert len(bad) == 0, (len(bad), report(bad, fx["shade_class"], fx["shade_tag"], fx))


def _lobes(fx):
    """Cook-Torrance lobe of each microfacet scatter record, from inputs alone: +1 microfacet,
    -1 diffuse, 0 where the first draw is within 1e-4 of Fprob or the inputs are not finite."""
    sc = fx["scatter_in"]
    m = sc["material"].astype(np.float64)
    d = sc["path"]["direction"].astype(np.float64)
    n = sc["normal"].astype(np.float64)
    with np.errstate(all="ignore"):
        wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
        cos = np.clip((n * wo).sum(axis=1), 0.0, 1.0)
        F0 = 0.04 + (m[:, 0:3] - 0.04) * m[:, 6:7]
        fprob = np.clip((F0 + (1.0 - F0) * ((1.0 - cos) ** 5)[:, None]).max(axis=1), 0.0, 1.0)
    state = R.rng_state(sc["iter"], sc["path"]["pixelIndex"], sc["path"]["remainingBounces"])
    choose = R.rng_draw(state, 1)[1].astype(np.float64)
    lobe = np.where(choose < fprob - 1e-4, 1, np.where(choose > fprob + 1e-4, -1, 0))
    lobe[~np.isfinite(fprob) | (fx["scatter_class"] != R.MICROFACET)] = 0
    return lobe


def test_fixture_covers_the_branches():
    """From the fixture's inputs and outputs alone: the edges it was built for are still in it."""
    fx = fixture()
    sc, out, cls = fx["scatter_in"], fx["scatter_out"], fx["scatter_class"]
    for mode_cls in (cls, fx["shade_class"]):
        assert set(np.unique(mode_cls)) == set(range(5))
        assert min(np.bincount(mode_cls, minlength=5)) >= 100
    assert set(np.unique(sc["iter"])) == set(R.BSDF_ITERS)            # three GPU launches, no more
    n, d_in, d_out = sc["normal"], sc["path"]["direction"], out["direction"]
    c_in, c_out = sc["path"]["color"], out["color"]
    unit_n = np.abs((n.astype(np.float64) ** 2).sum(axis=1) - 1) < 1e-3
    with np.errstate(all="ignore"):
        side_in = (n * d_in).sum(axis=1)
        side_out = (n * d_out).sum(axis=1)
    glass = (cls == R.GLASS) & unit_n & (np.abs(side_in) > 1e-3) & np.isfinite(side_out)
    assert (glass & (side_in * side_out < 0)).sum() >= 20, "glass never reflects"
    assert (glass & (side_in * side_out > 0)).sum() >= 20, "glass never refracts"
    # total internal reflection.  glm 0.9.6's refract multiplies its result by (k >= 0), so past the
    # critical angle it yields NaN, not 0: `length(wiW) < BABY_EPSILON` is false, neither fallback of
    # interactions.cu:161-165 / :226-230 runs, and the path leaves with a NaN direction and its
    # colour multiplied by the albedo.  That is the reference's TIR, and what is pinned here.
    sane = unit_n & np.isfinite(d_in).all(axis=1) & np.isfinite(sc["intersect"]).all(axis=1)
    tir = np.isin(cls, (R.TRANSMISSIVE, R.GLASS)) & sane & (side_in > 0) & np.isnan(d_out).all(axis=1)
    assert tir.sum() >= 10, "no total internal reflection"
    assert not (np.isin(cls, (R.TRANSMISSIVE, R.GLASS)) & sane & (side_in < 0) & np.isnan(d_out).any(axis=1)
                & (sc["material"][:, 7] >= 1)).any(), "TIR while entering"
    crit = np.char.startswith(fx["tags"][fx["scatter_tag"]], "critical angle") & (side_in > 0)
    for ior in (1.5, 2.4):
        k = crit & (sc["material"][:, 7] == np.float32(ior))
        kt = k & (cls == R.TRANSMISSIVE)
        assert (kt & tir).sum() >= 8 and (kt & ~tir).sum() >= 8, ("the sweep no longer crosses the critical angle", ior)
        # glass never gets that far: past the critical angle FresnelDielectricEval is exactly 1 and
        # `random < fresnel` reflects (a draw of exactly 1.0 aside), so its sweep reflects and stays finite
        kg = k & (cls == R.GLASS)
        assert kg.sum() >= 16 and np.isfinite(d_out[kg]).all() and (side_in * side_out < 0)[kg].sum() >= 8, ior
    lobe = _lobes(fx)
    assert (lobe == 1).sum() >= 100 and (lobe == -1).sum() >= 100, ((lobe == 1).sum(), (lobe == -1).sum())
    # `if (pdf > 0)` not taken: a live colour that no factor touched
    micro_live = (cls == R.MICROFACET) & np.isfinite(c_in).all(axis=1) & (c_in != 1).all(axis=1) & (c_in > 0).all(axis=1)
    assert (micro_live & (_words(out)[:, 6:9] == _words(sc["path"])[:, 6:9]).all(axis=1)).sum() >= 1, "pdf <= 0 never seen"
    finite_in = np.isfinite(c_in).all(axis=1)
    assert (finite_in & ~np.isfinite(c_out).all(axis=1) & (cls == R.DIFFUSE)).sum() >= 1, "no pdf == 0 diffuse sample"
    assert (~np.isfinite(c_out).all(axis=1)).sum() >= 10
    # normals: coordinateSystem's branch on both sides and on the tie, 0/0, non-unit, NaN
    ax, ay = np.abs(n[:, 0]), np.abs(n[:, 1])
    trig = np.isin(cls, (R.DIFFUSE, R.MICROFACET))
    for name, sel in (("|x| == |y|", (ax == ay) & (ax > 0)), ("|x| one ulp above |y|", ax == np.nextafter(ay, np.float32(2))),
                      ("|x| one ulp below |y|", (ax == np.nextafter(ay, np.float32(0))) & (ay > 0)),
                      ("(0, 0, +-1)", (ax == 0) & (ay == 0) & (np.abs(n[:, 2]) == 1)), ("zero normal", (n == 0).all(axis=1)),
                      ("NaN normal", np.isnan(n).any(axis=1)),
                      ("short normal", np.abs((n.astype(np.float64) ** 2).sum(axis=1) - 0.25) < 1e-3),
                      ("long normal", np.abs((n.astype(np.float64) ** 2).sum(axis=1) - 4) < 1e-3)):
        assert (sel & trig).sum() >= 2, name
    # directions: along +-n, perpendicular, grazing, back-facing for every class, non-unit
    dl = np.sqrt((d_in.astype(np.float64) ** 2).sum(axis=1))
    for c in range(5):
        k = cls == c
        assert (k & (side_in > 1e-3) & unit_n).sum() >= 4, ("back-facing", c)
        assert (k & (side_in == 0) & unit_n & (dl > 0.5)).sum() >= 1, ("perpendicular", c)
        assert (k & (np.abs(side_in) > 0) & (np.abs(side_in) <= 2.0 ** -10) & (np.abs(side_in) >= 2.0 ** -25)).sum() >= 4, ("grazing", c)
        assert (k & ((dl < 0.6) | (dl > 1.9))).sum() >= 2, ("non-unit direction", c)
        assert (k & unit_n & (np.abs(np.abs(side_in) - 1) < 1e-6) & (np.abs(dl - 1) < 1e-6)).sum() >= 2, ("along n", c)
    # searched seeds: a draw exactly 0, exactly 1, next to Fprob on both sides, a^2 == b^2
    state = R.rng_state(sc["iter"], sc["path"]["pixelIndex"], sc["path"]["remainingBounces"])
    u = np.stack([R.rng_draw(state, j)[1] for j in (1, 2, 3)], axis=1)
    micro = cls == R.MICROFACET
    assert (micro & (u[:, 2] == 1)).any() and (micro & (u[:, 2] == 0)).any(), "xi[0] in {0, 1} (third draw) missing"
    assert ((cls == R.DIFFUSE) & ((u[:, 0:2] == 1) | (u[:, 0:2] == 0)).any(axis=1)).any()
    tags = fx["tags"][fx["scatter_tag"]]
    assert np.char.startswith(tags, "choose -").sum() >= 20 and np.char.startswith(tags, "choose +").sum() >= 20
    a, b = np.float32(2) * u[:, 1] - np.float32(1), np.float32(2) * u[:, 0] - np.float32(1)
    assert ((cls == R.DIFFUSE) & (a * a == b * b)).any(), "a^2 == b^2 missing"
    # materials, throughput, bounces, pixel indices
    mats = fx["materials"]
    micro_m = mats[R.bsdf_class(mats) == R.MICROFACET]
    assert {(float(r), float(m)) for r, m in micro_m[:, 5:7]} == {(float(np.float32(r)), m) for r in (0, 0.001, 0.05, 0.5, 1)
                                                                 for m in (0.0, 0.5, 1.0)}
    for c in (R.TRANSMISSIVE, R.GLASS):
        assert sorted(float(v) for v in mats[R.bsdf_class(mats) == c][:, 7]) == [1.0, 1.5, float(np.float32(2.4))]
    assert (mats[:, 0:3] == 0).any() and (mats[:, 0:3] == 1).any() and (mats[:, 0:3] > 1).any()
    for c in range(5):
        k = cls == c
        assert (k & (c_in == 0).all(axis=1)).any() and (k & (c_in > 1).all(axis=1)).any()
        assert (k & np.isinf(c_in).any(axis=1)).any() and (k & np.isnan(c_in).any(axis=1)).any()
        assert {1, 8, 12} <= set(sc["path"]["remainingBounces"][k]) and {0, 639999, 2559999} <= set(sc["path"]["pixelIndex"][k])


def _vec_ulps(got, want, field):
    """Per record: largest |difference| of `field` in ulps of the fixture vector's largest
    component, and whether a component is finite on one side only (or the infinities differ)."""
    x, y = got[field].astype(np.float64), want[field].astype(np.float64)
    fin = np.isfinite(x) & np.isfinite(y)
    same = (got[field].view(np.uint32) == want[field].view(np.uint32)) | (np.isnan(x) & np.isnan(y))
    kind = (~fin & ~same).any(axis=1)
    mag = np.where(np.isfinite(y), np.abs(y), 0).max(axis=1).astype(np.float32)
    ulp = np.spacing(np.maximum(mag, np.float32(1e-37))).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(x - y), 0).max(axis=1) / ulp, kind


def check_portable_against_fixture(got, want, cls, tags, fx, who):
    """The trig_mode=1 contract against the reference fixture (figures at the top of the module)."""
    trig_free = np.isin(cls, TRIG_FREE)
    bad = differing(got, want)
    bad = bad[trig_free[bad]]
    assert len(bad) == 0, (who, len(bad), report(bad, cls, tags, fx))
    assert (_words(got)[:, 9:] == _words(want)[:, 9:]).all(), who      # pixelIndex, remainingBounces
    rim = np.char.startswith(fx["tags"][tags], "u01 ==") & ~trig_free
    plain = ~trig_free & ~rim
    d_dir, k_dir = _vec_ulps(got, want, "direction")
    d_org, k_org = _vec_ulps(got, want, "origin")
    d_col, k_col = _vec_ulps(got, want, "color")
    with np.errstate(invalid="ignore"):
        delta = np.nan_to_num(np.abs(got["direction"].astype(np.float64) - want["direction"]), nan=0.0, posinf=0.0).max(axis=1)
    flipped = plain & (delta > FLIP_DIRECTION_DELTA)
    figures = dict(who=who, plain=int(plain.sum()), rim=int(rim.sum()), flips=int(flipped.sum()),
                   dir=float(d_dir[plain & ~flipped].max()), origin=float(d_org[plain & ~flipped].max()),
                   color=float(d_col[plain & ~flipped].max()), rim_dir=float(d_dir[rim].max()),
                   rim_color_kind=int((k_col & rim).sum()))
    print(figures)
    assert flipped.sum() <= FLIP_CAP * (~trig_free).sum(), figures
    ok = plain & ~flipped
    assert not (k_dir | k_org | k_col)[ok].any(), (figures, np.flatnonzero((k_dir | k_org | k_col) & ok)[:8])
    assert figures["dir"] <= 2 * MEASURED_DIR_ULPS and figures["origin"] <= 2 * MEASURED_DIR_ULPS, figures
    assert figures["color"] <= 2 * MEASURED_COLOR_ULPS, figures
    assert not (k_dir | k_org)[rim].any(), figures
    assert figures["rim_dir"] <= 2 * MEASURED_RIM_DIR_ULPS, figures
    assert figures["rim_color_kind"] <= MEASURED_RIM_COLOR_KIND_MISMATCHES, figures
    return figures


def test_portable_trig_stays_close_to_reference():
    """trig_mode=1 (pt_libm sin / cos / pow5, what the GPU is bit-exact with) against the fixture.
    Reflective, transmissive and glass records are byte-equal.  Diffuse and microfacet records,
    measured: direction within 10.875 and colour within 25 ulps of the vector's largest component,
    0 lobe flips (cap: 1 % of those records); the 294 rim records within 5016.6 ulps in direction
    (see the constants above).  The assertions use twice the measured ulp figures, so only a change
    of pt_libm moves them."""
    fx = fixture()
    sc = check_portable_against_fixture(oracle_scatter(1), fx["scatter_out"], fx["scatter_class"], fx["scatter_tag"], fx,
                                        "scatter")
    sh = check_portable_against_fixture(oracle_shade(1), fx["shade_out"], fx["shade_class"], fx["shade_tag"], fx, "shade")
    assert sc["flips"] == 0 and sh["flips"] == 0      # measured: the near-Fprob seeds were chosen to keep it so


# ---------------------------------------------------------------------------------------------
# GPU: the kernel against the reference fixture
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_shade_matches_reference_pin(ptamd):
    """k_shade on the fixture's `shade` inputs, one launch per iteration.  Reflective, transmissive
    and glass records equal the reference FIXTURE (no oracle in between); diffuse and microfacet
    records equal or_shade(trig_mode=1) on these edge inputs and keep its measured distance to the
    fixture.  Comparison rule in the module docstring (the GPU's NaNs carry its own sign bit)."""
    fx = fixture()
    sh, cls, tags = fx["shade_in"], fx["shade_class"], fx["shade_tag"]
    scene = ptamd.SceneFile(SCENE, res=(80, 80))                      # wavefront capacity >= 6400 paths
    assert len(scene.materials) == len(fx["materials"]) and int(sh["isect"]["materialId"].max()) < len(scene.materials)
    tr = ptamd.PathTracer(scene)
    got = np.zeros(len(sh), ptamd.PATH)
    isect = np.ascontiguousarray(sh["isect"]).astype(ptamd.ISECT)
    paths = np.ascontiguousarray(sh["path"]).astype(ptamd.PATH)
    try:
        for it in R.BSDF_ITERS:
            k = np.flatnonzero(sh["iter"] == it)
            assert 0 < len(k) <= 6400
            got[k] = tr.test_shade(it, isect[k], paths[k])
    finally:
        tr.free()
    trig_free = np.isin(cls, TRIG_FREE)
    bad = differing(got, fx["shade_out"])
    bad = bad[trig_free[bad]]
    assert len(bad) == 0, ("GPU != reference", len(bad), report(bad, cls, tags, fx))
    bad = differing(got, oracle_shade(1))
    assert len(bad) == 0, ("GPU != or_shade(trig_mode=1)", len(bad), report(bad, cls, tags, fx))
    check_portable_against_fixture(got.astype(R.P_PATH), fx["shade_out"], cls, tags, fx, "gpu shade")
