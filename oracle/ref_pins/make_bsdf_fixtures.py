"""Writes tests/golden/bsdf_pin.npz from the reference's OWN scatterRay (TEST INFRASTRUCTURE).

Runs oracle/_ref/bsdf_pin (oracle/ref_pins/bsdf_pin.cpp linked with the reference's interactions.cu,
built by make_fixtures.sh) over deterministic inputs that sit on the edges of the shading code, not
on its workload: degenerate / non-unit / NaN normals, coordinateSystem's |x| == |y| branch,
directions along, against and perpendicular to the normal, the critical angle of every
refractive material ulp by ulp, and RNG seeds searched so that a draw lands next to Fprob, on
exactly 0 or exactly 1, or gives a^2 == b^2 in the concentric map.  Every case is written for both
harness modes: `shade` (scene material, intersect formed by the harness) and `scatter` (explicit
material and intersect), which also takes a few materials no scene file can express.

Usage: python oracle/ref_pins/make_bsdf_fixtures.py <harness> <scene.json> <out.npz> "<flags>"
"""
import ctypes
import io
import json
import os
import platform
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import refpins as R  # noqa: E402

f32 = np.float32
ITERS = R.BSDF_ITERS
DEPTHS = tuple(range(1, 13))
SEARCH_INDICES = 1 << 22          # pixel indices searched per (iter, depth) key
ZERO_SEARCH_INDICES = 1 << 28     # wider scan for the 1-in-2^31 engine value that gives u01 == 0


def unit(v):
    v = np.asarray(v, f32)
    return (v / np.sqrt((v * v).sum(dtype=f32), dtype=f32)).astype(f32)


def tangent(n):
    n = np.asarray(n, np.float64)
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.6 else np.array([0, 1.0, 0])
    t = np.cross(n, a)
    return t / np.linalg.norm(t)


class Cases:
    def __init__(self, materials):
        self.materials = materials
        self.cls = R.bsdf_class(materials)
        self.rows = []
        self.k = 0

    def ids(self, c):
        return [int(i) for i in np.flatnonzero(self.cls == c)]

    def add(self, mat, n, d, tag, color=None, rb=None, pix=None, it=None, t=None, origin=None, material=None):
        k = self.k
        self.k += 1
        u = R._u(1000 + k, 1, 8)[0]
        if color is None:
            color = (f32(0.1) + u[0:3] * f32(0.9)).astype(f32)
        if rb is None:
            rb = (1, 8, 12, 2, 5, 7)[k % 6]
        if pix is None:
            pix = (0, 639999, 2559999)[k % 3] if k % 11 == 0 else int(u[3] * f32(2560000))
        if it is None:
            it = ITERS[k % 3]
        if t is None:
            t = f32(0.5) + u[4] * f32(7.5)
        if origin is None:
            origin = (u[5:8] * f32(10) - f32(5)).astype(f32)
        self.rows.append(dict(mat=mat, n=np.asarray(n, f32), d=np.asarray(d, f32), tag=tag, color=np.asarray(color, f32),
                              rb=int(rb), pix=int(pix), it=int(it), t=f32(t), origin=np.asarray(origin, f32),
                              material=material))


def random_pair(seed, front=True):
    u = R._u(seed, 1, 6)[0] * f32(2) - f32(1)
    n, d = unit(u[0:3] + f32(1e-3)), unit(u[3:6] + f32(1e-3))
    if (np.dot(n, d) > 0) == front:
        d = -d
    return n, d


def fprob(material, n, d, powf):
    """sampleFCookTorrance's Fprob (interactions.cu:395-400) in float32, powf from glibc."""
    color, metallic = material[0:3].astype(f32), f32(material[6])
    F0 = (f32(0.04) + (color - f32(0.04)) * metallic).astype(f32)
    inv = f32(1) / np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), dtype=f32)
    wo = -(d * inv).astype(f32)
    c = f32(f32(n[0] * wo[0] + n[1] * wo[1]) + n[2] * wo[2])
    c = min(max(c, f32(0)), f32(1))
    p = f32(powf(f32(1) - c, f32(5)))
    F = (F0 + (f32(1) - F0) * p).astype(f32)
    return min(max(f32(F.max()), f32(0)), f32(1))


def search_seeds(probes):
    """One pass over every (iter, depth, index < SEARCH_INDICES) seed.  Returns
    near[probe] -> [(iter, depth, index)] whose first draw is within 4 ulps of the probe's Fprob,
    one[j] -> seeds whose j-th draw (1..3) is exactly 1.0, sq -> seeds with a^2 == b^2."""
    idx = np.arange(SEARCH_INDICES, dtype=np.uint32)
    hidx = R.utilhash(idx)
    bits = np.array([np.float32(p).view(np.int32) for p in probes], np.int64)
    want = np.unique((bits[:, None] + np.arange(-4, 5)[None, :]).ravel()).astype(np.int32)
    near = {i: [] for i in range(len(probes))}
    one = {1: [], 2: [], 3: []}
    sq = []
    for it in ITERS:
        for dp in DEPTHS:
            key = np.uint32(0x80000000 | (dp << 22) | it)
            x0 = (R.utilhash(np.array([key], np.uint32))[0] ^ hidx).astype(np.uint64) % np.uint64(R.RNG_M)
            x0[x0 == 0] = 1
            us = {}
            for j in (1, 2, 3):
                x, u = R.rng_draw(x0, j)
                us[j] = u
                for i in np.flatnonzero(u == 1):
                    one[j].append((it, dp, int(i)))
            b1 = us[1].view(np.int32)
            for i in np.flatnonzero(np.isin(b1, want)):
                for p in np.flatnonzero(np.abs(bits - int(b1[i])) <= 4):
                    near[int(p)].append((it, dp, int(i), int(b1[i]) - int(bits[p])))
            a = f32(2) * us[2] - f32(1)          # xi = (second draw, first draw) under g++'s argument order
            b = f32(2) * us[1] - f32(1)
            for i in np.flatnonzero(a * a == b * b)[:2]:
                sq.append((it, dp, int(i)))
    return near, one, sq


def search_zero_draws():
    """Seeds whose j-th draw (1..3) is exactly 0: engine value 1, i.e. state A^-j mod m."""
    targets = {}
    keys = [(it, dp) for it in ITERS for dp in DEPTHS]
    hk = R.utilhash(np.array([0x80000000 | (dp << 22) | it for it, dp in keys], np.uint32))
    for j in (1, 2, 3):
        x0 = pow(pow(R.RNG_A, j, R.RNG_M), -1, R.RNG_M)
        for h in (x0, x0 + R.RNG_M):
            for (it, dp), k in zip(keys, hk):
                targets[int(np.uint32(h) ^ k)] = (j, it, dp)
    want = np.array(sorted(targets), np.uint32)
    out = {1: [], 2: [], 3: []}
    step = 1 << 22
    for lo in range(0, ZERO_SEARCH_INDICES, step):
        h = R.utilhash(np.arange(lo, lo + step, dtype=np.uint32))
        for i in np.flatnonzero(np.isin(h, want)):
            j, it, dp = targets[int(h[i])]
            out[j].append((it, dp, lo + int(i)))
    return out


def build_cases(materials):
    C = Cases(materials)
    powf = ctypes.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    every = list(range(len(materials)))
    by = {c: C.ids(c) for c in range(5)}
    one_each = [by[c][k % len(by[c])] for c in range(5) for k in range(2)]
    seed = [0]

    def nxt():
        seed[0] += 1
        return seed[0]

    # ---- a few hundred ordinary front-facing hits per class -----------------------------------
    for c in range(5):
        for k in range(120):
            n, d = random_pair(nxt())
            C.add(by[c][k % len(by[c])], n, d, "random")
    # ---- normals ---------------------------------------------------------------------------------
    ax = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    normals = [np.array(a, f32) for a in ax] + [np.array((0, 0, 0), f32), np.array((-0.0, 0.0, -1.0), f32)]
    for sx, sy in ((1, 1), (1, -1), (-1, 1)):
        a = f32(0.57735026)
        for z in (f32(0.57735026), f32(0.0), f32(-0.8)):
            base = np.array((sx * a, sy * a, z), f32)
            normals.append(base)                                      # |n.x| == |n.y| exactly
            for tow in (f32(0), f32(1)):                              # and one ulp either side
                m = base.copy()
                m[0] = np.nextafter(m[0], tow)
                normals.append(m)
    for k in range(4):
        n, _ = random_pair(nxt())
        normals += [(n * f32(0.5)).astype(f32), (n * f32(2)).astype(f32)]    # interpolated mesh normals
    for k in range(3):
        n, _ = random_pair(nxt())
        n[k] = np.nan
        normals.append(n)
    norm_mats = one_each[:8] + by[R.MICROFACET][0::4] + by[R.MICROFACET][1::4][:2]
    for n in normals:
        for m in norm_mats:
            _, d = random_pair(nxt())
            if np.isfinite(n).all() and np.dot(n, d) > 0:
                d = -d
            C.add(m, n, d, "normal-edge")
    # ---- directions ------------------------------------------------------------------------------
    bases = [np.array((0, 1, 0), f32), unit((1, 1, 0)), unit((0.3, -0.5, 0.81))]
    for bi, n in enumerate(bases):
        tn = tangent(n).astype(f32)
        dirs = [(-n, "along -n"), (n.copy(), "along +n"), (tn, "perpendicular"), (-tn, "perpendicular")]
        for e in range(10, 25, 2):
            for sg in (1, -1):
                dirs.append(((tn + n * f32(sg * 2.0 ** -e)).astype(f32), "grazing 2^-%d" % e))
        for k in range(4):
            _, d = random_pair(nxt())
            if np.dot(n, d) < 0:
                d = -d
            dirs.append((d, "back-facing"))
        for s in (0.5, 2.0, 1e-3, 1e3):
            _, d = random_pair(nxt())
            if np.dot(n, d) > 0:
                d = -d
            dirs.append(((d * f32(s)).astype(f32), "non-unit direction"))
        for d, tag in dirs:
            for m in (every if bi == 0 else one_each):
                C.add(m, n, d, tag)
    # exact grazing on an axis normal: dot(d, n) is exactly +-2^-e
    for e in range(10, 25):
        for sg in (1, -1):
            for m in one_each:
                C.add(m, (0, 1, 0), (1.0, sg * 2.0 ** -e, 0.0), "grazing exact 2^-%d" % e)
    # ---- transmissive / glass across the critical angle, from inside (dot(d, n) > 0) ----------------
    for m in by[R.TRANSMISSIVE] + by[R.GLASS]:
        ior = f32(materials[m][7])
        if not ior > 1:
            continue
        cc = np.sqrt(f32(1) - f32(1) / (ior * ior), dtype=f32)
        for n in (np.array((0, 1, 0), f32), unit((0.3, -0.5, 0.81))):
            tn = tangent(n).astype(f32)
            for step in range(-12, 13):
                c = cc
                for _ in range(abs(step)):
                    c = np.nextafter(c, f32(2) if step > 0 else f32(0))
                s = np.sqrt(f32(1) - c * c, dtype=f32)
                C.add(m, n, (n * c + tn * s).astype(f32), "critical angle %+d ulp" % step)
                if step % 4 == 0:    # entering from outside at the same angle (never TIR)
                    C.add(m, n, (-n * c + tn * s).astype(f32), "critical angle, outside")
    # ---- throughput in ---------------------------------------------------------------------------
    for col in ((0, 0, 0), (1, 1, 1), (2, 3, 4), (np.inf, 1, 1), (1, np.nan, 1), (0, np.inf, 0.5)):
        for m in every:
            n, d = random_pair(nxt())
            C.add(m, n, d, "throughput edge", color=col)
    # ---- searched seeds --------------------------------------------------------------------------
    probes, probe_case = [], []
    for m in by[R.MICROFACET]:
        n, d = np.array((0, 1, 0), f32), np.array((0, -1, 0), f32)      # cosTheta == 1: Fprob == max(F0)
        probes.append(fprob(materials[m], n, d, powf))
        probe_case.append((m, n, d))
    for k, m in enumerate(by[R.MICROFACET]):
        n, d = random_pair(nxt())
        probes.append(fprob(materials[m], n, d, powf))
        probe_case.append((m, n, d))
    near, one, sq = search_seeds(probes)
    zero = search_zero_draws()
    stats = {"near_fprob": 0, "draw_is_one": {j: len(v) for j, v in one.items()},
             "draw_is_zero": {j: len(v) for j, v in zero.items()}, "a2_eq_b2": len(sq),
             "xi_zero_zero": "impossible: u01 == 0 needs engine value 1, and 48271 * 1 mod m != 1"}
    for p, (m, n, d) in enumerate(probe_case):
        seen = set()
        for it, dp, ix, off in sorted(near[p], key=lambda s: (s[3], s[0], s[1], s[2])):
            if off in seen:
                continue
            seen.add(off)
            C.add(m, n, d, "choose %+d ulp of Fprob" % off, it=it, rb=dp, pix=ix)
            stats["near_fprob"] += 1
    micro_sure = [m for m in by[R.MICROFACET] if materials[m][6] == 1 and materials[m][0:3].max() >= 1]   # Fprob == 1
    lists = [(one, "u01 == 1"), (zero, "u01 == 0")]
    for found, tag in lists:
        for j in (1, 2, 3):
            for it, dp, ix in found[j][:4]:
                for k in range(2):
                    n, d = (np.array((0, 1, 0), f32), unit((0.6, -0.8, 0))) if k == 0 else random_pair(nxt())
                    for m in micro_sure + by[R.MICROFACET][3:12:4]:
                        C.add(m, n, d, "%s at draw %d" % (tag, j), it=it, rb=dp, pix=ix)
                    for m in by[R.DIFFUSE][:2] + by[R.GLASS][1:2]:
                        C.add(m, n, d, "%s at draw %d" % (tag, j), it=it, rb=dp, pix=ix)
    for it, dp, ix in sq[:24]:
        n, d = random_pair(nxt())
        C.add(by[R.DIFFUSE][0], n, d, "a^2 == b^2", it=it, rb=dp, pix=ix)
        C.add(by[R.MICROFACET][0], n, d, "a^2 == b^2", it=it, rb=dp, pix=ix)
    # ---- materials only `scatter` can express ------------------------------------------------------
    extra = []
    for row in ((0.5, 0.5, 0.5, 0, 0, 0.3, -1, 1.5, 0),          # roughness without metallic: diffuse
                (0.5, 0.5, 0.5, 0, 0, -0.0, 0.0, 1.5, 0),         # -0 >= 0: microfacet
                (0.5, 0.5, 0.5, 0, 0, np.nan, 0.5, 1.5, 0),       # NaN roughness: diffuse
                (0.5, 0.5, 0.5, 1e-30, 0, 0.5, 0.5, 1.5, 0),      # any positive hasReflective: mirror
                (0.5, 0.5, 0.5, 0.5, 2.0, -1, -1, 1.5, 5.0),      # emittance is not scatterRay's business
                (0.9, 0.9, 0.9, 0, 1, -1, -1, 0.5, 0),            # IOR below 1
                (0.9, 0.9, 0.9, 1, 1, -1, -1, 0.0, 0),            # IOR 0: 1 / IOR is inf
                (0.9, 0.8, 0.7, 0, 0, 2.0, 1.5, 1.5, 0)):         # roughness, metallic above 1
        extra.append(np.array(row, f32))
    for mrow in extra:
        for k in range(12):
            n, d = random_pair(nxt(), front=(k % 4 != 3))
            C.add(-1, n, d, "scatter-only material", material=mrow)
    return C, stats


def assemble(C):
    rows = C.rows
    n = len(rows)
    sc = np.zeros(n, R.P_SCATTER_IN)
    tags = []
    for i, r in enumerate(rows):
        p = sc["path"][i:i + 1]
        p["origin"], p["direction"], p["color"] = r["origin"], r["d"], r["color"]
        p["pixelIndex"], p["remainingBounces"] = r["pix"], r["rb"]
        sc["material"][i] = C.materials[r["mat"]] if r["mat"] >= 0 else r["material"]
        sc["intersect"][i] = (r["origin"] + (r["d"] * r["t"]).astype(f32)).astype(f32)
        sc["normal"][i] = r["n"]
        sc["iter"][i] = r["it"]
        tags.append(r["tag"])
    keep = np.array([r["mat"] >= 0 for r in rows])
    sh = np.zeros(int(keep.sum()), R.P_SHADE_IN)
    sh["path"] = sc["path"][keep]
    sh["iter"] = sc["iter"][keep]
    sh["isect"]["t"] = np.array([r["t"] for r in rows], f32)[keep]
    sh["isect"]["surfaceNormal"] = sc["normal"][keep]
    sh["isect"]["materialId"] = np.array([r["mat"] for r in rows], np.int32)[keep]
    return sc, sh, tags, keep


def run_harness(harness, scene, sc, sh):
    with tempfile.TemporaryDirectory() as tmp:
        a, b, c, d = (os.path.join(tmp, x) for x in ("sc.in", "sc.out", "sh.in", "sh.out"))
        sc.tofile(a)
        sh.tofile(c)
        subprocess.run([harness, "scatter", a, b], check=True, stdout=subprocess.DEVNULL)
        subprocess.run([harness, "shade", scene, c, d], check=True, stdout=subprocess.DEVNULL)
        return np.fromfile(b, R.P_PATH), np.fromfile(d, R.P_PATH)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so two runs give identical bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    harness, scene, out_path, flags = sys.argv[1:5]
    txt = subprocess.run([harness, "materials", scene], check=True, capture_output=True, text=True).stdout
    lines = txt[txt.index("BSDF_PIN_MATERIALS"):].splitlines()
    materials = np.array([[float(v) for v in ln.split()] for ln in lines[1:1 + int(lines[0].split()[1])]], f32)
    C, stats = build_cases(materials)
    sc, sh, tags, keep = assemble(C)
    sc_out, sh_out = run_harness(harness, scene, sc, sh)
    assert len(sc_out) == len(sc) and len(sh_out) == len(sh)
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    meta = {"generator": "oracle/ref_pins/make_bsdf_fixtures.py", "harness": "oracle/ref_pins/bsdf_pin.cpp",
            "scene": "tests/golden/bsdf_pin_scene.json", "g++": gxx, "glibc": " ".join(platform.libc_ver()),
            "flags": flags, "records": {"scatter": len(sc), "shade": len(sh)}, "searched_seeds": stats,
            "seed_search": {"iters": ITERS, "depths": [DEPTHS[0], DEPTHS[-1]], "indices": SEARCH_INDICES,
                            "zero_draw_indices": ZERO_SEARCH_INDICES}}
    utags = sorted(set(tags))
    tag_id = np.array([utags.index(t) for t in tags], np.uint16)
    save_npz(out_path, {
        "materials": materials, "scatter_in": sc, "scatter_out": sc_out, "scatter_tag": tag_id, "tags": np.array(utags),
        # the shade inputs share path / normal / iter with the scatter record `shade_index` names
        # (tests/refpins.bsdf_shade_inputs rebuilds them), which keeps the file small
        "shade_index": np.flatnonzero(keep).astype(np.int32), "shade_t": sh["isect"]["t"],
        "shade_material": sh["isect"]["materialId"], "shade_out": sh_out,
        "meta": np.array(json.dumps(meta, sort_keys=True))})
    print("bsdf fixture:", out_path, len(sc), "scatter /", len(sh), "shade records,", os.path.getsize(out_path), "bytes")
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
