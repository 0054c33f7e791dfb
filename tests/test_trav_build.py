"""The SAH traversal hierarchy built on the device (include/pt/pt_trav_build.h, csrc/pt_trav_build.hip):
the interface without a GPU, and on one the device's tree against the host's, byte for byte."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path

INVALID, NODEVICE = -1, -4


def _leaves(shape, n, seed=7):
    """n leaf boxes (lo, hi, s) and the max_height that goes with the shape."""
    g = np.random.default_rng(seed + n)
    s = g.random(n, dtype=np.float32)
    if shape == "equal":                       # one centroid (eighths are exact): the index-order halving
        r = (g.integers(0, 8, (n, 1)) / 8).astype(np.float32)
        return np.float32([1, 2, 3]) - r, np.float32([1, 2, 3]) + r, s, 1 << 30
    if shape == "expo":                        # lopsided SAH splits under the tightest height bound: the median
        lo = np.stack([2.0 ** (g.permutation(n) * (40.0 / n)) for _ in range(3)], 1).astype(np.float32)
        hi = (lo * np.float32(1.001)).astype(np.float32)
        assert all(len(np.unique(lo[:, a].astype(np.float64) + hi[:, a])) == n for a in range(3))   # distinct centroids
        return lo, hi, s, 1 + int(np.ceil(np.log2(n)))
    lo = (g.random((n, 3), dtype=np.float32) * 100 - 50).astype(np.float32)
    hi = (lo + g.random((n, 3), dtype=np.float32) * 3).astype(np.float32)
    if shape == "plane":                       # one axis without extent
        lo[:, 1] = hi[:, 1] = np.float32(0.25)
    return lo, hi, s, 1 << 30


def test_interface_without_a_device(ptamd):
    header = open(os.path.join(REPO, "include", "pt", "pt_trav_build.h")).read()
    names = re.findall(r"^(?:int32_t|const char\*) (pt_\w+)\(", header, re.M)
    assert names == ptamd.TRAV_BUILD_SYMBOLS and all(getattr(ptamd.lib, n).argtypes is not None for n in names)
    assert "trav_build" not in open(os.path.join(REPO, "include", "pt", "pathtrace_abi.h")).read()
    piece, subt = (int(re.search(r"#define %s (\d+)" % k, header).group(1))
                   for k in ("PT_TRAV_BUILD_PIECE", "PT_TRAV_BUILD_SUBTREE"))
    assert (piece, subt) == (ptamd.TRAV_BUILD_PIECE, ptamd.TRAV_BUILD_SUBTREE) and ptamd.TRAV_INNER.itemsize == 72
    ptamd.lib.pt_free()
    prev = ptamd.get_trav_build()[:2]
    try:
        ptamd.set_trav_build(True)
        default = ptamd.get_trav_build()[1]
        assert ptamd.get_trav_build() == (True, default, False) and default > 1      # no context: inactive
        ptamd.set_trav_build(True, 12)
        ptamd.lib.pt_free()
        assert ptamd.get_trav_build() == (True, 12, False)                           # sticky
        assert ptamd.lib.pt_get_trav_build(None, None, None) == 0
        ptamd.set_trav_build(False, -3)
        assert ptamd.get_trav_build() == (False, default, False)
    finally:
        ptamd.set_trav_build(*prev)
    lo, hi, s, _ = _leaves("uniform", 33)
    tree, height = ptamd.trav_build(lo, hi, s)
    kids = tree["c"].reshape(-1)
    assert len(tree) == 32 and 7 <= height <= 33
    assert sorted(kids["ref"][kids["leaf"] == 1]) == list(range(33))                 # every leaf exactly once
    assert sorted(kids["ref"][kids["leaf"] == 0]) == list(range(1, 32))              # every node but the root
    import torch
    if torch.cuda.device_count() == 0:
        with pytest.raises(ptamd.PtError) as e:
            ptamd.trav_build(lo, hi, s, where="gpu")
        assert e.value.code == NODEVICE


SIZES = [2, 3, 31, 33, 257]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["uniform", "plane", "expo", "equal"])
def test_device_tree_is_the_hosts_tree(shape, ptamd):
    """Sizes: the small ones, one just above a piece (two pieces, level kernels) and one above the
    in-LDS subtree threshold over three pieces; every numbering."""
    sizes = [5] if shape == "equal" else SIZES + [ptamd.TRAV_BUILD_PIECE + 3,
                                                  max(ptamd.TRAV_BUILD_SUBTREE, 2 * ptamd.TRAV_BUILD_PIECE) + 5]
    for n in sizes:
        lo, hi, s, max_height = _leaves(shape, n)
        for bfs in (0, 3, 1 << 30):
            want, wh = ptamd.trav_build(lo, hi, s, "host", bfs, max_height)
            got, gh = ptamd.trav_build(lo, hi, s, "gpu", bfs, max_height)
            assert (len(got), gh) == (len(want), wh) == (n - 1, wh), (shape, n, bfs)
            assert got.tobytes() == want.tobytes(), (shape, n, bfs, np.flatnonzero(got != want)[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one-leaf", "nan", "inverted"])
def test_rejections_agree(case, ptamd):
    lo, hi, s, _ = _leaves("uniform", 1 if case == "one-leaf" else 40)
    if case == "nan":
        hi[17, 2] = np.nan
    if case == "inverted":
        lo[5, 0] = hi[5, 0] + 1
    codes = []
    for where in ("host", "gpu"):
        with pytest.raises(ptamd.PtError) as e:
            ptamd.trav_build(lo, hi, s, where)
        codes.append(e.value.code)
    assert codes == [INVALID, INVALID]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, 2], ids=["records4", "records8"])
def test_pt_init_on_the_device_tree(wide, ptamd):
    sc = ptamd.SceneFile(scene_path("cornell_obj_bnnuy"), res=(48, 48), depth=8)
    runs = []
    for on in (False, 2):
        tr = ptamd.PathTracer(sc, trav_build=on, bvh_wide=wide)
        try:
            assert ptamd.get_trav_build() == (False, ptamd.get_trav_build()[1], bool(on))   # put back; active
            assert ptamd.get_bvh_wide()[2] == bool(wide)
            tr.trace_frames(1, 2)
            runs.append((tr.image().tobytes(), tr.stats()["segments_total"]))
        finally:
            tr.free()
    assert runs[0] == runs[1] and runs[0][1] > 0
