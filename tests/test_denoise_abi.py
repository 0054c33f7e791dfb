"""The denoiser's public surface without a GPU: include/pt/pt_denoise.h against the library's
exports and the ctypes prototypes, the documented defaults, call-order errors before pt_init, and
pt_render's --denoise argument check."""
import ctypes
import os
import re
import subprocess

from conftest import REPO, scene_path

HEADER = os.path.join(REPO, "include", "pt", "pt_denoise.h")
PT_RENDER = os.path.join(REPO, "project3-cuda-path-tracer-2025_amd", "build", "pt_render")
PT_E_STATE = -2


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_function_is_exported_and_prototyped(ptamd):
    names = _declared()
    assert {"pt_denoise_default_params", "pt_gbuffer_capture", "pt_gbuffer_get", "pt_denoise"} <= set(names)
    assert sorted(ptamd.DENOISE_SYMBOLS) == names
    for n in names:
        fn = getattr(ptamd.lib, n)                      # AttributeError: not exported
        assert fn.argtypes is not None, n               # prototyped in ptamd._load
    assert not set(names) & set(ptamd.ABI_SYMBOLS)      # a header of its own, not pathtrace_abi.h
    abi = open(os.path.join(REPO, "include", "pt", "pathtrace_abi.h")).read()
    assert "denoise" not in abi and "gbuffer" not in abi
    assert ptamd.lib.pt_abi_version() == 3


def test_default_params(ptamd):
    p = ptamd.denoise_default_params()
    assert ctypes.sizeof(p) == 20
    assert (p.levels, p.demodulate_albedo) == (5, 1)
    f32 = lambda v: ctypes.c_float(v).value
    assert (p.sigma_color, p.sigma_normal, p.sigma_position) == (f32(0.45), f32(0.35), f32(0.20))
    q = ptamd.denoise_default_params(levels=3, sigma_color=0.2)
    assert (q.levels, q.sigma_color, q.sigma_normal) == (3, f32(0.2), f32(0.35))


def test_calls_before_init_are_state_errors(ptamd):
    L = ptamd.lib
    L.pt_free()
    assert L.pt_gbuffer_capture(1) == PT_E_STATE
    assert b"pt_init" in L.pt_last_error()
    assert L.pt_gbuffer_get(None, None, None, 0) == PT_E_STATE
    assert L.pt_denoise(None, 1, None, None) == PT_E_STATE
    assert L.pt_debug_denoise_times(None, None, None) == PT_E_STATE
    assert L.pt_abi_version() == 3


def test_pt_render_rejects_a_malformed_level_count():
    for bad in ("many", "0", "9", "3x", "-2"):
        r = subprocess.run([PT_RENDER, scene_path("cornell"), "--denoise", bad], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert "usage: --denoise [LEVELS]" in r.stderr and bad in r.stderr
