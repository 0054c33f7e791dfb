"""The naive mesh mode's public surface without a GPU: include/pt/pt_naive_mesh.h against the
library's exports and the ctypes prototypes, an unchanged pathtrace_abi.h, and the state rules of
pt_set_naive_mesh / pt_get_naive_mesh (process-global, sticky, initial value from PT_NAIVE_MESH)."""
import ctypes
import os
import re
import subprocess
import sys

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "pt", "pt_naive_mesh.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", src)))


def test_abi_unchanged_and_symbols_exported(ptamd):
    names = _declared()
    assert {"pt_set_naive_mesh", "pt_get_naive_mesh"} <= set(names)
    assert sorted(ptamd.NAIVE_MESH_SYMBOLS) == names
    for n in names:
        fn = getattr(ptamd.lib, n)                      # AttributeError: not exported
        assert fn.argtypes is not None, n               # prototyped in ptamd._load
    assert not set(names) & set(ptamd.ABI_SYMBOLS)      # a header of its own, not pathtrace_abi.h
    abi = open(os.path.join(REPO, "include", "pt", "pathtrace_abi.h")).read()
    assert "naive" not in abi.lower()
    assert "#define PT_ABI_VERSION 3" in abi and ptamd.lib.pt_abi_version() == 3
    # pt_options: 15 int32 + device_ids[16] + combine, as before
    assert ctypes.sizeof(ptamd._Options) == 4 * (15 + 16 + 1) == 128
    o = ptamd._Options()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    guard = (ctypes.c_uint8 * 160)(*([0xa5] * 160))
    ctypes.memmove(guard, ctypes.byref(o), 128)
    ptamd.lib.pt_default_options(ctypes.cast(guard, ctypes.c_void_p))
    assert bytes(guard[128:]) == b"\xa5" * 32           # the library writes sizeof(pt_options) = 128 bytes
    assert ptamd.naive_mesh_tile() >= 1


def test_setter_and_getter_state_rules(ptamd):
    L = ptamd.lib
    L.pt_free()
    prev = ptamd.get_naive_mesh()[0]
    try:
        nxt, act = ctypes.c_int32(-7), ctypes.c_int32(-7)
        assert L.pt_set_naive_mesh(1) == 0
        assert L.pt_get_naive_mesh(ctypes.byref(nxt), ctypes.byref(act)) == 0
        assert (nxt.value, act.value) == (1, 0)         # no context: active is 0
        assert L.pt_get_naive_mesh(None, None) == 0     # either pointer may be NULL
        assert L.pt_get_naive_mesh(ctypes.byref(nxt), None) == 0 and nxt.value == 1   # sticky
        # with the mode on, the default pipeline is the staged one; off, the fused one again
        assert ptamd.default_options().pipeline == ptamd.PIPELINE_STAGED
        assert L.pt_set_naive_mesh(5) == 0              # any non-zero value: on
        assert ptamd.get_naive_mesh() == (True, False)
        assert L.pt_set_naive_mesh(0) == 0
        assert ptamd.get_naive_mesh() == (False, False)
        assert ptamd.default_options().pipeline == ptamd.PIPELINE_FUSED
        L.pt_free()                                     # freeing does not touch the setting
        ptamd.set_naive_mesh(True)
        L.pt_free()
        assert ptamd.get_naive_mesh() == (True, False)
    finally:
        ptamd.set_naive_mesh(prev)


def test_initial_value_comes_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); import ptamd; "
            "print(int(ptamd.get_naive_mesh()[0]), ptamd.default_options().pipeline)" % PKG)
    for value, want in ((None, "0 0"), ("1", "1 1"), ("0", "0 0"), ("", "0 0")):
        env = {k: v for k, v in os.environ.items() if k != "PT_NAIVE_MESH"}
        if value is not None:
            env["PT_NAIVE_MESH"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split("\n")[0].strip() == want, (value, r.stdout)
