"""The runtime's pure host parts, stand-alone under the sanitizers (host/runtime_host_check.cpp).

`make asan` builds build/asan/runtime_host_check (AddressSanitizer + UndefinedBehaviorSanitizer, plain
g++, no device code) and, where g++ links -fsanitize=thread, build/tsan/runtime_host_check.  The
program checks, and this test only runs it and reads its verdict:

  bands   host/band_layout.h: for every H in 1..17, rows in 1..5, count in 1..4, W in {1, 3}, the
          shards' bands (tail included) cover every byte of the image exactly once, none past H rows
  worker  host/worker.h: 1000 post / wait rounds in order, an error returned once, restart after
          join, the destructor of a never-started worker
  tuning  host/tuning.h: no PT_* variable set -> the default-constructed Tuning, and clamped inputs

The test preloads nothing and passes the environment through as it is: the sanitizer runtimes are
linked into the program itself.
"""
import os
import shutil
import subprocess

import pytest

from conftest import PKG

ASAN_EXE = os.path.join(PKG, "build", "asan", "runtime_host_check")
TSAN_EXE = os.path.join(PKG, "build", "tsan", "runtime_host_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0:allocator_may_return_null=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ for the sanitizer build")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", PKG, "asan"], check=True, capture_output=True, timeout=600)


def _run(exe, part):
    p = subprocess.run([exe, part], capture_output=True, text=True, timeout=120, env=ENV)
    out = p.stdout + p.stderr
    for word in ("AddressSanitizer", "LeakSanitizer", "ThreadSanitizer", "runtime error", "FAILED"):
        assert word not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
    return p.stdout


def test_band_layout_covers_the_image_once(built):
    out = _run(ASAN_EXE, "bands")
    assert "bands ok cases=%d" % (2 * 17 * 5 * 4) in out, out


def test_worker_thread(built):
    assert "worker ok" in _run(ASAN_EXE, "worker")


def test_tuning_defaults_and_clamps(built):
    assert "tuning ok" in _run(ASAN_EXE, "tuning")


def test_worker_thread_under_tsan(built):
    if not os.path.exists(TSAN_EXE):
        pytest.skip("this g++ does not link -fsanitize=thread")
    assert "worker ok" in _run(TSAN_EXE, "worker")
