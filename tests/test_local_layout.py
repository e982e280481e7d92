"""CPU: the short-circuit reader's geometry (csrc/client/local_layout.h: the chunk-rounded buffer, the first
byte read, the windows and their chunks and .meta words, where a corrupt block's good bytes end, counted by the
host and by the guarded delivery kernel, and the span of a window a read takes) under AddressSanitizer and
UndefinedBehaviorSanitizer, driven by tests/native/local_layout_check.cpp, a program of its own that includes
that header alone."""
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_local_layout_under_asan_ubsan(tmp_path):
    exe = tmp_path / "local_layout_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "local_layout_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "local layout ok" in out.stdout


def test_local_layout_header_needs_no_gpu_runtime():
    for name in ("local_layout.h", "local_range.h"):
        with open(os.path.join(CSRC, "client", name)) as f:
            includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
        assert includes and not [i for i in includes if "hip" in i.lower()], (name, includes)
    with open(os.path.join(CSRC, "launch_plan.h")) as f:  # the one header it takes from outside client/
        assert not [ln for ln in f if ln.startswith("#include") and "hip" in ln.lower()]
