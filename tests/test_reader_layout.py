"""CPU: the block reader's batch geometry (csrc/client/reader_layout.h: where a packet's words and data land
in a batch arena, when a batch closes or the arena grows, which packet a verify result names, the delivery
cursor, the arena's size) under AddressSanitizer and UndefinedBehaviorSanitizer, driven by
tests/native/reader_layout_check.cpp, a program of its own that includes that header alone."""
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reader_layout_under_asan_ubsan(tmp_path):
    exe = tmp_path / "reader_layout_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "reader_layout_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "reader layout ok" in out.stdout


def test_reader_layout_header_needs_no_gpu_runtime():
    with open(os.path.join(CSRC, "client", "reader_layout.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i.lower()], includes
