"""CPU: the composite CRC arithmetic (csrc/crc_compose.cpp: the product in GF(2)[x]/P, x^(8n), the
composition of two CRCs, the composites of stored words and of blocks) under AddressSanitizer and
UndefinedBehaviorSanitizer, driven by tests/native/crc_compose_check.cpp. The arithmetic is plain host
C++, so the program links it alone: no GPU runtime and no Python-loaded native code."""
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_crc_compose_under_asan_ubsan(tmp_path):
    exe = tmp_path / "crc_compose_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "crc_compose_check.cpp"),
           os.path.join(CSRC, "crc_compose.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    # the sanitizer runtime is linked into the program; verify_asan_link_order=0: the environment may
    # preload other libraries ahead of it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "crc compose ok" in out.stdout


def test_compose_sources_need_no_gpu_runtime():
    for name in ("crc_compose.h", "crc_compose.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert "#include <hip" not in text and "#include \"hip" not in text, name
