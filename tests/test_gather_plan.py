"""CPU: the gather planner (csrc/launch_plan.cpp: bounds, empty ranges, merging, tile prefix sums, the
split of long lists over launches) under AddressSanitizer and UndefinedBehaviorSanitizer, driven by
tests/native/gather_plan_check.cpp, a program of its own that links the planner alone. And the new C
calls' argument checks, which return before any device is touched."""
import ctypes
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gather_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "gather_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "gather_plan_check.cpp"),
           os.path.join(CSRC, "launch_plan.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gather plan ok" in out.stdout


def test_new_calls_reject_a_null_context_without_a_device():
    from libhdfs3_amd import _native

    lib = _native.lib()
    r = (_native.CopyRange * 1)()
    r[0].len = 1
    assert lib.hdfs3_gather_dev_async(None, 16, 16, 32, 16, r, 1) == -22  # -EINVAL
    pk = (_native.PktDesc * 1)()
    placed = ctypes.c_uint64(7)
    assert lib.hdfs3_crc32c_verify_packets_gather_dev(None, 16, 16, pk, 1, 512, 0, 32, 16, 0, None, None,
                                                      ctypes.byref(placed)) == -22
    assert lib.hdfs3_block_reader_read_dev(None, 16, 16) == -22
    assert lib.hdfs3_block_reader_device_stats(None, None, None) == -22
    ctypes.set_errno(0)
    assert lib.hdfs3_input_read_dev(None, 16, 16) == -1 and ctypes.get_errno() == 22
    assert lib.hdfs3_input_pread_dev(None, 0, 16, 16) == -1 and ctypes.get_errno() == 22
    assert lib.hdfs3_fs_read_dev(None, None, 16, 16) == -1 and ctypes.get_errno() == 22
    assert lib.hdfs3_fs_pread_dev(None, None, 16, 16, 0) == -1 and ctypes.get_errno() == 22


def test_copy_range_binding_matches_the_header():
    from libhdfs3_amd import _native

    assert ctypes.sizeof(_native.CopyRange) == 24
    assert [f[0] for f in _native.CopyRange._fields_] == ["src_off", "dst_off", "len"]
    src = open(os.path.join(REPO, "include", "hdfs3_crc.h")).read()
    body = src.split("typedef struct hdfs3_copy_range {")[1].split("}")[0]
    assert [w for w in ("src_off", "dst_off", "len") if w in body] == ["src_off", "dst_off", "len"]
    assert body.index("src_off") < body.index("dst_off") < body.index("len;")
