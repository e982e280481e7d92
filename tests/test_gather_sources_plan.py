"""CPU: the planner of the gather with a source per range (csrc/launch_plan.cpp: gather_sources_first_bad and
plan_gather_launch over ranges that carry their source address: bounds, wrap-around of src + len, empty
ranges, merging of address-adjacent ranges, tile prefix sums, 64-range splits, and a host model of the
kernel's loads) under AddressSanitizer and UndefinedBehaviorSanitizer, driven by
tests/native/gather_sources_plan_check.cpp, a program of its own that links the planner alone. And the
argument checks of hdfs3_gather_sources_dev_async, hdfs3_output_writev_dev and hdfs3_fs_writev_dev that return
before any device is touched, and their structs' ctypes bindings."""
import ctypes
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gather_sources_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "gather_sources_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "gather_sources_plan_check.cpp"),
           os.path.join(CSRC, "launch_plan.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gather sources plan ok" in out.stdout


def test_new_calls_reject_null_handles_without_a_device():
    from libhdfs3_amd import _native

    lib = _native.lib()
    r = (_native.SrcRange * 1)()
    r[0].d_src, r[0].len = 64, 1
    assert lib.hdfs3_gather_sources_dev_async(None, 16, 16, r, 1) == -22  # -EINVAL
    assert lib.hdfs3_gather_sources_dev_async(None, 16, 16, None, 0) == -22
    iov = (_native.DevIovec * 1)()
    iov[0].d_base, iov[0].len = 64, 1
    for call in (lambda: lib.hdfs3_output_writev_dev(None, iov, 1), lambda: lib.hdfs3_output_writev_dev(None, None, 0),
                 lambda: lib.hdfs3_fs_writev_dev(None, None, iov, 1)):
        ctypes.set_errno(0)
        assert call() == -1 and ctypes.get_errno() == 22


def _struct_body(header, name):
    src = open(os.path.join(REPO, "include", header)).read()
    return src.split("typedef struct %s {" % name)[1].split("}")[0]


def test_struct_bindings_match_the_headers():
    from libhdfs3_amd import _native

    assert ctypes.sizeof(_native.SrcRange) == 24 == ctypes.sizeof(_native.CopyRange)
    assert [f[0] for f in _native.SrcRange._fields_] == ["d_src", "dst_off", "len"]
    assert [_native.SrcRange.d_src.offset, _native.SrcRange.dst_off.offset, _native.SrcRange.len.offset] == [0, 8, 16]
    body = _struct_body("hdfs3_crc.h", "hdfs3_src_range")
    assert body.index("const void *d_src;") < body.index("uint64_t dst_off;") < body.index("uint64_t len;")

    assert ctypes.sizeof(_native.DevIovec) == 16
    assert [f[0] for f in _native.DevIovec._fields_] == ["d_base", "len"]
    assert [_native.DevIovec.d_base.offset, _native.DevIovec.len.offset] == [0, 8]
    body = _struct_body("hdfs3_client.h", "hdfs3_dev_iovec")
    assert body.index("const void *d_base;") < body.index("uint64_t len;")
