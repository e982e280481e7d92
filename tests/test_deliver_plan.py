"""CPU: the guarded delivery's arithmetic (csrc/launch_plan.h: deliver_limit, deliver_clip, deliver_gate,
one set of constexpr functions compiled into the kernel and used by the host) and the planner as the
delivery uses it, under AddressSanitizer and UndefinedBehaviorSanitizer, driven by
tests/native/deliver_plan_check.cpp, a program of its own. And the new C calls' argument checks, which
return before any device is touched, and the guard's ctypes layout against the header."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_deliver_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "deliver_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "deliver_plan_check.cpp"),
           os.path.join(CSRC, "launch_plan.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "deliver plan ok" in out.stdout


def test_new_calls_reject_null_arguments_without_a_device():
    from libhdfs3_amd import _native

    lib = _native.lib()
    r = (_native.CopyRange * 1)()
    r[0].len = 1
    guard = _native.DeliverGuard(64, None, None, 0, 0, 2048, 512)
    # a null ctx, then (with any non-null ctx value never dereferenced before the check) a null guard
    assert lib.hdfs3_deliver_verified_dev_async(None, 16, 16, 32, 16, r, 1, ctypes.byref(guard)) == -22  # -EINVAL
    assert lib.hdfs3_deliver_verified_dev_async(None, 16, 16, 32, 16, r, 1, None) == -22
    assert lib.hdfs3_deliver_verified_dev_async(None, None, 0, None, 0, None, 0, None) == -22
    assert lib.hdfs3_local_reader_read_dev(None, 16, 16) == -22
    assert lib.hdfs3_local_reader_device_stats(None, None, None) == -22
    launches, placed = ctypes.c_uint64(5), ctypes.c_uint64(6)
    assert lib.hdfs3_local_reader_device_stats(None, ctypes.byref(launches), ctypes.byref(placed)) == -22
    assert (launches.value, placed.value) == (5, 6)


def test_deliver_guard_binding_matches_the_header():
    from libhdfs3_amd import _native

    names = ["d_result", "d_gate_in", "d_gate_out", "data_off", "chunk_base", "granule", "bpc"]
    assert [f[0] for f in _native.DeliverGuard._fields_] == names
    assert ctypes.sizeof(_native.DeliverGuard) == 56  # 3 pointers, 3 u64, a u32 and its padding
    assert _native.DeliverGuard.bpc.offset == 48 and _native.DeliverGuard.bpc.size == 4
    src = open(os.path.join(REPO, "include", "hdfs3_crc.h")).read()
    body = src.split("typedef struct hdfs3_deliver_guard {")[1].split("}")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w\s\*]+?)\b(\w+);", body)]
    assert [f[1] for f in fields] == names
    kinds = {"d_result": "const uint64_t *", "d_gate_in": "const uint64_t *", "d_gate_out": "uint64_t *",
             "data_off": "uint64_t", "chunk_base": "uint64_t", "granule": "uint64_t", "bpc": "uint32_t"}
    assert {n: re.sub(r"\s+", " ", t) for t, n in fields} == kinds
