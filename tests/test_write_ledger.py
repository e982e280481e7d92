"""CPU: the output stream's batch ledger (csrc/client/batch_ledger.cpp: which bytes of a batch the host
wrote and which were placed from device memory, what to upload and whether to copy back) under
AddressSanitizer and UndefinedBehaviorSanitizer, driven by tests/native/write_ledger_check.cpp, a program
of its own that links the ledger alone. And the device-write calls' argument checks, which return before
any device is touched."""
import ctypes
import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "libhdfs3_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_write_ledger_under_asan_ubsan(tmp_path):
    exe = tmp_path / "write_ledger_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(REPO, "tests", "native", "write_ledger_check.cpp"),
           os.path.join(CSRC, "client", "batch_ledger.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "write ledger ok" in out.stdout


def test_device_write_calls_reject_null_arguments_without_a_device():
    from libhdfs3_amd import _native

    lib = _native.lib()
    ctypes.set_errno(0)
    assert lib.hdfs3_output_write_dev(None, 16, 16) == -1 and ctypes.get_errno() == 22  # EINVAL
    assert lib.hdfs3_output_device_stats(None, None, None) == -22
    ctypes.set_errno(0)
    assert lib.hdfs3_fs_write_dev(None, None, 16, 16) == -1 and ctypes.get_errno() == 22


def test_device_write_is_declared_and_bound():
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import OutputStream

    assert "hdfs3_output_write_dev" in _native.CLIENT_API and "hdfs3_output_device_stats" in _native.CLIENT_API
    assert "hdfs3_fs_write_dev" in _native.HDFS_API
    assert callable(OutputStream.write_device) and callable(OutputStream.device_stats)
    assert _native.lib().hdfs3_crc_abi_version() == 1  # the change only adds
