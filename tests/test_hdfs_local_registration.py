"""CPU: the hdfs.h layer's registration of short-circuit replicas, hdfs3_fs_add_local_replica and
hdfs3_fs_set_local_read (include/hdfs3_hdfs.h), over hdfs3_fs_new's path table. No file is opened, so no GPU
is touched; the reads themselves are in test_input_stream_local.py."""
import ctypes
import errno
import os
import re

import pytest

from util import REPO

POOL = b"BP-loopback"


@pytest.fixture
def fs():
    from libhdfs3_amd import _native

    lib = _native.lib()
    h = lib.hdfs3_fs_new(b"registration-test", None, None)
    assert h
    yield lib, h
    lib.hdfsDisconnect(h)


def _add_file(lib, h, path, blocks):
    from libhdfs3_amd.engine import _located_blocks

    arr, keep = _located_blocks(blocks, POOL, 1)
    assert lib.hdfs3_fs_add_file(h, path, arr, len(blocks)) == 0


def _fails(rc, want):
    return rc == -1 and ctypes.get_errno() == want


TWO_BLOCKS = [(1, 1000, [("127.0.0.1", 1), ("127.0.0.1", 2)]), (2, 500, [("127.0.0.1", 1)])]


def test_add_local_replica_errors_and_success(fs):
    lib, h = fs
    add = lib.hdfs3_fs_add_local_replica
    assert _fails(add(h, b"/nope", 0, 0, b"/d", b"/m"), errno.ENOENT)  # no located blocks registered
    _add_file(lib, h, b"/f", TWO_BLOCKS)
    assert _fails(add(h, b"/other", 0, 0, b"/d", b"/m"), errno.ENOENT)
    for block, replica in [(-1, 0), (2, 0), (0, -1), (0, 2), (1, 1)]:  # block 1 has one replica
        assert _fails(add(h, b"/f", block, replica, b"/d", b"/m"), errno.EINVAL), (block, replica)
    for data, meta in [(None, b"/m"), (b"/d", None), (b"", b"/m"), (b"/d", b"")]:
        assert _fails(add(h, b"/f", 0, 0, data, meta), errno.EINVAL), (data, meta)
    assert _fails(add(None, b"/f", 0, 0, b"/d", b"/m"), errno.EINVAL)
    assert _fails(add(h, None, 0, 0, b"/d", b"/m"), errno.EINVAL)
    assert add(h, b"/f", 0, 0, b"/d", b"/m") == 0
    assert add(h, b"/f", 0, 1, b"/d1", b"/m1") == 0
    assert add(h, b"/f", 1, 0, b"/d2", b"/m2") == 0
    assert _fails(add(h, b"/f", 0, 1, b"/x", b"/y"), errno.EINVAL)  # a duplicate, whatever the paths
    assert lib.hdfsGetLastError()


def test_re_adding_the_file_drops_its_local_replicas(fs):
    lib, h = fs
    add = lib.hdfs3_fs_add_local_replica
    _add_file(lib, h, b"/f", TWO_BLOCKS)
    assert add(h, b"/f", 0, 0, b"/d", b"/m") == 0
    assert _fails(add(h, b"/f", 0, 0, b"/d", b"/m"), errno.EINVAL)
    _add_file(lib, h, b"/f", TWO_BLOCKS[:1])  # replaces the entry
    assert add(h, b"/f", 0, 0, b"/d", b"/m") == 0  # the duplicate rule no longer fires
    assert _fails(add(h, b"/f", 1, 0, b"/d", b"/m"), errno.EINVAL)  # and the indices are the new table's


def test_set_local_read(fs):
    from libhdfs3_amd import _native

    lib, h = fs
    assert lib.hdfs3_fs_set_local_read(h, 0, None) == 0
    assert lib.hdfs3_fs_set_local_read(h, 1, None) == 0
    ok = _native.LocalOpts(0, 1, 64 << 10, 2, 1)
    assert lib.hdfs3_fs_set_local_read(h, 1, ctypes.byref(ok)) == 0
    for bad in [_native.LocalOpts(0, 1, 64 << 10, 2, 2), _native.LocalOpts(0, 1, (1 << 30) + 1, 2, 0)]:
        assert _fails(lib.hdfs3_fs_set_local_read(h, 1, ctypes.byref(bad)), errno.EINVAL)
    assert _fails(lib.hdfs3_fs_set_local_read(None, 1, None), errno.EINVAL)


def test_the_new_declarations_are_exported_and_bound():
    from libhdfs3_amd import _native

    lib = _native.load()
    hdfs_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hdfs3_hdfs.h")).read(), flags=re.S)
    client_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hdfs3_client.h")).read(), flags=re.S)
    for name, header, table in [("hdfs3_fs_add_local_replica", hdfs_h, _native.HDFS_API),
                                ("hdfs3_fs_set_local_read", hdfs_h, _native.HDFS_API),
                                ("hdfs3_input_set_local_replicas", client_h, _native.CLIENT_API),
                                ("hdfs3_input_local_stats", client_h, _native.CLIENT_API)]:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in table, name
