"""GPU: hdfs3_input_read_dev / hdfs3_input_pread_dev and their hdfs.h-layer forms hdfs3_fs_read_dev /
hdfs3_fs_pread_dev: the input stream's block walk, failover and error convention with the destination in
device memory. The destination is pre-filled with a canary and downloaded whole: whatever is not
verified file data must still be the canary."""
import ctypes
import errno
import os

import numpy as np
import pytest

from util import oracle_compute, splitmix_bytes

pytestmark = pytest.mark.gpu

BPC = 512
CANARY = 0xC3
SIZES = [1 << 20, 1 << 20, 1 << 20]
STARTS = [0, 1 << 20, 2 << 20, 3 << 20]
POOL = b"BP-loopback"


@pytest.fixture(scope="module")
def cluster():
    """Two healthy replicas of a 3-block file, one replica with block 1 corrupt, and the file's bytes."""
    from loopback import LoopbackDatanode

    a, b, bad = LoopbackDatanode(), LoopbackDatanode(), LoopbackDatanode()
    blocks, parts = [], []
    for i, n in enumerate(SIZES):
        d = splitmix_bytes(n, 300 + i)
        c = oracle_compute(d, BPC)
        for node in (a, b):
            node.add_block(700 + i, d, c, BPC)
        if i == 1:
            x = d.copy()
            x[600_000] ^= 0x20  # packet 9 of block 1
            bad.add_block(700 + i, x, c, BPC)
        else:
            bad.add_block(700 + i, d, c, BPC)
        blocks.append((700 + i, n))
        parts.append(d)
    yield a, b, bad, blocks, np.concatenate(parts)
    for node in (a, b, bad):
        node.stop()


class Dest:
    def __init__(self, ctx, nbytes, off=0):
        from libhdfs3_amd.engine import DeviceBuffer

        self.ctx, self.off = ctx, off
        self.buf = DeviceBuffer(off + nbytes + 64)
        ctx.memset(self.buf, CANARY, self.buf.nbytes)
        self.ptr = self.buf.ptr + off

    def download(self):
        return self.ctx.download(self.buf, self.buf.nbytes)

    def check(self, want):
        exp = np.full(self.buf.nbytes, CANARY, np.uint8)
        exp[self.off:self.off + want.nbytes] = want
        assert np.array_equal(self.download(), exp)

    def free(self):
        self.buf.free()


def _stream(blocks, nodes, **kw):
    from libhdfs3_amd.engine import InputStream

    return InputStream([(bid, n, [("127.0.0.1", x.port) for x in nodes]) for bid, n in blocks], **kw)


def _read_to_eof(s, dest, total, chunk):
    pos = 0
    while True:
        n = s.read_into_device(dest.ptr + pos, min(chunk, total + 16 - pos))
        if n == 0:
            return pos
        blk = max(i for i in range(3) if STARTS[i] <= pos)
        assert pos + n <= STARTS[blk + 1]  # readOneBlock never returns bytes of two blocks
        pos += n
        assert s.tell() == pos


def test_read_dev_to_the_end_of_the_file(gpu_ctx, cluster):
    a, b, bad, blocks, whole = cluster
    dest = Dest(gpu_ctx, whole.nbytes, off=1)
    try:
        with _stream(blocks, [a]) as s:
            assert _read_to_eof(s, dest, whole.nbytes, 700_001) == whole.nbytes
            assert s.stats()["readers_opened"] == 3 and s.stats()["failovers"] == 0
        dest.check(whole)
    finally:
        dest.free()


def test_pread_dev_across_a_block_boundary(gpu_ctx, cluster):
    from libhdfs3_amd.engine import HdfsIOError

    a, b, bad, blocks, whole = cluster
    pos, n = (1 << 20) - 70_001, 1_200_003  # ends inside block 2
    dest = Dest(gpu_ctx, n, off=5)
    try:
        with _stream(blocks, [a]) as s:
            s.seek(4321)
            assert s.pread_into_device(pos, dest.ptr, n) == n
            assert s.tell() == 4321
            with pytest.raises(HdfsIOError) as ei:
                s.pread_into_device(whole.nbytes, dest.ptr, 4)
            assert ei.value.errno == errno.EINVAL
            host = np.zeros(16, np.uint8)  # not device memory: the caller's mistake, no replica is burnt
            with pytest.raises(HdfsIOError) as ei:
                s.pread_into_device(0, host.ctypes.data, 16)
            assert ei.value.errno == errno.EINVAL and s.stats()["failovers"] == 0
        dest.check(whole[pos:pos + n])
    finally:
        dest.free()


def test_a_corrupt_first_replica_fails_over(gpu_ctx, cluster):
    a, b, bad, blocks, whole = cluster
    dest = Dest(gpu_ctx, whole.nbytes)
    try:
        with _stream(blocks, [bad, b]) as s:
            assert _read_to_eof(s, dest, whole.nbytes, 1 << 20) == whole.nbytes
            assert s.stats()["failovers"] == 1
        dest.check(whole)
    finally:
        dest.free()
    # pread_dev over the corrupt packet: the second replica's bytes from the range's first byte on
    pos, n = (1 << 20) + 500_000, 300_000
    dest = Dest(gpu_ctx, n, off=9)
    try:
        with _stream(blocks, [bad, b]) as s:
            assert s.pread_into_device(pos, dest.ptr, n) == n
            assert s.stats()["failovers"] == 1
        dest.check(whole[pos:pos + n])
    finally:
        dest.free()


def test_every_replica_corrupt_leaves_verified_data_or_canary(gpu_ctx, cluster):
    from libhdfs3_amd.engine import HdfsIOError

    a, b, bad, blocks, whole = cluster
    for pread in (False, True):
        dest = Dest(gpu_ctx, whole.nbytes)
        try:
            with _stream(blocks, [bad, bad]) as s:
                with pytest.raises(HdfsIOError) as ei:
                    if pread:
                        s.pread_into_device(0, dest.ptr, whole.nbytes)
                    else:
                        _read_to_eof(s, dest, whole.nbytes, 1 << 20)
                assert ei.value.errno == errno.EIO
            got = dest.download()
            file_part = got[:whole.nbytes]
            ok = (file_part == whole) | (file_part == CANARY)
            assert ok.all(), int(np.flatnonzero(~ok)[0])
            assert np.all(got[whole.nbytes:] == CANARY)
            # the packets before the bad one were delivered, nothing from it on (9 packets into block 1)
            good_end = (1 << 20) + 9 * 65536
            assert np.array_equal(file_part[:good_end], whole[:good_end])
            assert np.all(file_part[good_end:] == CANARY)
        finally:
            dest.free()


def test_read_dev_with_block_read_ahead(gpu_ctx, cluster):
    a, b, bad, blocks, whole = cluster
    dest = Dest(gpu_ctx, whole.nbytes, off=3)
    try:
        with _stream(blocks, [a]) as s:
            s.set_readahead(2)
            assert _read_to_eof(s, dest, whole.nbytes, 400_000) == whole.nbytes
        dest.check(whole)
    finally:
        dest.free()


def test_hdfs_h_layer_device_reads_match_hdfsRead_and_hdfsPread(gpu_ctx, cluster):
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import _located_blocks

    a, b, bad, blocks, whole = cluster
    lib = _native.lib()
    fs = lib.hdfs3_fs_new(b"device-test", None, None)
    assert fs
    dest = Dest(gpu_ctx, whole.nbytes + 300_000, off=11)
    try:
        arr, keep = _located_blocks([(bid, n, [("127.0.0.1", a.port)]) for bid, n in blocks], POOL, 1)
        assert lib.hdfs3_fs_add_file(fs, b"/f", arr, len(blocks)) == 0
        f = lib.hdfsOpenFile(fs, b"/f", os.O_RDONLY, 0, 0, 0)
        g = lib.hdfsOpenFile(fs, b"/f", os.O_RDONLY, 0, 0, 0)
        assert f and g, lib.hdfsGetLastError()
        host = np.zeros(whole.nbytes, np.uint8)
        pos = 0
        while True:  # the two files in step: same counts, same bytes
            n_dev = lib.hdfs3_fs_read_dev(fs, f, dest.ptr + pos, 900_000)
            n_host = lib.hdfsRead(fs, g, host.ctypes.data + pos, 900_000) if pos < whole.nbytes else 0
            assert n_dev == n_host, (pos, n_dev, n_host, lib.hdfsGetLastError())
            if n_dev == 0:
                break
            pos += n_dev
            assert lib.hdfsTell(fs, f) == pos
        assert pos == whole.nbytes and np.array_equal(host, whole)
        ppos, pn = (2 << 20) - 12_345, 300_000
        phost = np.zeros(pn, np.uint8)
        assert lib.hdfsPread(fs, g, phost.ctypes.data, pn, ppos) == pn
        assert lib.hdfs3_fs_pread_dev(fs, f, dest.ptr + whole.nbytes, pn, ppos) == pn
        dest.check(np.concatenate([host, phost]))
        # hdfs.h's error convention: -1 and errno
        ctypes.set_errno(0)
        assert lib.hdfs3_fs_pread_dev(fs, f, dest.ptr, 16, whole.nbytes) == -1 and ctypes.get_errno() == errno.EINVAL
        assert lib.hdfs3_fs_read_dev(fs, f, None, 16) == -1 and ctypes.get_errno() == errno.EINVAL
        assert lib.hdfsCloseFile(fs, f) == 0 and lib.hdfsCloseFile(fs, g) == 0
    finally:
        lib.hdfsDisconnect(fs)
        dest.free()
