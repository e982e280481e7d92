"""GPU: hdfs3_block_reader_read_dev, the block reader's delivery into device memory, against the
loopback datanode. Same contract as hdfs3_block_reader_read (test_block_reader.py); in addition the
bytes are in place when the call returns and nothing past the returned count is written: the
destination is pre-filled with a canary and downloaded whole."""
import errno

import numpy as np
import pytest

from util import oracle_compute, splitmix_bytes

pytestmark = pytest.mark.gpu

CANARY = 0x5C
BLOCK = 2 << 20


@pytest.fixture(scope="module")
def dn():
    from loopback import LoopbackDatanode

    node = LoopbackDatanode()
    yield node
    node.stop()


@pytest.fixture(scope="module")
def blocks(dn):
    """The blocks the tests read, served once: id -> (data as served, true data)."""
    out = {}
    for bpc in (512, 4096):
        data = splitmix_bytes(BLOCK, 70 + bpc)
        dn.add_block(bpc, data, oracle_compute(data, bpc), bpc)
        out[bpc] = data
    tail = splitmix_bytes(3_000_000 + 123, 42)  # last chunk short
    dn.add_block(2000, tail, oracle_compute(tail, 512), 512)
    out[2000] = tail
    good = out[512]
    bad = good.copy()
    bad[20 * 65536 + 4321] ^= 0x08  # packet 20 (64 KiB packets)
    dn.add_block(3000, bad, oracle_compute(good, 512), 512)
    out[3000] = bad
    dn.add_block(7000, good, None, 512, ctype=0)  # CHECKSUM_NULL
    return out


class Dest:
    """A canary-filled device buffer; the destination starts `off` bytes into it."""

    def __init__(self, ctx, nbytes, off=0):
        from libhdfs3_amd.engine import DeviceBuffer

        self.ctx, self.off = ctx, off
        self.buf = DeviceBuffer(off + nbytes + 64)
        ctx.memset(self.buf, CANARY, self.buf.nbytes)
        self.ptr = self.buf.ptr + off

    def check(self, want):
        """`want` at the destination, canary everywhere else"""
        got = self.ctx.download(self.buf, self.buf.nbytes)
        exp = np.full(self.buf.nbytes, CANARY, np.uint8)
        exp[self.off:self.off + want.nbytes] = want
        assert np.array_equal(got, exp)

    def free(self):
        self.buf.free()


def _read_dev(r, dest, length, chunk=1 << 20):
    pos = 0
    while pos < length:
        got = r.read_into_device(dest.ptr + pos, min(chunk, length - pos))
        if got == 0:
            break
        pos += got
    return pos


@pytest.mark.parametrize("bpc,batch", [(512, 64), (512, 1), (4096, 5)])
def test_full_block_into_device_memory(gpu_ctx, dn, blocks, bpc, batch):
    from libhdfs3_amd.engine import BlockReader

    data = blocks[bpc]
    dest = Dest(gpu_ctx, data.nbytes)
    try:
        with BlockReader("127.0.0.1", dn.port, bpc, 0, data.nbytes, batch_packets=batch) as r:
            assert _read_dev(r, dest, data.nbytes) == data.nbytes
            assert r.read_into_device(dest.ptr, 16) == 0  # end of range
            st = r.device_stats()
        dest.check(data)
        assert st["bytes_gathered"] == data.nbytes and st["gather_launches"] >= 1
    finally:
        dest.free()


@pytest.mark.parametrize("start,length", [(1, 1000), (511, 2), (65535, 70000), (-1000, 1000)])
def test_ranged_reads_into_an_odd_destination_offset(gpu_ctx, dn, blocks, start, length):
    from libhdfs3_amd.engine import BlockReader

    data = blocks[2000]
    start = start if start >= 0 else data.nbytes + start
    dest = Dest(gpu_ctx, length, off=7)
    try:
        with BlockReader("127.0.0.1", dn.port, 2000, start, length, batch_packets=7) as r:
            assert _read_dev(r, dest, length, chunk=33333) == length
        dest.check(data[start:start + length])
    finally:
        dest.free()


def test_corruption_delivers_the_packets_before_it_and_nothing_after(gpu_ctx, dn, blocks):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import BlockReader

    served, good = blocks[3000], blocks[512]
    dest = Dest(gpu_ctx, served.nbytes)
    try:
        with BlockReader("127.0.0.1", dn.port, 3000, 0, served.nbytes, batch_packets=16) as r:
            pos = 0
            with pytest.raises(Hdfs3CrcError) as ei:
                while True:
                    got = r.read_into_device(dest.ptr + pos, 1 << 19)
                    assert got > 0
                    pos += got
            assert ei.value.rc == -errno.EIO and "ChecksumException" in str(ei.value)
        # every packet before the bad one and nothing else: canary from the returned count onward
        assert pos == 20 * 65536
        dest.check(good[:pos])
    finally:
        dest.free()


@pytest.mark.parametrize("block_id,kw", [(3000, {"verify": False}), (7000, {})])
def test_unverified_blocks_deliver_the_served_bytes(gpu_ctx, dn, blocks, block_id, kw):
    """verify off, and a CHECKSUM_NULL block: nothing was uploaded for a verify, so the device read uploads
    the batch itself; the bytes are the ones served (the corrupt ones, with verify off)."""
    from libhdfs3_amd.engine import BlockReader

    served = blocks[3000] if block_id == 3000 else blocks[512]
    dest = Dest(gpu_ctx, served.nbytes, off=3)
    try:
        with BlockReader("127.0.0.1", dn.port, block_id, 0, served.nbytes, batch_packets=4, **kw) as r:
            assert _read_dev(r, dest, served.nbytes, chunk=300_001) == served.nbytes
        dest.check(served)
    finally:
        dest.free()


def test_host_and_device_reads_alternate_on_one_reader(gpu_ctx, dn, blocks):
    from libhdfs3_amd.engine import BlockReader

    data = blocks[4096]
    dest = Dest(gpu_ctx, data.nbytes)
    host = np.zeros(data.nbytes, np.uint8)
    dev_parts = []
    try:
        with BlockReader("127.0.0.1", dn.port, 4096, 0, data.nbytes, batch_packets=3) as r:
            pos, turn = 0, 0
            while pos < data.nbytes:
                n = min(100_003, data.nbytes - pos)
                if turn % 2:
                    got = r.read_into_device(dest.ptr + pos, n)
                    dev_parts.append((pos, got))
                else:
                    got = r.read_into(host, pos, n)
                assert got > 0
                pos += got
                turn += 1
            st = r.device_stats()
        got = gpu_ctx.download(dest.buf, dest.buf.nbytes)
        exp = np.full(dest.buf.nbytes, CANARY, np.uint8)
        for p, n in dev_parts:
            exp[p:p + n] = data[p:p + n]
            host[p:p + n] = data[p:p + n]  # the device's share, checked just above
        assert np.array_equal(got, exp)
        assert np.array_equal(host, data)
        assert st["bytes_gathered"] == sum(n for _, n in dev_parts)
    finally:
        dest.free()


def test_a_host_pointer_is_refused_and_the_reader_stays_usable(gpu_ctx, dn, blocks):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import BlockReader

    data = blocks[512]
    host = np.full(4096, CANARY, np.uint8)
    dest = Dest(gpu_ctx, data.nbytes)
    try:
        with BlockReader("127.0.0.1", dn.port, 512, 0, data.nbytes) as r:
            with pytest.raises(Hdfs3CrcError) as ei:
                r.read_into_device(host.ctypes.data, 4096)
            assert ei.value.rc == -errno.EINVAL and np.all(host == CANARY)
            assert _read_dev(r, dest, data.nbytes) == data.nbytes
        dest.check(data)
    finally:
        dest.free()
