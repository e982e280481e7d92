"""GPU: hdfs3_output_writev_dev (the output stream's vectored write from device memory) and its hdfs.h form
hdfs3_fs_writev_dev. The expected value is test_output_stream_device.py's: every packet handed to the sink must
be byte-identical to what the reference's OutputStreamImpl + Packet produce (tests/writer_model.py, CRC words
from the oracle) when each entry of a vectored call is one hdfsWrite of the same bytes. Ops: ("w", n)
hdfs3_output_write of the next n bytes, ("d", n) hdfs3_output_write_dev, ("v", [n0, n1, ...]) one
hdfs3_output_writev_dev whose entries take the next n0, n1, ... bytes, ("f", 0) flush, ("s", 0) sync.

A vectored call's entries are laid at random misalignments into three device allocations in turn (empty
entries get a null or a stray pointer), and all three are overwritten with a canary (on another stream,
synchronised) as soon as the call has returned: a call that returned before a source was read would put
canary bytes into the packets."""
import ctypes
import errno
import os
import random

import numpy as np
import pytest

from util import oracle_crc, splitmix_bytes
from writer_model import OutputStreamModel

pytestmark = pytest.mark.gpu

CANARY = 0xC3
BS = 512 * 12
SMALL = dict(packet_size=2048, block_size=BS, batch_packets=2)  # 4 chunks per packet, 3 packets per block
CAP = 160 * 1024  # bytes of each of the three allocations


def crc(b: bytes) -> int:
    return oracle_crc(np.frombuffer(b, np.uint8)) if b else 0


class Scratch:
    """Three device allocations the entries of one call are laid into."""

    def __init__(self, ctx, seed=0):
        from libhdfs3_amd.engine import DeviceBuffer

        self.ctx, self.rng = ctx, random.Random(seed)
        self.bufs = [DeviceBuffer(CAP) for _ in range(3)]
        self.clobber()

    def clobber(self):
        for b in self.bufs:
            self.ctx.memset(b, CANARY, CAP)  # synchronises its own stream

    def place(self, pieces, gap=None):
        """Uploads the pieces (uint8 arrays), piece i into allocation i % 3 behind a random gap of 1..40 bytes
        (or `gap` bytes: 0 lays the pieces of one allocation back to back); returns [(ptr, n)]."""
        images = [np.full(CAP, CANARY, np.uint8) for _ in range(3)]
        fill = [self.rng.randrange(16), self.rng.randrange(16), self.rng.randrange(16)]
        entries = []
        for i, p in enumerate(pieces):
            a = i % 3
            if p.nbytes == 0:
                entries.append((self.rng.choice([None, self.bufs[a].ptr + fill[a], 12345]), 0))
                continue
            fill[a] += self.rng.randrange(1, 41) if gap is None else gap
            assert fill[a] + p.nbytes <= CAP
            images[a][fill[a]:fill[a] + p.nbytes] = p
            entries.append((self.bufs[a].ptr + fill[a], p.nbytes))
            fill[a] += p.nbytes
        for b, img in zip(self.bufs, images):
            self.ctx.upload(img, b)
        return entries

    def free(self):
        for b in self.bufs:
            b.free()


def total_of(ops):
    return sum(sum(n) if op == "v" else n for op, n in ops if op in "wdv")


def run_both(ctx, ops, data, append=None, stats_out=None, seed=0, **cfg):
    from libhdfs3_amd.engine import OutputStream

    model = OutputStreamModel(crc, bpc=cfg.get("bytes_per_checksum", 512), packet_size=cfg.get("packet_size", 65536),
                              block_size=cfg.get("block_size", 64 << 20), append=append)
    gpu = OutputStream(append=append, **cfg)
    scr = Scratch(ctx, seed)
    try:
        pos = 0
        for op, n in ops:
            if op == "w":
                model.write(data[pos:pos + n].tobytes())
                assert gpu.write(data[pos:pos + n]) == n
                pos += n
            elif op == "d":
                model.write(data[pos:pos + n].tobytes())
                (ptr, _), = scr.place([data[pos:pos + n]])
                assert gpu.write_device(ptr, n) == n
                scr.clobber()
                pos += n
            elif op == "v":
                pieces = []
                for k in n:
                    pieces.append(data[pos:pos + k])
                    model.write(pieces[-1].tobytes())
                    pos += k
                entries = scr.place(pieces)
                assert gpu.writev_device(entries) == sum(n)
                scr.clobber()
            elif op == "f":
                model.flush()
                gpu.flush()
                assert [p for p, _ in gpu.packets] == [p for p, _ in model.sent]  # flush drains everything
            elif op == "s":
                model.sync()
                gpu.sync()
            assert gpu.tell() == model.cursor
        if stats_out is not None:
            stats_out.update(gpu.device_stats())
        model.close()
        gpu.close()
    finally:
        scr.free()
    return model.sent, gpu.packets


def assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gp, gi), (wp, wi)) in enumerate(zip(got, want)):
        assert gi == wi, (i, gi, wi)
        assert gp == wp, i


def random_ops(rng, total, sizes):
    """w / d / f / s and vectored calls of 1-40 entries of 0-5000 bytes, empty entries included"""
    ops, left = [], total
    while left > 0:
        r = rng.random()
        if r < 0.10:
            ops.append(("f", 0))
        elif r < 0.14:
            ops.append(("s", 0))
        elif r < 0.55:
            ns = []
            for _ in range(rng.randint(1, 40)):
                k = 0 if rng.random() < 0.15 else min(left - sum(ns), rng.choice([1, 3, 17, 100, 511, 512, 513, 2048,
                                                                                  rng.randint(0, 5000)]))
                ns.append(k)
            ops.append(("v", ns))
            left -= sum(ns)
        else:
            n = min(left, rng.choice(sizes))
            ops.append((rng.choice("wd"), n))
            left -= n
    return ops


# ---- equivalence with the model -------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sequences_match_the_model(gpu_ctx, seed):
    rng = random.Random(seed)
    data = splitmix_bytes(200_000, 90 + seed)
    ops = random_ops(rng, data.nbytes, [1, 3, 100, 511, 512, 513, 2047, 2048, 2049, 4096, 6144, 7000])
    assert sum(1 for op, _ in ops if op == "v") >= 3
    want, got = run_both(gpu_ctx, ops, data, seed=seed, **SMALL)
    assert_same(got, want)


def test_one_call_over_batches_and_a_block_end(gpu_ctx):
    """One vectored call of 30,000 bytes: a batch is 2 packets x 2048 bytes and a block 6144, so the call spans
    seven batches and four block ends; mixed bytes before and after it share its first and last chunk."""
    ns = [700, 0, 5000, 1, 4096, 15, 2048, 513, 6144, 3000, 8483]
    ops = [("w", 100), ("v", ns), ("d", 300), ("v", [5, 5]), ("w", 7)]
    assert sum(ns) == 30000
    data = splitmix_bytes(total_of(ops), 95)
    want, got = run_both(gpu_ctx, ops, data, **SMALL)
    assert_same(got, want)


def test_seven_hundred_one_byte_entries(gpu_ctx):
    ops = [("w", 3), ("v", [1] * 700), ("f", 0), ("v", [1] * 5)]
    data = splitmix_bytes(total_of(ops), 96)
    st = {}
    want, got = run_both(gpu_ctx, ops, data, stats_out=st, **SMALL)
    assert_same(got, want)
    assert st["bytes_from_device"] == 705


def test_append_mode_first_packet_from_a_vectored_call(gpu_ctx):
    """The file ends mid-chunk: the first packet is one chunk of 412 bytes, supplied by the first vectored
    call (and flushed inside, so the partial chunk is re-sent)."""
    append = (3 * BS + 5 * 512 + 100, 5 * 512 + 100)
    rng = random.Random(5)
    ops = [("v", [7, 0, 100]), ("f", 0), ("v", [305, 1000, 3]), ("f", 0)]
    ops += random_ops(rng, 40_000 - total_of(ops), [1, 100, 412, 512, 513, 2048, 5000])
    data = splitmix_bytes(total_of(ops), 97)
    want, got = run_both(gpu_ctx, ops, data, append=append, **SMALL)
    assert_same(got, want)


def test_chunks_of_4096_bytes(gpu_ctx):
    rng = random.Random(4096)
    data = splitmix_bytes(300_000, 98)
    ops = random_ops(rng, data.nbytes, [1, 4095, 4096, 4097, 3 * 4096, 65536, 70000])
    want, got = run_both(gpu_ctx, ops, data, bytes_per_checksum=4096, packet_size=65536, block_size=4096 * 40,
                         batch_packets=3)
    assert_same(got, want)


# ---- launches and bytes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("gap,launches", [(7, 4), (0, 1)])
def test_default_geometry_launches_per_call(gpu_ctx, gap, launches):
    """200 entries x 100 bytes in one call on a fresh default stream: all of them lie in the first packet of
    one batch. With gaps between them in memory they are 200 ranges, 64 to a launch: exactly 4 launches.
    Adjacent in memory (one allocation, back to back) they are one planned range: exactly 1."""
    from libhdfs3_amd.engine import OutputStream

    data = splitmix_bytes(20000, 99)
    scr = Scratch(gpu_ctx, 9)
    model = OutputStreamModel(crc)
    try:
        with OutputStream() as s:
            pieces = [data[100 * i:100 * (i + 1)] for i in range(200)]
            if gap:
                entries = scr.place(pieces, gap=gap)
            else:  # place() deals pieces to the three allocations in turn: take one allocation's run
                (ptr, n), = scr.place([data])
                entries = [(ptr + 100 * i, 100) for i in range(200)]
            before = s.device_stats()
            assert s.writev_device(entries) == 20000
            scr.clobber()
            after = s.device_stats()
            assert after["scatter_launches"] - before["scatter_launches"] == launches
            assert after["bytes_from_device"] - before["bytes_from_device"] == 20000
        model.write(data.tobytes())
        model.close()
        assert_same(s.packets, model.sent)
    finally:
        scr.free()


def test_empty_lists_return_zero_without_a_launch(gpu_ctx):
    from libhdfs3_amd.engine import OutputStream

    scr = Scratch(gpu_ctx, 10)
    try:
        with OutputStream(**SMALL) as s:
            before = gpu_ctx.kernel_launches
            assert s.writev_device([]) == 0
            assert s._lib.hdfs3_output_writev_dev(s.s, None, 0) == 0
            assert s.writev_device([(None, 0), (scr.bufs[0].ptr, 0), (12345, 0)]) == 0
            assert s.tell() == 0
            assert s.device_stats() == {"scatter_launches": 0, "bytes_from_device": 0}
            assert gpu_ctx.kernel_launches == before
        assert s.packets == []  # nothing was ever written: no packet at all
    finally:
        scr.free()


# ---- errors ---------------------------------------------------------------------------------------------

def test_a_host_pointer_entry_is_einval_and_the_stream_goes_on(gpu_ctx):
    from libhdfs3_amd.engine import HdfsIOError, OutputStream

    data = splitmix_bytes(9000, 100)
    model = OutputStreamModel(crc, packet_size=2048, block_size=BS)
    scr = Scratch(gpu_ctx, 11)
    host = np.zeros(64, np.uint8)
    try:
        with OutputStream(**SMALL) as s:
            entries = scr.place([data[:300], data[300:1000]])
            assert s.writev_device(entries) == 1000
            (p0, _), (p1, _) = entries
            last_byte_off = (p0, 1 << 44)  # starts in the allocation, ends far outside every mapping
            for bad in [[(p0, 10), (host.ctypes.data, 64), (p1, 10)], [(p0, 10), (None, 5), (p1, 10)],
                        [(p0, 10), last_byte_off, (p1, 10)], [(p0, (1 << 63) - 1), (p1, 1)]]:
                with pytest.raises(HdfsIOError) as ei:
                    s.writev_device(bad)
                assert ei.value.errno == errno.EINVAL
                assert s.tell() == 1000
            iov = s.dev_iovec([(p0, 10)])
            for args in [(s.s, None, 1), (s.s, iov, -1)]:
                ctypes.set_errno(0)
                assert s._lib.hdfs3_output_writev_dev(*args) == -1 and ctypes.get_errno() == errno.EINVAL
                assert s.tell() == 1000
            scr.clobber()
            entries = scr.place([data[1000:1001], data[1001:5000], data[5000:]])
            assert s.writev_device(entries) == 8000  # not sticky: the same packet sequence
            scr.clobber()
            assert s.device_stats()["bytes_from_device"] == 9000
        for a, b in [(0, 300), (300, 1000), (1000, 1001), (1001, 5000), (5000, 9000)]:
            model.write(data[a:b].tobytes())
        model.close()
        assert_same(s.packets, model.sent)  # a model that never saw the refused calls
    finally:
        scr.free()


def test_a_failing_sink_fails_the_stream_under_vectored_writes(gpu_ctx):
    from libhdfs3_amd.engine import HdfsIOError, OutputStream

    calls = []

    def sink(pkt, info):
        calls.append(info["seqno"])
        return -errno.ENOSPC if info["seqno"] == 2 else 0

    data = splitmix_bytes(CAP // 2, 101)
    scr = Scratch(gpu_ctx, 12)
    try:
        s = OutputStream(sink=sink, **SMALL)
        entries = scr.place([data[i:i + 4096] for i in range(0, data.nbytes, 4096)])
        with pytest.raises(HdfsIOError) as ei:  # the call returns, with the sink's error
            s.writev_device(entries)
        assert ei.value.errno == errno.ENOSPC
        scr.clobber()  # its placements were waited for: nothing reads the sources any more
        for call in (lambda: s.writev_device(entries[:2]), lambda: s.write_device(entries[0][0], 10),
                     lambda: s.write(data[:10])):
            with pytest.raises(HdfsIOError) as ei:
                call()
            assert ei.value.errno == errno.EIO
        assert calls[:3] == [0, 1, 2]
        with pytest.raises(HdfsIOError):
            s.close()
    finally:
        scr.free()


# ---- the hdfs.h form ------------------------------------------------------------------------------------

def test_hdfs_h_layer_writev_dev(gpu_ctx):
    """hdfsWrite, hdfs3_fs_writev_dev and hdfs3_fs_write_dev on one hdfsFile over a packet sink: the packets of
    the model fed the same pieces one hdfsWrite each."""
    from libhdfs3_amd import _native

    lib = _native.lib()
    data = splitmix_bytes(30_000, 102)
    cuts = [0, 1000, 1007, 4000, 4000, 9000, 9513, 20000, 26000, 30000]  # w | v: 5 entries, one empty | d | v: 2 entries
    model = OutputStreamModel(crc, packet_size=2048, block_size=BS)
    got = []

    def sink(_user, pkt, n, info):
        got.append(ctypes.string_at(pkt, n))
        return 0

    cb = _native.PACKET_SINK(sink)
    wopts = _native.WriterOpts(0, 512, 2048, BS, 2)
    fs = lib.hdfs3_fs_new(b"writev-dev-test", None, ctypes.byref(wopts))
    assert fs
    scr = Scratch(gpu_ctx, 13)
    try:
        assert lib.hdfs3_fs_set_sink(fs, b"/v", ctypes.cast(cb, ctypes.c_void_p), None) == 0
        f = lib.hdfsOpenFile(fs, b"/v", os.O_WRONLY | os.O_CREAT, 0, 0, 0)
        assert f, lib.hdfsGetLastError()
        assert lib.hdfsWrite(fs, f, data.ctypes.data, 1000) == 1000
        entries = scr.place([data[a:b] for a, b in zip(cuts[1:6], cuts[2:7])])
        iov = (_native.DevIovec * 5)(*[_native.DevIovec(p, n) for p, n in entries])
        ctypes.set_errno(0)
        assert lib.hdfs3_fs_writev_dev(fs, f, None, 1) == -1 and ctypes.get_errno() == errno.EINVAL
        host = (_native.DevIovec * 1)(_native.DevIovec(data.ctypes.data, 16))
        assert lib.hdfs3_fs_writev_dev(fs, f, host, 1) == -1 and ctypes.get_errno() == errno.EINVAL
        assert lib.hdfsTell(fs, f) == 1000
        assert lib.hdfs3_fs_writev_dev(fs, f, iov, 5) == 9513 - 1000, lib.hdfsGetLastError()
        scr.clobber()
        (p, n), = scr.place([data[9513:20000]])
        assert lib.hdfs3_fs_write_dev(fs, f, p, n) == n
        scr.clobber()
        entries = scr.place([data[20000:26000], data[26000:]])
        iov = (_native.DevIovec * 2)(*[_native.DevIovec(p, n) for p, n in entries])
        assert lib.hdfs3_fs_writev_dev(fs, f, iov, 2) == 10000, lib.hdfsGetLastError()
        scr.clobber()
        assert lib.hdfsTell(fs, f) == data.nbytes
        assert lib.hdfsCloseFile(fs, f) == 0, lib.hdfsGetLastError()
    finally:
        lib.hdfsDisconnect(fs)
        scr.free()
    for a, b in zip(cuts, cuts[1:]):
        model.write(data[a:b].tobytes())
    model.close()
    assert got == [p for p, _ in model.sent]
