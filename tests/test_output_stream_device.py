"""GPU: hdfs3_output_write_dev (the output stream's write from device memory) and its hdfs.h form
hdfs3_fs_write_dev. The expected value is the one test_output_stream.py uses: every packet handed to the
sink must be byte-identical to what the reference's OutputStreamImpl + Packet produce for the same call
sequence (tests/writer_model.py, CRC words from the oracle), whether a piece came from host or from device
memory. Ops: ("w", n) hdfs3_output_write of the next n bytes, ("d", n) hdfs3_output_write_dev of the next n
bytes, ("f", 0) flush, ("s", 0) sync.

By default every device write goes through a scratch buffer that is overwritten with a canary (on another
stream, synchronised) as soon as the call has returned: a write_dev that returned before its source was
read would put canary bytes into the packets."""
import ctypes
import errno
import os
import random

import numpy as np
import pytest

from util import oracle_compute, oracle_crc, splitmix_bytes
from writer_model import OutputStreamModel

pytestmark = pytest.mark.gpu

CANARY = 0xC3
BS = 512 * 12
SMALL = dict(packet_size=2048, block_size=BS)  # 4 chunks per packet, 3 packets per block


def crc(b: bytes) -> int:
    return oracle_crc(np.frombuffer(b, np.uint8)) if b else 0


def ops_of(text):
    """'w100 d300 f s' -> [("w", 100), ("d", 300), ("f", 0), ("s", 0)]"""
    return [(t[0], int(t[1:] or 0)) for t in text.split()]


def total_of(ops):
    return sum(n for op, n in ops if op in "wd")


class Source:
    """The device side of a run. clobber: each write's bytes are uploaded to a scratch buffer `off` bytes
    into its allocation, written from there, and the scratch is overwritten at once. Otherwise the whole
    data sits in one buffer that is only ever read, and must be unchanged at the end."""

    def __init__(self, ctx, data, off=0, clobber=True):
        from libhdfs3_amd.engine import DeviceBuffer

        self.ctx, self.data, self.off, self.clobber = ctx, data, off, clobber
        biggest = data.nbytes
        self.buf = DeviceBuffer(off + biggest + 64)
        ctx.memset(self.buf, CANARY, self.buf.nbytes)
        if not clobber:
            ctx.upload(data, self.buf, off)

    def write(self, stream, pos, n):
        if not self.clobber:
            return stream.write_device(self.buf.ptr + self.off + pos, n)
        self.ctx.upload(self.data[pos:pos + n], self.buf, self.off)
        got = stream.write_device(self.buf.ptr + self.off, n)
        self.ctx.memset(self.buf, CANARY, n, self.off)  # synchronises its own stream
        return got

    def check_untouched(self):
        exp = np.full(self.buf.nbytes, CANARY, np.uint8)
        if not self.clobber:
            exp[self.off:self.off + self.data.nbytes] = self.data
        assert np.array_equal(self.ctx.download(self.buf, self.buf.nbytes), exp)

    def free(self):
        self.buf.free()


def run_both(ctx, ops, data, off=0, clobber=True, append=None, stream_out=None, **cfg):
    from libhdfs3_amd.engine import OutputStream

    model = OutputStreamModel(crc, bpc=cfg.get("bytes_per_checksum", 512), packet_size=cfg.get("packet_size", 65536),
                              block_size=cfg.get("block_size", 64 << 20), append=append)
    gpu = OutputStream(append=append, **cfg)
    src = Source(ctx, data, off, clobber)
    try:
        pos = 0
        for op, n in ops:
            if op in "wd":
                chunk = data[pos:pos + n]
                model.write(chunk.tobytes())
                assert (gpu.write(chunk) if op == "w" else src.write(gpu, pos, n)) == n
                pos += n
                assert gpu.tell() == model.cursor
            elif op == "f":
                model.flush()
                gpu.flush()
                assert [p for p, _ in gpu.packets] == [p for p, _ in model.sent]  # flush drains everything
            elif op == "s":
                model.sync()
                gpu.sync()
        if stream_out is not None:
            stream_out.update(gpu.device_stats(), **gpu.stats())
        model.close()
        gpu.close()
        src.check_untouched()
    finally:
        src.free()
    return model.sent, gpu.packets


def assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gp, gi), (wp, wi)) in enumerate(zip(got, want)):
        assert gi == wi, (i, gi, wi)
        assert gp == wp, i


def random_mix(rng, total, sizes, flush_p=0.12):
    ops, left = [], total
    while left > 0:
        r = rng.random()
        if r < flush_p:
            ops.append(("f", 0))
        elif r < flush_p * 1.3:
            ops.append(("s", 0))
        else:
            n = min(left, rng.choice(sizes))
            ops.append((rng.choice("wd"), n))
            left -= n
    return ops


# ---- device-only writes ------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1, 7, 15])
def test_device_only_writes_match_the_model(gpu_ctx, off):
    """One write_dev of each size (inside a chunk, around the 16-byte line, around a chunk, two packets, many
    blocks), the source starting `off` bytes into its allocation."""
    data = splitmix_bytes(70000, 11 + off)
    for size in [1, 15, 16, 17, 511, 512, 513, 4096, 70000]:
        want, got = run_both(gpu_ctx, [("d", size)], data[:size], off=off, batch_packets=2, **SMALL)
        assert_same(got, want)
    # and all of them on one stream, one after the other
    ops = [("d", n) for n in [1, 15, 16, 17, 511, 512, 513, 4096]]
    want, got = run_both(gpu_ctx, ops, data[:total_of(ops)], off=off, batch_packets=3, **SMALL)
    assert_same(got, want)


# ---- mixed host and device writes --------------------------------------------------------------------

MIXES = [
    # inside a chunk, across a packet end (2048), a batch end (2 packets) and a block end (6144)
    "w100 d300 w112 d5000 w1 d1 w510 d2048 w2047 d1 w6144 d6144 w3 d3",
    "d100 w300 d112 w5000 d1 w1 d510 w2048 d2047 w1 d6144 w6144 d3 w3",
    # every byte of a chunk from the other side in turn
    " ".join(("w1 d1 " * 300).split()),
    # a packet whose first and last chunk are host bytes around placed ones, then the reverse
    "w512 d1024 w512 d512 w1024 d512 w2048 d2048 d2048 w2048",
]


@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_mixed_host_and_device_writes(gpu_ctx, mix, batch):
    ops = ops_of(MIXES[mix])
    data = splitmix_bytes(total_of(ops), 20 + mix)
    want, got = run_both(gpu_ctx, ops, data, off=mix, batch_packets=batch, **SMALL)
    assert_same(got, want)


@pytest.mark.parametrize("seed,batch", [(1, 2), (2, 3), (3, 2)])
def test_seeded_random_mix(gpu_ctx, seed, batch):
    rng = random.Random(seed)
    data = splitmix_bytes(150_000, 30 + seed)
    ops = random_mix(rng, data.nbytes, [1, 3, 100, 511, 512, 513, 2047, 2048, 2049, 4096, 6144, 7000, 20000])
    want, got = run_both(gpu_ctx, ops, data, off=seed, batch_packets=batch, **SMALL)
    assert_same(got, want)


# ---- flush and sync with device-sourced partial chunks -----------------------------------------------

@pytest.mark.parametrize("text", [
    "d700 f d1300",
    "d700 f w10",
    "d700 f f s",
    "d10 s s",
    f"d{512 * 4 + 1} f",
    "w200 d100 f d100 f w100 f d12 s d2000",  # the re-sent partial chunk itself mixed, re-sent three times
])
def test_flush_and_sync_with_device_partial_chunks(gpu_ctx, text):
    ops = ops_of(text)
    data = splitmix_bytes(total_of(ops), 3)
    want, got = run_both(gpu_ctx, ops, data, off=5, batch_packets=2, **SMALL)
    assert got == want


# ---- append ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("append", [
    (3 * BS + 5 * 512 + 100, 5 * 512 + 100),  # ends mid-chunk: one 412-byte chunk first
    (4 * BS - 1, BS - 1),                     # one byte short of a block
    (4 * BS, -1),                             # on a block boundary: no last block
])
def test_append_with_device_writes(gpu_ctx, append):
    rng = random.Random(append[0])
    data = splitmix_bytes(40_000, 40)
    first = 7 if append[1] != BS - 1 else 1  # a first flush inside the partial chunk
    ops = [("d", first), ("f", 0)] + random_mix(rng, data.nbytes - first, [1, 100, 412, 512, 513, 2048, 5000, 7000],
                                                flush_p=0.15)
    want, got = run_both(gpu_ctx, ops, data, off=3, append=append, batch_packets=3, **SMALL)
    assert_same(got, want)


# ---- chunk sizes: the compute routes a host batch takes, over placed bytes -----------------------------

@pytest.mark.parametrize("bpc,packet_size,block_size,batch", [
    (512, 65536, 512 * 400, 3),
    (4096, 65536, 4096 * 40, 3),
    (100, 1000, 100 * 37, 5),        # odd chunk size, ragged everything
    (8192, 65536, 8192 * 24, 2),     # chunks above 4 KiB: pieces + combine
    (12288, 65536, 12288 * 18, 2),   # 6 chunks = 18 rounds per packet
])
def test_chunk_sizes(gpu_ctx, bpc, packet_size, block_size, batch):
    rng = random.Random(bpc)
    data = splitmix_bytes(300_000 if bpc != 100 else 30_000, bpc)
    sizes = [1, bpc - 1, bpc, bpc + 1, 3 * bpc, 65536, 70000] if bpc != 100 else [1, 99, 100, 101, 900, 1000, 3700]
    ops = random_mix(rng, data.nbytes, sizes, flush_p=0.05)
    want, got = run_both(gpu_ctx, ops, data, off=9, bytes_per_checksum=bpc, packet_size=packet_size,
                         block_size=block_size, batch_packets=batch)
    assert_same(got, want)


# ---- the default shape, once: full 64-packet batches (the pitch walk), one placement launch per batch ----

def test_default_shape_long_device_writes(gpu_ctx):
    data = splitmix_bytes(9 << 20, 50)
    ops = []
    for i in range(9):
        ops.append(("d", 1 << 20))
        if i in (2, 6):
            ops.append(("f", 0))
    st = {}
    want, got = run_both(gpu_ctx, ops, data, off=1, clobber=False, stream_out=st, block_size=8 << 20)
    assert_same(got, want)
    assert st["bytes_from_device"] == data.nbytes
    # a call places its bytes with one launch per batch it touches: a 1 MiB call lies in one batch of
    # 64 x 65,024 bytes or straddles two
    assert 9 <= st["scatter_launches"] <= 18


# ---- the source: reusable on return, never written ---------------------------------------------------

def test_source_is_never_written(gpu_ctx):
    """The whole data in one device buffer that is only read, canary before and after it: byte-identical
    after close (Source.check_untouched), with mixed writes and flushes in between."""
    rng = random.Random(7)
    data = splitmix_bytes(60_000, 60)
    ops = random_mix(rng, data.nbytes, [1, 17, 512, 2048, 5000, 9000])
    want, got = run_both(gpu_ctx, ops, data, off=13, clobber=False, batch_packets=2, **SMALL)
    assert_same(got, want)


def test_source_is_reusable_when_the_call_returns(gpu_ctx):
    """64 KiB packets, so placements are large enough to still be running if the call did not wait: the
    scratch source is overwritten with the canary after every write_dev (Source.write)."""
    data = splitmix_bytes(3 << 20, 61)
    ops = [("d", n) for n in [1 << 20, 300_000, 65536, 1, 700_000]]
    ops.append(("d", data.nbytes - total_of(ops)))
    want, got = run_both(gpu_ctx, ops, data, off=7, batch_packets=4, block_size=1 << 20)
    assert_same(got, want)
    assert not any(bytes([CANARY]) * 64 in p for p, _ in got)


# ---- errors ------------------------------------------------------------------------------------------

def test_a_host_pointer_is_einval_and_the_stream_goes_on(gpu_ctx):
    from libhdfs3_amd.engine import HdfsIOError, OutputStream

    data = splitmix_bytes(5000, 70)
    model = OutputStreamModel(crc, packet_size=2048, block_size=BS)
    src = Source(gpu_ctx, data, off=2, clobber=False)
    host = np.zeros(64, np.uint8)
    try:
        with OutputStream(batch_packets=2, **SMALL) as s:
            assert s.write_device(src.buf.ptr + 2, 300) == 300
            for bad in [(host.ctypes.data, 64), (None, 16), (src.buf.ptr, 0), (src.buf.ptr, -1)]:
                with pytest.raises(HdfsIOError) as ei:
                    s.write_device(*bad)
                assert ei.value.errno == errno.EINVAL
                assert s.tell() == 300
            assert s.write_device(src.buf.ptr + 2 + 300, 4700) == 4700  # not sticky: the same packet sequence
            assert s.device_stats()["bytes_from_device"] == 5000
        model.write(data[:300].tobytes())
        model.write(data[300:].tobytes())
        model.close()
        assert s.packets == model.sent
    finally:
        src.free()


def test_a_failing_sink_fails_the_stream_under_device_writes(gpu_ctx):
    from libhdfs3_amd.engine import HdfsIOError, OutputStream

    calls = []

    def sink(pkt, info):
        calls.append(info["seqno"])
        return -errno.ENOSPC if info["seqno"] == 2 else 0

    data = splitmix_bytes(1 << 20, 71)
    src = Source(gpu_ctx, data, clobber=False)
    try:
        s = OutputStream(sink=sink, batch_packets=1)
        with pytest.raises(HdfsIOError) as ei:  # the call returns, with the sink's error
            for off in range(0, data.nbytes, 65536):
                s.write_device(src.buf.ptr + off, 65536)
        assert ei.value.errno == errno.ENOSPC
        with pytest.raises(HdfsIOError) as ei:
            s.write_device(src.buf.ptr, 10)
        assert ei.value.errno == errno.EIO
        with pytest.raises(HdfsIOError) as ei:
            s.write(data[:10])
        assert ei.value.errno == errno.EIO
        assert calls[:3] == [0, 1, 2]
        with pytest.raises(HdfsIOError):
            s.close()
        src.check_untouched()
    finally:
        src.free()


def test_device_stats(gpu_ctx):
    from libhdfs3_amd.engine import OutputStream

    data = splitmix_bytes(10_000, 72)
    with OutputStream(batch_packets=2, **SMALL) as s:
        s.write(data)
        s.flush()
        assert s.device_stats() == {"scatter_launches": 0, "bytes_from_device": 0}  # a host-only stream
    st = {}
    run_both(gpu_ctx, ops_of("d1"), data[:1], stream_out=st, batch_packets=2, **SMALL)
    assert st["bytes_from_device"] == 1 and st["scatter_launches"] == 1
    st = {}
    ops = ops_of("w100 d300 d4000 w50 d5550")
    run_both(gpu_ctx, ops, data, stream_out=st, batch_packets=2, **SMALL)
    assert st["bytes_from_device"] == 300 + 4000 + 5550
    assert st["scatter_launches"] >= 3  # at least one per call


# ---- through datanodes ---------------------------------------------------------------------------------

HOST = "127.0.0.1"


@pytest.fixture
def nodes():
    from loopback import LoopbackDatanode

    dns = [LoopbackDatanode() for _ in range(2)]
    yield dns
    for d in dns:
        d.stop()


def test_round_trip_device_to_datanodes_to_device(gpu_ctx, nodes):
    """write_device through hdfs3_output_open_pipeline into a 2-node pipeline, 3 blocks of 1 MiB; every
    replica stores the bytes and the oracle's words; read_dev brings them back into a canary-filled
    device buffer, downloaded whole."""
    from libhdfs3_amd.engine import DeviceBuffer, InputStream, OutputStream, Pipeline

    bs = 1 << 20
    data = splitmix_bytes(3 * bs, 80)
    chain = [(HOST, d.port) for d in nodes]
    src = Source(gpu_ctx, data, off=3, clobber=False)
    dest = DeviceBuffer(data.nbytes + 128)
    try:
        with Pipeline([(300 + i, chain) for i in range(3)]) as pipe:
            with OutputStream(pipeline=pipe, block_size=bs) as out:
                pos = 0
                for n in [700_001, 1, 1 << 20, 65536]:
                    assert out.write_device(src.buf.ptr + 3 + pos, n) == n
                    pos += n
                out.flush()
                assert pipe.stats()["acks"] == pipe.stats()["packets"]
                assert out.write_device(src.buf.ptr + 3 + pos, data.nbytes - pos) == data.nbytes - pos
                assert out.device_stats()["bytes_from_device"] == data.nbytes
            assert pipe.stats()["block_bytes_acked"] == [bs, bs, bs]
        for d in nodes:
            assert d.wait_finalized(3) == 3
            assert d.write_stats()["checksum_errors"] == 0
            for i in range(3):
                got, words, bpc = d.get_block(300 + i)
                want = data[i * bs:(i + 1) * bs]
                assert bpc == 512 and np.array_equal(got, want)
                assert np.array_equal(words, oracle_compute(want, 512))
        gpu_ctx.memset(dest, CANARY, dest.nbytes)
        with InputStream([(300 + i, bs, [(HOST, nodes[1].port)]) for i in range(3)]) as s:
            pos = 0
            while True:
                n = s.read_into_device(dest.ptr + 64 + pos, min(900_000, data.nbytes + 16 - pos))
                if n == 0:
                    break
                pos += n
        assert pos == data.nbytes
        exp = np.full(dest.nbytes, CANARY, np.uint8)
        exp[64:64 + data.nbytes] = data
        assert np.array_equal(gpu_ctx.download(dest, dest.nbytes), exp)
        src.check_untouched()
    finally:
        src.free()
        dest.free()


def test_hdfs_h_layer_write_dev(gpu_ctx, nodes):
    """A file written half with hdfsWrite and half with hdfs3_fs_write_dev through a pipeline, read back
    with hdfsRead."""
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import _located_blocks

    lib = _native.lib()
    bs = 1 << 20
    data = splitmix_bytes(bs + 300_000, 81)
    half = 650_001
    wopts = _native.WriterOpts(0, 512, 65536, bs, 8)
    fs = lib.hdfs3_fs_new(b"write-dev-test", None, ctypes.byref(wopts))
    assert fs
    src = Source(gpu_ctx, data, off=1, clobber=False)
    try:
        chain = [(HOST, d.port) for d in nodes]
        arr, keep = _located_blocks([(400 + i, 0, chain) for i in range(2)], b"BP-loopback", 1)
        assert lib.hdfs3_fs_set_pipeline(fs, b"/w", arr, 2) == 0
        f = lib.hdfsOpenFile(fs, b"/w", os.O_WRONLY | os.O_CREAT, 0, 0, 0)
        assert f, lib.hdfsGetLastError()
        assert lib.hdfsWrite(fs, f, data.ctypes.data, half) == half
        ctypes.set_errno(0)
        assert lib.hdfs3_fs_write_dev(fs, f, None, 16) == -1 and ctypes.get_errno() == errno.EINVAL
        assert lib.hdfs3_fs_write_dev(fs, f, data.ctypes.data, 16) == -1 and ctypes.get_errno() == errno.EINVAL
        assert lib.hdfsTell(fs, f) == half
        rest = data.nbytes - half
        assert lib.hdfs3_fs_write_dev(fs, f, src.buf.ptr + 1 + half, rest) == rest, lib.hdfsGetLastError()
        assert lib.hdfsTell(fs, f) == data.nbytes
        assert lib.hdfsCloseFile(fs, f) == 0, lib.hdfsGetLastError()
        g = lib.hdfsOpenFile(fs, b"/w", os.O_RDONLY, 0, 0, 0)
        assert g, lib.hdfsGetLastError()
        ctypes.set_errno(0)
        assert lib.hdfs3_fs_write_dev(fs, g, src.buf.ptr, 16) == -1 and ctypes.get_errno() == errno.EINVAL  # a reader
        out = np.zeros(data.nbytes + 1, np.uint8)
        got = 0
        while True:
            r = lib.hdfsRead(fs, g, out.ctypes.data + got, min(1 << 20, out.nbytes - got))
            assert r >= 0, lib.hdfsGetLastError()
            if r == 0:
                break
            got += r
        assert lib.hdfsCloseFile(fs, g) == 0
        assert got == data.nbytes and np.array_equal(out[:got], data)
        src.check_untouched()
    finally:
        lib.hdfsDisconnect(fs)
        src.free()
