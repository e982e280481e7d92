"""GPU: hdfs3_local_reader_read_dev, the short-circuit reader's delivery into device memory. Same contract as
hdfs3_local_reader_read (test_local_reader.py): every chunk verified, the short tail included; nothing of the
buffer_size buffer holding a bad chunk is returned; then -EIO. In addition the bytes are in place when the
call returns and nothing past the returned count is ever written: the destination is pre-filled with a
canary, starts 3 bytes into its allocation and is downloaded whole. Windows are 2 x 64 KiB and the block is
five windows + 777 bytes, so one call spans six windows (the last one short) and six chained deliveries."""
import errno
import struct

import numpy as np
import pytest

from util import oracle_compute, splitmix_bytes

pytestmark = pytest.mark.gpu

CANARY = 0x5C
BUF = 64 << 10
WINDOW = 2 * BUF
N = 5 * WINDOW + 777
OPTS = dict(buffer_size=BUF, window_buffers=2)


@pytest.fixture(params=["default", "mmap", "pread"])
def staging(request, monkeypatch):
    """Every staging of the short-circuit reader must deliver identical results: default
    (verified windows pread in parallel into pinned arenas; unverified reads copied straight
    out of the mmap'd file), HDFS3_LOCAL_MMAP=1 (verified windows registered and DMA'd from the
    mapping) and HDFS3_LOCAL_MMAP=0 (no mapping at all)."""
    if request.param == "default":
        monkeypatch.delenv("HDFS3_LOCAL_MMAP", raising=False)
    else:
        monkeypatch.setenv("HDFS3_LOCAL_MMAP", "1" if request.param == "mmap" else "0")
    return request.param


def write_block(path, name, data, bpc=512, ctype=2, crc=None):
    d, m = path / f"{name}", path / f"{name}.meta"
    d.write_bytes(data.tobytes())
    words = b"" if ctype == 0 else (oracle_compute(data, bpc) if crc is None else crc).tobytes()
    m.write_bytes(struct.pack(">hBI", 1, ctype, bpc) + words)
    return str(d), str(m)


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    """The clean block and its words, computed and written once: data, words at bpc 512, {bpc: (file, meta)}."""
    path = tmp_path_factory.mktemp("local_dev")
    data = splitmix_bytes(N, 0x10CA1)
    words = oracle_compute(data, 512)
    files = {512: write_block(path, "blk_512", data, 512, crc=words), 4096: write_block(path, "blk_4096", data, 4096)}
    return data, words, files


class Dest:
    """A canary-filled device buffer; the destination starts 3 bytes into it."""

    def __init__(self, ctx, nbytes, off=3):
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
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]

    def free(self):
        self.buf.free()


def _read_dev(r, dest, length, piece):
    pos = 0
    while pos < length:
        got = r.read_into_device(dest.ptr + pos, min(piece, length - pos))
        if got == 0:
            break
        pos += got
    return pos


@pytest.mark.parametrize("piece", [N, 100_000])
@pytest.mark.parametrize("bpc", [512, 4096])
def test_whole_block_into_device_memory(gpu_ctx, block, staging, bpc, piece):
    from libhdfs3_amd.engine import LocalBlockReader

    data, _, files = block
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(*files[bpc], **OPTS) as r:
            if piece == N:
                assert r.read_into_device(dest.ptr, N) == N  # one call spans every window
            else:
                assert _read_dev(r, dest, N, piece) == N
            assert r.read_into_device(dest.ptr, 16) == 0  # end of block
            st, host = r.device_stats(), r.stats()
        dest.check(data)
        assert st["bytes_delivered"] == N and st["deliver_launches"] >= 5
        assert host["bytes_per_checksum"] == bpc and host["gpu_batches"] == 6
        assert (host["mapped_windows"] == 6) if staging == "mmap" else host["mapped_windows"] == 0
    finally:
        dest.free()


def test_offset_reads(gpu_ctx, block, staging):
    from libhdfs3_amd.engine import LocalBlockReader

    data, _, files = block
    for off in [1, 511, 517, WINDOW + 1, N - 10, N]:
        dest = Dest(gpu_ctx, N - off)
        try:
            with LocalBlockReader(*files[512], offset=off, **OPTS) as r:
                assert _read_dev(r, dest, N - off + 5, 300_001) == N - off, off
            dest.check(data[off:])
        finally:
            dest.free()


@pytest.mark.parametrize("where", [0, 70_000, WINDOW + 5, N - 1])
def test_corruption_withholds_the_whole_local_buffer(gpu_ctx, block, tmp_path, staging, where):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import LocalBlockReader

    data, words, _ = block
    bad = data.copy()
    bad[where] ^= 0x20  # the last position is inside the short tail chunk: checked locally
    d, m = write_block(tmp_path, "blk_bad", bad, crc=words)
    count = where // BUF * BUF
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(d, m, **OPTS) as r:
            if count:
                assert r.read_into_device(dest.ptr, N) == count  # one call: every later window already enqueued
            for _ in range(2):  # the call that finds it with nothing to deliver, and every call after: sticky
                with pytest.raises(Hdfs3CrcError) as ei:
                    r.read_into_device(dest.ptr + count, N - count)
                assert ei.value.rc == -errno.EIO and "ChecksumException" in str(ei.value)
            assert r.device_stats()["bytes_delivered"] == count
        dest.check(data[:count])  # everything past the count is still canary
    finally:
        dest.free()


def test_corruption_met_by_small_reads(gpu_ctx, block, tmp_path):
    """Reads that end inside the bad window but before its bad buffer are served; the reader stops exactly at
    the buffer that holds the bad chunk, whichever call reaches it."""
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import LocalBlockReader

    data, words, _ = block
    bad = data.copy()
    where = WINDOW + BUF + 100  # window 1, its second buffer
    bad[where] ^= 1
    d, m = write_block(tmp_path, "blk_bad_small", bad, crc=words)
    count = where // BUF * BUF
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(d, m, **OPTS) as r:
            pos = 0
            with pytest.raises(Hdfs3CrcError) as ei:
                while True:
                    got = r.read_into_device(dest.ptr + pos, 50_000)
                    assert got > 0
                    pos += got
            assert ei.value.rc == -errno.EIO and pos == count
        dest.check(data[:count])
    finally:
        dest.free()


def test_corrupt_meta_word(gpu_ctx, block, tmp_path, staging):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import LocalBlockReader

    data, words, _ = block
    crc = words.copy()
    crc[4 * 100] ^= 1  # chunk 100 = bytes [51200, 51712): the first buffer
    d, m = write_block(tmp_path, "blk_meta", data, crc=crc)
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(d, m, **OPTS) as r:
            with pytest.raises(Hdfs3CrcError) as ei:
                r.read_into_device(dest.ptr, N)
            assert ei.value.rc == -errno.EIO and "chunk 100" in str(ei.value)
        dest.check(data[:0])
    finally:
        dest.free()


@pytest.mark.parametrize("kind", ["null_type", "verify_off"])
def test_unverified_blocks_deliver_every_byte_without_a_kernel(gpu_ctx, block, tmp_path, staging, kind):
    from libhdfs3_amd.engine import LocalBlockReader

    data, words, _ = block
    bad = data.copy()
    bad[1234] ^= 1
    if kind == "null_type":
        d, m = write_block(tmp_path, "blk_null", bad, ctype=0)
        kw = {}
    else:
        d, m = write_block(tmp_path, "blk_off", bad, crc=words)
        kw = {"verify": False}
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(d, m, **OPTS, **kw) as r:
            assert _read_dev(r, dest, N, 300_001) == N
            assert r.read_into_device(dest.ptr, 16) == 0
            st = r.device_stats()
        dest.check(bad)
        assert st == {"deliver_launches": 0, "bytes_delivered": N}
    finally:
        dest.free()


def test_a_host_pointer_is_refused_and_the_reader_stays_usable(gpu_ctx, block):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import LocalBlockReader

    data, _, files = block
    host = np.full(4096, CANARY, np.uint8)
    dest = Dest(gpu_ctx, N)
    try:
        with LocalBlockReader(*files[512], **OPTS) as r:
            for args in [(host.ctypes.data, 4096), (dest.ptr, 0), (dest.ptr, -5), (None, 16)]:
                with pytest.raises(Hdfs3CrcError) as ei:
                    r.read_into_device(*args)
                assert ei.value.rc == -errno.EINVAL
            assert np.all(host == CANARY)
            assert _read_dev(r, dest, N, N) == N
        dest.check(data)
    finally:
        dest.free()


def test_host_and_device_reads_alternate_on_one_reader(gpu_ctx, block, staging):
    from libhdfs3_amd.engine import LocalBlockReader

    data, _, files = block
    dest = Dest(gpu_ctx, N)
    host = np.zeros(N, np.uint8)
    dev_parts = []
    try:
        with LocalBlockReader(*files[512], **OPTS) as r:
            pos, turn = 0, 0
            while pos < N:
                n = min(100_003, N - pos)
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
            exp[3 + p:3 + p + n] = data[p:p + n]
            host[p:p + n] = data[p:p + n]  # the device's share, checked just above
        assert np.array_equal(got, exp)
        assert np.array_equal(host, data)
        assert st["bytes_delivered"] == sum(n for _, n in dev_parts)
    finally:
        dest.free()


def test_host_and_device_reads_agree_call_by_call(gpu_ctx, tmp_path):
    """read() and read_dev() on the same block give the same sequence of return values up to and including
    the first error, the same bytes, and the same answer to one more call. Chunks of 512, buffers of 4 KiB,
    windows of two: three windows + 700 bytes is four windows (more than the three slots) and ends in a short
    chunk. Clean, and one flipped byte in the first buffer, in the second buffer of the second window, in the
    first chunk of the third window and in the tail chunk; opened at 0 and at 513 (buffers and windows are then
    counted from byte 512); calls of 1000 bytes, of a window, and of the whole block."""
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import LocalBlockReader

    bpc, buf, window = 512, 4096, 8192
    n = 3 * window + 700
    opts = dict(buffer_size=buf, window_buffers=2)
    data = splitmix_bytes(n, 0xA9EE)
    words = oracle_compute(data, bpc)

    def calls(read, length, piece):
        """every call's return value (an error as ("error", rc)) until an error or the end, and one call more"""
        seq, pos, ended = [], 0, False
        while len(seq) < 100:
            try:
                got = read(pos, min(piece, max(length - pos, 1)))
            except Hdfs3CrcError as e:
                got = ("error", e.rc, "ChecksumException" in str(e))
            seq.append(got)
            if ended:
                return seq, pos
            if isinstance(got, tuple) or got == 0:
                ended = True
            else:
                pos += got
        raise AssertionError(seq[:8])

    compared = 0
    for off in (0, 513):
        first = off // bpc * bpc
        flips = {"clean": None, "first_buffer": first + 500, "window1_buffer1": first + window + buf + 300,
                 "window2_chunk0": first + 2 * window + 5, "tail_chunk": n - 3}
        for name, where in flips.items():
            blk = data.copy()
            if where is not None:
                blk[where] ^= 0x40
            d, m = write_block(tmp_path, f"blk_{off}_{name}", blk, bpc, crc=words)
            # the rule both reads state: nothing of the buffer, counted from `first`, that holds the bad chunk
            good = n if where is None else first + (where // bpc * bpc - first) // buf * buf
            want = blk[off:max(good, off)]
            for piece in (1000, window, n):
                host = np.full(n - off + 64, CANARY, np.uint8)
                with LocalBlockReader(d, m, offset=off, **opts) as r:
                    h_seq, h_pos = calls(lambda pos, k: r.read_into(host, pos, k), n - off, piece)
                dest = Dest(gpu_ctx, n - off)
                try:
                    with LocalBlockReader(d, m, offset=off, **opts) as r:
                        d_seq, d_pos = calls(lambda pos, k: r.read_into_device(dest.ptr + pos, k), n - off, piece)
                    case = (off, name, piece)
                    assert h_seq == d_seq, (case, h_seq[-4:], d_seq[-4:])
                    assert h_pos == d_pos == want.nbytes, (case, h_pos, d_pos, want.nbytes)
                    assert isinstance(h_seq[-1], tuple) == (where is not None), (case, h_seq[-4:])
                    assert np.array_equal(host[:h_pos], want) and np.all(host[h_pos:] == CANARY), case
                    dest.check(want)  # and canary everywhere past the count
                    compared += 1
                finally:
                    dest.free()
    assert compared == 2 * 5 * 3
