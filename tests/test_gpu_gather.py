"""GPU: the range-gather kernel (csrc/crc32c_gather.hip) through hdfs3_gather_dev_async, and the
verify-then-deliver call hdfs3_crc32c_verify_packets_gather_dev. The expected destination is numpy
slicing over a canary-filled buffer that is downloaded whole, so a byte written outside a range, or a
line read back and merged, shows as a damaged canary or a damaged neighbour."""
import numpy as np
import pytest

from util import oracle_compute, splitmix_bytes

pytestmark = pytest.mark.gpu

CANARY = 0xA5
MAX_RANGES = 64  # kGatherMaxRanges (csrc/launch_plan.h)


def _gather(ctx, src, dst_len, ranges, src_base=0, dst_base=0):
    """ranges over a source uploaded at +src_base of its allocation into a canary destination that starts at
    +dst_base of its allocation; returns (destination as downloaded, expected)."""
    from libhdfs3_amd.engine import DeviceBuffer

    d_src = DeviceBuffer(src.nbytes + src_base)
    d_dst = DeviceBuffer(dst_len + dst_base + 64)
    try:
        ctx.upload(src, d_src, src_base)
        ctx.memset(d_dst, CANARY, d_dst.nbytes)
        ctx.gather_dev(d_dst.ptr + dst_base, dst_len, d_src.ptr + src_base, src.nbytes, ranges)
        got = ctx.download(d_dst, d_dst.nbytes)
    finally:
        d_src.free()
        d_dst.free()
    want = np.full(d_dst.nbytes, CANARY, np.uint8)
    for s, d, n in ranges:
        want[dst_base + d:dst_base + d + n] = src[s:s + n]
    return got, want


@pytest.fixture(scope="module")
def source():
    return splitmix_bytes((4 << 20) + 4096, 0x6A7)


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 31, 33, 255, 4095, 4096, 4097, 65536 + 3])
def test_every_misalignment(gpu_ctx, source, length):
    """All 16 x 16 source / destination misalignments of one length in one call (256 ranges: four
    launches), each range in a slot of its own with canary around it."""
    slot = (length + 16 + 63) // 64 * 64 + 64
    ranges = []
    for sa in range(16):
        for da in range(16):
            i = sa * 16 + da
            ranges.append((1024 + 48 * i + sa, i * slot + 16 + da, length))
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, source[:1024 + 48 * 256 + 16 + length + 7], 256 * slot, ranges)
    assert np.array_equal(got, want)
    assert gpu_ctx.kernel_launches - before == (4 if length else 0)


def test_ranges_abutting_inside_destination_lines(gpu_ctx, source):
    rng = np.random.default_rng(11)
    ranges, d = [], 5
    for i in range(64):
        n = 1000 + i
        ranges.append((int(rng.integers(0, (4 << 20) - n)), d, n))
        d += n
    got, want = _gather(gpu_ctx, source, d + 9, ranges)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("src_base,dst_base", [(0, 0), (5, 3), (15, 9)])
def test_ranges_at_the_ends_of_the_source(gpu_ctx, source, src_base, dst_base):
    """One range ends on the source's last byte, one starts on its first, with the buffers themselves at
    unaligned addresses: the quads around those bytes leave the source buffer."""
    src = source[:70001]
    ranges = [(src.nbytes - 5000, 7, 5000), (0, 6000, 3000), (src.nbytes - 1, 5500, 1), (0, 5600, 1),
              (0, 10000, src.nbytes)]
    got, want = _gather(gpu_ctx, src, 10000 + src.nbytes, ranges, src_base, dst_base)
    assert np.array_equal(got, want)


def test_one_long_range(gpu_ctx, source):
    n = (4 << 20) + 5
    got, want = _gather(gpu_ctx, source, n + 20, [(3, 9, n)])
    assert np.array_equal(got, want)


def test_more_ranges_than_a_launch_carries(gpu_ctx, source):
    rng = np.random.default_rng(12)
    ranges, d = [], 0
    for i in range(3 * MAX_RANGES + 7):
        n = 0 if i % 17 == 5 else int(rng.integers(1, 3000))
        ranges.append((int(rng.integers(0, 1 << 20)), d, n))
        d += n + int(rng.integers(1, 40))  # a gap: no two ranges merge
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, source, d, ranges)
    assert np.array_equal(got, want)
    nonempty = sum(1 for r in ranges if r[2])
    assert gpu_ctx.kernel_launches - before == -(-nonempty // MAX_RANGES)


@pytest.mark.parametrize("bad", [(70000, 0, 2), (0, 999, 2), (1 << 40, 0, 1), (0, 0, 1 << 40)])
def test_out_of_bounds_range_is_refused_before_any_launch(gpu_ctx, source, bad):
    from libhdfs3_amd._native import Hdfs3CrcError

    src = source[:70001]
    before = gpu_ctx.kernel_launches
    with pytest.raises(Hdfs3CrcError) as ei:
        _gather(gpu_ctx, src, 1000, [(0, 0, 100), bad])
    assert ei.value.rc == -22
    assert gpu_ctx.kernel_launches == before
    # the valid range ahead of it was not copied either
    from libhdfs3_amd.engine import DeviceBuffer

    d_src, d_dst = gpu_ctx.upload(src), DeviceBuffer(1000)
    try:
        gpu_ctx.memset(d_dst, CANARY, 1000)
        with pytest.raises(Hdfs3CrcError):
            gpu_ctx.gather_dev(d_dst.ptr, 1000, d_src.ptr, src.nbytes, [(0, 0, 100), bad])
        assert np.all(gpu_ctx.download(d_dst, 1000) == CANARY)
    finally:
        d_src.free()
        d_dst.free()


# ---- hdfs3_crc32c_verify_packets_gather_dev ----------------------------------------------------------

def _wire_arena(bpc, lens, seed):
    """Packets in the wire layout ([words][data], data 16-byte aligned): (arena, descriptors, data per packet)."""
    parts, pk, datas, off = [], [], [], 0
    for i, n in enumerate(lens):
        data = splitmix_bytes(n, seed + i)
        crc = oracle_compute(data, bpc)
        pad = (-(off + crc.nbytes)) % 16
        parts += [np.zeros(pad, np.uint8), crc, data]
        pk.append((off + pad + crc.nbytes, off + pad, n))
        datas.append(data)
        off += pad + crc.nbytes + n
    return np.concatenate(parts), pk, datas


def _verify_gather(ctx, arena, pk, bpc, dst_off, check_short_tail=False):
    from libhdfs3_amd.engine import DeviceBuffer

    total = sum(p[2] for p in pk)
    d_arena, d_dst = ctx.upload(arena), DeviceBuffer(dst_off + total + 50)
    try:
        ctx.memset(d_dst, CANARY, d_dst.nbytes)
        res = ctx.verify_packets_gather_dev(d_arena.ptr, arena.nbytes, pk, bpc, d_dst.ptr, d_dst.nbytes, dst_off,
                                            check_short_tail)
        return res, ctx.download(d_dst, d_dst.nbytes)
    finally:
        d_arena.free()
        d_dst.free()


def _expect(datas, good, dst_off, size):
    want = np.full(size, CANARY, np.uint8)
    body = np.concatenate(datas[:good]) if good else np.zeros(0, np.uint8)
    want[dst_off:dst_off + body.nbytes] = body
    return want, body.nbytes


@pytest.mark.parametrize("bpc", [512, 4096])
def test_verify_packets_gather(gpu_ctx, bpc):
    lens = [8 * bpc] * 5
    arena, pk, datas = _wire_arena(bpc, lens, 900 + bpc)
    # clean: everything delivered, back to back, at an odd destination offset
    (bp, bc, placed), got = _verify_gather(gpu_ctx, arena, pk, bpc, 13)
    want, n = _expect(datas, 5, 13, got.nbytes)
    assert (bp, bc, placed) == (-1, -1, n) and np.array_equal(got, want)
    # a flipped bit in packet 3, chunk 5: packets 0-2 delivered, canary after
    bad = arena.copy()
    bad[pk[3][0] + 5 * bpc + 77] ^= 4
    (bp, bc, placed), got = _verify_gather(gpu_ctx, bad, pk, bpc, 13)
    want, n = _expect(datas, 3, 13, got.nbytes)
    assert (bp, bc, placed) == (3, 5, n) and np.array_equal(got, want)
    # a flip in packet 0: nothing is written
    bad = arena.copy()
    bad[pk[0][0] + 3] ^= 1
    (bp, bc, placed), got = _verify_gather(gpu_ctx, bad, pk, bpc, 13)
    assert (bp, bc, placed) == (0, 0, 0) and np.all(got == CANARY)


@pytest.mark.parametrize("bpc", [512, 4096])
def test_verify_packets_gather_short_tail(gpu_ctx, bpc):
    """A short last packet whose tail chunk's stored word is corrupt: ignored by remote semantics
    (check_short_tail 0: all delivered), a mismatch under local semantics (1: the packets before it)."""
    lens = [8 * bpc] * 4 + [2 * bpc + 100]
    arena, pk, datas = _wire_arena(bpc, lens, 950 + bpc)
    arena[pk[4][1] + 2 * 4] ^= 0xFF  # the word of packet 4's third (short) chunk
    (bp, bc, placed), got = _verify_gather(gpu_ctx, arena, pk, bpc, 1, check_short_tail=False)
    want, n = _expect(datas, 5, 1, got.nbytes)
    assert (bp, bc, placed) == (-1, -1, n) and np.array_equal(got, want)
    (bp, bc, placed), got = _verify_gather(gpu_ctx, arena, pk, bpc, 1, check_short_tail=True)
    want, n = _expect(datas, 4, 1, got.nbytes)
    assert (bp, bc, placed) == (4, 2, n) and np.array_equal(got, want)


def test_verify_packets_gather_refuses_a_destination_too_small(gpu_ctx):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import DeviceBuffer

    arena, pk, _ = _wire_arena(512, [4096] * 2, 990)
    d_arena, d_dst = gpu_ctx.upload(arena), DeviceBuffer(8192)
    try:
        gpu_ctx.memset(d_dst, CANARY, 8192)
        with pytest.raises(Hdfs3CrcError) as ei:
            gpu_ctx.verify_packets_gather_dev(d_arena.ptr, arena.nbytes, pk, 512, d_dst.ptr, 8192, 1)
        assert ei.value.rc == -22 and np.all(gpu_ctx.download(d_dst, 8192) == CANARY)
    finally:
        d_arena.free()
        d_dst.free()
