"""GPU: the gather with a source per range (csrc/crc32c_gather.hip, its third instantiation) through
hdfs3_gather_sources_dev_async. As in test_gpu_gather.py the expected destination is numpy slicing over a
canary-filled buffer that is downloaded whole, so a byte written outside a range, or a line read back and
merged, shows as a damaged canary or a damaged neighbour; the sources are separate allocations, downloaded
after every call and compared. That no load leaves a range's own bytes cannot be shown by a passing run
(allocations are page-granular): it is the kernel's `fast` condition against [src_b, src_e), which in this
instantiation are the range's own first byte and end, and the same test in front of every byte load."""
import numpy as np
import pytest

from util import splitmix_bytes

pytestmark = pytest.mark.gpu

CANARY = 0xA5
MAX_RANGES = 64  # kGatherMaxRanges (csrc/launch_plan.h)
SIZES = [(4 << 20) + 4096, 90000, 80001, 70001]  # the allocations ranges are read from


class Sources:
    def __init__(self, ctx):
        self.ctx = ctx
        self.host = [splitmix_bytes(n, 0x51C + i) for i, n in enumerate(SIZES)]
        self.dev = [ctx.upload(h) for h in self.host]

    def ptr(self, a, off):
        return self.dev[a].ptr + off

    def check_unchanged(self):
        for h, d in zip(self.host, self.dev):
            assert np.array_equal(self.ctx.download(d, h.nbytes), h)

    def free(self):
        for d in self.dev:
            d.free()


@pytest.fixture(scope="module")
def sources(gpu_ctx):
    s = Sources(gpu_ctx)
    yield s
    s.free()


def _gather(ctx, srcs, dst_len, ranges, dst_base=0):
    """ranges = [(allocation, src_off, dst_off, len)] into a canary destination that starts at +dst_base of
    its allocation; returns (destination as downloaded, expected). Every source is compared afterwards."""
    from libhdfs3_amd.engine import DeviceBuffer

    d_dst = DeviceBuffer(dst_len + dst_base + 64)
    try:
        ctx.memset(d_dst, CANARY, d_dst.nbytes)
        ctx.gather_sources_dev(d_dst.ptr + dst_base, dst_len, [(srcs.ptr(a, s), d, n) for a, s, d, n in ranges])
        got = ctx.download(d_dst, d_dst.nbytes)
    finally:
        d_dst.free()
    want = np.full(dst_len + dst_base + 64, CANARY, np.uint8)
    for a, s, d, n in ranges:
        want[dst_base + d:dst_base + d + n] = srcs.host[a][s:s + n]
    srcs.check_unchanged()
    return got, want


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 31, 33, 255, 4095, 4096, 4097, 65536 + 3])
def test_every_misalignment(gpu_ctx, sources, length):
    """All 16 x 16 source / destination misalignments of one length in one call (256 ranges: four launches),
    consecutive ranges from three separate allocations in turn, each in a destination slot of its own with
    canary around it."""
    slot = (length + 16 + 63) // 64 * 64 + 64
    ranges = []
    for sa in range(16):
        for da in range(16):
            i = sa * 16 + da
            ranges.append((i % 3, 1024 + 48 * i + sa, i * slot + 16 + da, length))
    assert all(sources.ptr(a, s) % 16 == i // 16 for i, (a, s, _, _) in enumerate(ranges))
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, sources, 256 * slot, ranges)
    assert np.array_equal(got, want)
    assert gpu_ctx.kernel_launches - before == (4 if length else 0)


def test_ranges_abutting_inside_destination_lines(gpu_ctx, sources):
    rng = np.random.default_rng(21)
    ranges, d = [], 5
    for i in range(64):
        n = 1000 + i
        ranges.append((i % 3, int(rng.integers(0, SIZES[i % 3] - n)), d, n))
        d += n
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, sources, d + 9, ranges, dst_base=3)
    assert np.array_equal(got, want)
    assert gpu_ctx.kernel_launches - before == 1


@pytest.mark.parametrize("dst_base", [0, 3, 9])
def test_ranges_at_the_ends_of_an_allocation(gpu_ctx, sources, dst_base):
    """A range that is the last byte of an allocation of 70001 bytes and one that is its first byte, ranges that
    end on its last and start on its first byte, and the whole allocation: the quads around those bytes
    leave the range."""
    n = SIZES[3]
    assert n == 70001
    ranges = [(3, n - 1, 5500, 1), (3, 0, 5600, 1), (3, n - 5000, 7, 5000), (3, 0, 6000, 3000), (3, n - 17, 9100, 17),
              (3, 0, 10000, n)]
    got, want = _gather(gpu_ctx, sources, 10000 + n, ranges, dst_base)
    assert np.array_equal(got, want)


def test_one_long_range(gpu_ctx, sources):
    n = (4 << 20) + 5
    got, want = _gather(gpu_ctx, sources, n + 20, [(0, 3, 9, n)])
    assert np.array_equal(got, want)


def test_more_ranges_than_a_launch_carries(gpu_ctx, sources):
    rng = np.random.default_rng(22)
    ranges, d = [], 0
    for i in range(3 * MAX_RANGES + 7):
        n = 0 if i % 17 == 5 else int(rng.integers(1, 3000))
        ranges.append((i % 4, int(rng.integers(0, 60000)), d, n))
        d += n + int(rng.integers(1, 40))  # a gap: no two ranges merge
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, sources, d, ranges)
    assert np.array_equal(got, want)
    nonempty = sum(1 for r in ranges if r[3])
    assert gpu_ctx.kernel_launches - before == -(-nonempty // MAX_RANGES)


def test_address_adjacent_ranges_merge_into_one_launch(gpu_ctx, sources):
    """200 ranges that continue each other in source address and in the destination are one planned range:
    one launch where 200 apart would take four."""
    ranges = [(1, 11 + 100 * i, 5 + 100 * i, 100) for i in range(200)]
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, sources, 20100, ranges, dst_base=1)
    assert np.array_equal(got, want)
    assert gpu_ctx.kernel_launches - before == 1
    apart = [(1, 11 + 101 * i, 5 + 100 * i, 100) for i in range(200)]  # a byte between them in memory
    before = gpu_ctx.kernel_launches
    got, want = _gather(gpu_ctx, sources, 20100, apart, dst_base=1)
    assert np.array_equal(got, want)
    assert gpu_ctx.kernel_launches - before == 4


@pytest.mark.parametrize("bad", ["past_dst", "dst_off_past_dst", "huge_len", "null_src", "wrapping_src"])
def test_a_bad_range_is_refused_before_any_launch(gpu_ctx, sources, bad):
    from libhdfs3_amd._native import Hdfs3CrcError
    from libhdfs3_amd.engine import DeviceBuffer

    p = sources.ptr(1, 0)
    bad_range = {"past_dst": (p, 999, 2), "dst_off_past_dst": (p, 1001, 0), "huge_len": (p, 0, 1 << 40),
                 "null_src": (None, 200, 1), "wrapping_src": ((1 << 64) - 4, 200, 8)}[bad]
    d_dst = DeviceBuffer(1000)
    try:
        gpu_ctx.memset(d_dst, CANARY, 1000)
        before = gpu_ctx.kernel_launches
        with pytest.raises(Hdfs3CrcError) as ei:
            gpu_ctx.gather_sources_dev(d_dst.ptr, 1000, [(p, 0, 100), bad_range])
        assert ei.value.rc == -22
        assert gpu_ctx.kernel_launches == before
        # the valid range ahead of it was not copied either
        assert np.all(gpu_ctx.download(d_dst, 1000) == CANARY)
        # an empty range may have a null source, and an all-empty list needs no destination
        gpu_ctx.gather_sources_dev(d_dst.ptr, 1000, [(None, 1000, 0), (p, 0, 0)])
        gpu_ctx.gather_sources_dev(None, 0, [(None, 0, 0)])
        with pytest.raises(Hdfs3CrcError) as ei:
            gpu_ctx.gather_sources_dev(None, 1000, [(p, 0, 1)])
        assert ei.value.rc == -22
        assert gpu_ctx.kernel_launches == before
        assert np.all(gpu_ctx.download(d_dst, 1000) == CANARY)
    finally:
        d_dst.free()
    sources.check_unchanged()
