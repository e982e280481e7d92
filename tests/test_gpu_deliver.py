"""GPU: the guarded delivery kernel (csrc/crc32c_gather.hip) through hdfs3_deliver_verified_dev_async,
behind a real hdfs3_crc32c_verify_dev_async on the same stream. The source holds 512 bytes of padding and
then 8 KiB + 100 bytes of data (17 chunks of 512, the last one short), so chunk 0 is the source byte 512;
the stored words are the oracle's over the clean data. The expected destination is numpy slicing over a
canary-filled buffer that is downloaded whole: a byte at or past the limit that arrives, a byte below it
that does not, or a line read back and merged shows as a difference."""
import numpy as np
import pytest

from util import oracle_compute, splitmix_bytes

pytestmark = pytest.mark.gpu

CANARY = 0xC3
BPC = 512
DATA_OFF = 512
DATA_LEN = 8192 + 100
SRC_LEN = DATA_OFF + DATA_LEN + 412  # bytes behind the data too: a range may run past it
DST_LEN = 10000
CHUNK_BASE = 1000
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def clean():
    """(source buffer as uploaded, stored words of its data): computed once, never changed."""
    src = splitmix_bytes(SRC_LEN, 0xD311)
    return src, oracle_compute(src[DATA_OFF:DATA_OFF + DATA_LEN], BPC)


def flipped(src, k):
    bad = src.copy()
    bad[DATA_OFF + k * BPC + 7] ^= 0x10  # chunk 16 is the short tail: checked (check_short_tail = 1)
    return bad


def limit_of(k, granule=2048):
    return DATA_OFF + (k * BPC) // granule * granule


class Rig:
    """Device side of one test: sources, words, a canary destination and four words (result A, result B,
    gate 0, gate 1)."""

    def __init__(self, ctx, words):
        from libhdfs3_amd.engine import DeviceBuffer

        self.ctx = ctx
        self.d_crc = ctx.upload(words)
        self.d_dst = DeviceBuffer(DST_LEN + 64)
        self.d_words = DeviceBuffer(32)
        self.srcs = []
        ctx.memset(self.d_dst, CANARY, self.d_dst.nbytes)
        ctx.memset(self.d_words, 0, 32)
        self.dst = self.d_dst.ptr + 3  # the destination itself starts at an odd address
        self.res = [self.d_words.ptr, self.d_words.ptr + 8]
        self.gate = [self.d_words.ptr + 16, self.d_words.ptr + 24]

    def source(self, src):
        self.srcs.append(self.ctx.upload(src))
        return self.srcs[-1].ptr

    def set_word(self, ptr, value):
        self.ctx.upload(np.array([value & MASK], np.uint64).view(np.uint8), ptr)

    def word(self, ptr):
        return int(self.ctx.download(ptr, 8).view(np.uint64)[0])

    def verify(self, d_src, which=0):
        self.ctx.verify_dev_async(d_src + DATA_OFF, DATA_LEN, BPC, self.d_crc.ptr, self.res[which], check_short_tail=True)

    def deliver(self, d_src, ranges, which=0, granule=2048, gate_in=None, gate_out=None, **kw):
        args = dict(d_result=self.res[which], bpc=BPC, granule=granule, data_off=DATA_OFF, chunk_base=CHUNK_BASE,
                    d_gate_in=gate_in, d_gate_out=gate_out)
        args.update(kw)
        self.ctx.deliver_verified_dev(self.dst, DST_LEN, d_src, SRC_LEN, ranges, **args)

    def check(self, *parts):
        """parts = (source, ranges, limit): the bytes of every range below its limit, canary elsewhere"""
        got = self.ctx.download(self.d_dst, self.d_dst.nbytes)
        want = np.full(self.d_dst.nbytes, CANARY, np.uint8)
        for src, ranges, limit in parts:
            for s, d, n in ranges:
                m = max(0, min(n, limit - s))
                want[3 + d:3 + d + m] = src[s:s + m]
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]

    def free(self):
        for b in [self.d_crc, self.d_dst, self.d_words] + self.srcs:
            b.free()


@pytest.fixture
def rig(gpu_ctx, clean):
    r = Rig(gpu_ctx, clean[1])
    yield r
    r.free()


def test_clean_data_is_delivered_whole(rig, clean):
    src = clean[0]
    # (source - destination) mod 16 of 0, 5 and 6 (the destination starts at +3); odd destination offsets
    ranges = [(DATA_OFF + 3, 16, 1400), (2001, 3001, 2500), (5000, 5999, DATA_OFF + DATA_LEN - 5000)]
    assert [(s - (d + 3)) % 16 for s, d, _ in ranges] == [0, 5, 6]
    d_src = rig.source(src)
    rig.verify(d_src)
    rig.deliver(d_src, ranges, gate_out=rig.gate[1])
    rig.check((src, ranges, 1 << 62))
    assert rig.word(rig.gate[1]) == 0 and rig.word(rig.res[0]) == 0


def _ranges_around(limit):
    """One range that ends at the limit, one that straddles it (the limit falls 8 bytes into a 16-byte line of
    the destination, whose allocation is 256-byte aligned), one wholly past it."""
    straddle = (limit - 300, 4005 - 300, 700)
    assert (3 + straddle[1] + 300) % 16 == 8
    return [(limit - 512, 100, 512), straddle, (limit + 5, 6001, 90), (limit, 7000, 1)]


@pytest.mark.parametrize("k", [0, 3, 4, 16])
def test_a_flipped_bit_withholds_its_granule_and_everything_after(rig, clean, k):
    src = flipped(clean[0], k)
    limit = limit_of(k)
    assert limit == {0: 512, 3: 512, 4: 2560, 16: 8704}[k]
    ranges = _ranges_around(limit)
    d_src = rig.source(src)
    rig.verify(d_src)
    rig.deliver(d_src, ranges, gate_out=rig.gate[0])
    rig.check((src, ranges, limit))
    assert rig.ctx.decode_result(rig.word(rig.res[0])) == k
    assert rig.ctx.decode_result(rig.word(rig.gate[0])) == CHUNK_BASE + k


def test_a_closed_gate_writes_nothing_and_is_passed_on(rig, clean):
    src = clean[0]
    closed = ~5 & MASK
    d_src = rig.source(src)
    rig.set_word(rig.gate[0], closed)
    rig.verify(d_src)
    rig.deliver(d_src, [(DATA_OFF, 0, 4000), (100, 5000, 1)], gate_in=rig.gate[0], gate_out=rig.gate[1])
    rig.check()
    assert rig.word(rig.gate[1]) == closed and rig.word(rig.res[0]) == 0


def test_a_chain_on_one_stream_stops_at_the_first_bad_delivery(rig, clean):
    """A (bad chunk 4) then B (clean), every step enqueued before anything is read back: B's data passed its
    own verify, but the chain stopped at A, so B writes nothing and the last gate names A's chunk."""
    bad, good = flipped(clean[0], 4), clean[0]
    d_a, d_b = rig.source(bad), rig.source(good)
    ra, rb = [(DATA_OFF, 0, 4000)], [(DATA_OFF, 5000, 4000)]
    rig.verify(d_a, 0)
    rig.deliver(d_a, ra, 0, gate_in=rig.gate[0], gate_out=rig.gate[1])
    rig.verify(d_b, 1)
    rig.deliver(d_b, rb, 1, gate_in=rig.gate[1], gate_out=rig.gate[0], chunk_base=5000)
    rig.check((bad, ra, limit_of(4)), (good, rb, 0))
    assert rig.word(rig.res[1]) == 0
    assert rig.ctx.decode_result(rig.word(rig.gate[0])) == CHUNK_BASE + 4
    # and the other way round: a clean delivery first leaves the gate open for the one behind it
    rig.ctx.memset(rig.d_dst, CANARY, rig.d_dst.nbytes)
    rig.ctx.memset(rig.d_words, 0, 32)
    rig.verify(d_b, 1)
    rig.deliver(d_b, rb, 1, gate_in=rig.gate[0], gate_out=rig.gate[1], chunk_base=5000)
    rig.verify(d_a, 0)
    rig.deliver(d_a, ra, 0, gate_in=rig.gate[1], gate_out=rig.gate[0])
    rig.check((bad, ra, limit_of(4)), (good, rb, 1 << 62))
    assert rig.word(rig.gate[1]) == 0 and rig.ctx.decode_result(rig.word(rig.gate[0])) == CHUNK_BASE + 4


def test_more_ranges_than_a_launch_carries_share_one_limit(rig, clean):
    src = flipped(clean[0], 4)
    limit = limit_of(4)
    ranges = [(100 * i + 7, 16 * i + 3, 1) for i in range(70)]  # none merges: two launches
    last = [0, 1, 2, 30, 31, 32]  # the second launch's six: both launches hold ranges on both sides of the limit
    ranges = [r for i, r in enumerate(ranges) if i not in last] + [ranges[i] for i in last]
    for part in (ranges[:64], ranges[64:]):
        assert any(s < limit for s, _, _ in part) and any(s >= limit for s, _, _ in part)
    d_src = rig.source(src)
    rig.verify(d_src)
    before = rig.ctx.kernel_launches
    rig.deliver(d_src, ranges, gate_in=rig.gate[0], gate_out=rig.gate[1])
    assert rig.ctx.kernel_launches - before == 2
    rig.check((src, ranges, limit))
    assert rig.ctx.decode_result(rig.word(rig.gate[1])) == CHUNK_BASE + 4


def test_chunk_granularity(rig, clean):
    src = flipped(clean[0], 3)
    limit = limit_of(3, granule=BPC)
    assert limit == DATA_OFF + 3 * BPC
    ranges = _ranges_around(limit)
    d_src = rig.source(src)
    rig.verify(d_src)
    rig.deliver(d_src, ranges, granule=BPC, gate_out=rig.gate[0])
    rig.check((src, ranges, limit))
    assert rig.ctx.decode_result(rig.word(rig.gate[0])) == CHUNK_BASE + 3


def test_an_empty_list_still_passes_the_gate_on(rig, clean):
    d_src = rig.source(flipped(clean[0], 16))
    rig.verify(d_src)
    before = rig.ctx.kernel_launches
    rig.deliver(d_src, [], gate_out=rig.gate[1])
    rig.deliver(d_src, [(0, 0, 0)], gate_in=rig.gate[1], gate_out=rig.gate[0])
    assert rig.ctx.kernel_launches - before == 2
    rig.check()
    assert rig.ctx.decode_result(rig.word(rig.gate[1])) == CHUNK_BASE + 16
    assert rig.ctx.decode_result(rig.word(rig.gate[0])) == CHUNK_BASE + 16


@pytest.mark.parametrize("what", ["null_result", "granule_0", "bpc_0", "gate_out_is_gate_in", "gate_out_is_result",
                                  "range_past_source", "range_past_destination"])
def test_invalid_arguments_are_refused_before_any_launch(rig, clean, what):
    from libhdfs3_amd._native import Hdfs3CrcError

    d_src = rig.source(clean[0])
    rig.verify(d_src)
    ranges = [(DATA_OFF, 0, 100)]
    kw = dict(gate_in=rig.gate[0], gate_out=rig.gate[1])
    if what == "null_result":
        kw["d_result"] = None
    elif what == "granule_0":
        kw["granule"] = 0
    elif what == "bpc_0":
        kw["bpc"] = 0
    elif what == "gate_out_is_gate_in":
        kw["gate_out"] = rig.gate[0]
    elif what == "gate_out_is_result":
        kw["gate_out"] = rig.res[0]
    elif what == "range_past_source":
        ranges.append((SRC_LEN - 1, 200, 2))
    else:
        ranges.append((0, DST_LEN - 1, 2))
    before = rig.ctx.kernel_launches
    with pytest.raises(Hdfs3CrcError) as ei:
        rig.deliver(d_src, ranges, **kw)
    assert ei.value.rc == -22 and rig.ctx.kernel_launches == before
    rig.check()
    assert rig.word(rig.gate[1]) == 0
