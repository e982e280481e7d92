"""GPU parity of packet streams at their small edges (hdfs3_pkt_stream and the pitch walk behind it):
streams of one, two and three packets at every chunk size the walk serves, unit counts around the
walk's wave split and its workgroup-size switch, and the argument checks of a one-packet stream.
Everything is compared with the oracle by exact equality: every (packet, chunk) key, every computed
word, and every byte of the device allocation that must not change.

A one-packet stream used to be planned with one unit per packet, so unit u of it walked to "packet" u
at u * pitch. Every one-packet case here therefore sits in a device allocation that reaches 33 x
max(pitch, 4096) bytes past the packet, filled with a canary, while the call is given the true, smaller
arena length: a walk that leaves the packet reads and writes canary inside the allocation and shows
up as a wrong key or a changed byte."""
import numpy as np
import pytest

from test_gpu_packet_stream import build_arena, oracle_key
from util import oracle_compute

pytestmark = pytest.mark.gpu

CANARY = 0xC3  # outside the arena, and data bytes past a short last packet
BLANK = 0xA5   # word regions before a compute


@pytest.fixture(scope="module")
def res(gpu_ctx):
    from libhdfs3_amd.engine import DeviceBuffer

    buf = DeviceBuffer(8 * 8)
    yield buf
    buf.free()


class Stream:
    """n packets of plen bytes (the last one `last`) as [gap][words][data] at one pitch, the data 16-byte
    aligned, inside a canary-filled allocation image `img`; `arena_len` is what the calls are told."""

    def __init__(self, n, plen, last, bpc, seed):
        words = 4 * (-(-plen // bpc))
        gap = 32 + (-(32 + words)) % 16
        arena, self.pitch, self.crc_off, self.data_off, datas = build_arena(n, plen, last, bpc, seed, gap)
        assert self.data_off % 16 == 0 and self.pitch % 16 == 0
        self.n, self.plen, self.last, self.bpc, self.words = n, plen, last, bpc, words
        self.lens = [d.size for d in datas]
        lp = (n - 1) * self.pitch
        if n == 1:
            self.arena_len = self.data_off + last
            slack = 33 * max(self.pitch, 4096)
        else:
            self.arena_len = arena.size
            slack = 64
        self.img = np.full(self.arena_len + slack, CANARY, np.uint8)
        self.img[:self.arena_len] = arena[:self.arena_len]
        self.img[lp + self.data_off + last:] = CANARY
        self.last_words = 4 * (-(-last // bpc))
        self.img[lp + self.crc_off + self.last_words:lp + self.data_off] = CANARY

    def ps(self, pitch=None):
        from libhdfs3_amd.engine import CrcContext

        return CrcContext.packet_stream(self.crc_off, self.data_off, self.pitch if pitch is None else pitch, self.n,
                                        self.plen, self.last)

    def descs(self):
        return [(i * self.pitch + self.data_off, i * self.pitch + self.crc_off, self.lens[i]) for i in range(self.n)]

    def data_at(self, p, q):
        return p * self.pitch + self.data_off + q

    def want_key(self, local):
        """the oracle's first bad (packet, chunk) of the image as it stands"""
        datas = [self.img[self.data_at(i, 0):self.data_at(i, self.lens[i])] for i in range(self.n)]
        return oracle_key(datas, self.img, self.pitch, self.crc_off, self.bpc, local)

    def flips(self):
        """one byte in every 4 KiB unit of every packet (at a position that moves through the unit's
        chunks and lanes), each packet's last byte, and one byte inside a short tail chunk"""
        out = []
        for p, dl in enumerate(self.lens):
            for u in range(-(-dl // 4096)):
                span = min(4096, dl - u * 4096)
                out.append((p, u * 4096 + (u * 523 + p * 131 + 5) % span))
            if dl:
                out.append((p, dl - 1))
            if dl % self.bpc:
                out.append((p, dl // self.bpc * self.bpc + (dl % self.bpc) // 2))
        return out

    def blanked(self):
        """(the image with every word region blanked, what a compute must turn it into)"""
        blank, want = self.img.copy(), self.img.copy()
        for i in range(self.n):
            blank[i * self.pitch + self.crc_off:i * self.pitch + self.data_off] = BLANK
        lp = (self.n - 1) * self.pitch
        # the words of a short last packet end before its region does: the rest keeps the blank
        want[lp + self.crc_off + self.last_words:lp + self.data_off] = BLANK
        return blank, want


def decode(ctx, w):
    if w == 0:
        return -1, -1
    key = ctx.decode_result(int(w))
    return key >> 32, key & 0xFFFFFFFF


def verify_chain(ctx, res, launches, bpc, local=False):
    """launches = [(device buffer, arena_len, stream, overlap_previous)], each into its own result word"""
    ctx.memset(res, 0, 8 * len(launches))
    for i, (dev, alen, ps, overlap) in enumerate(launches):
        ctx.verify_packet_stream_async(dev.ptr, alen, ps, bpc, res.ptr + 8 * i, local, overlap_previous=overlap)
    ctx.synchronize()
    return [decode(ctx, w) for w in ctx.download(res, 8 * len(launches)).view(np.uint64).tolist()]


def verify_one(ctx, res, dev, alen, ps, bpc, local):
    return verify_chain(ctx, res, [(dev, alen, ps, False)], bpc, local)[0]


def poke(ctx, dev, s, off, mask):
    """flip bits of one byte in the image and on the device: one byte travels"""
    s.img[off] ^= mask
    ctx.upload(s.img[off:off + 1], dev, offset=off)


def check_compute(ctx, s, ps):
    blank, want = s.blanked()
    dev = ctx.upload(blank)
    ctx.compute_packet_stream_async(dev.ptr, s.arena_len, ps, s.bpc)
    got = ctx.download(dev, blank.nbytes)
    dev.free()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])} of {want.size} (arena {s.arena_len})"


# ---- a. one, two and three packets ------------------------------------------------------------------
BPCS = [512, 1024, 2048, 4096, 8192, 12288, 65536]


def small_shapes(n, bpc):
    shapes = [(65536, 65536), (65536, 65536 - 300), (65536, 65024 - 11), (65536, 4096)]
    if 4096 + bpc <= 65536:
        shapes.append((65536, 4096 + bpc))
    shapes += [(65536, 4096 * 5 + 100), (65536, 100)]
    if n > 1:
        shapes.append((65536, 0))
    shapes.append((131072, 131072 - 7))
    if bpc <= 4096:
        shapes.append((4096 * 3, 4096 * 3))
    if bpc == 12288:
        # neither 65536 nor 131072 is whole 12 KiB chunks, so no shape above reaches n > 1 at R = 3:
        # packets of 5 chunks
        shapes += [(61440, 61440), (61440, 4096 * 5 + 100)] + ([(61440, 0)] if n > 1 else [])
    # every packet but the last is whole chunks
    return [(plen, last) for plen, last in shapes if n == 1 or plen % bpc == 0]


SMALL_CASES = [(n, bpc, plen, last, mode) for n in (1, 2, 3) for bpc in BPCS for plen, last in small_shapes(n, bpc)
               for mode in (("pitch0", "pitch", "odd") if n == 1 else ("pitch",))]


@pytest.mark.parametrize("n,bpc,plen,last,mode", SMALL_CASES,
                         ids=[f"n{n}-bpc{b}-{p}-{l}-{m}" for n, b, p, l, m in SMALL_CASES])
def test_small_stream_matches_oracle(gpu_ctx, res, n, bpc, plen, last, mode):
    """mode (one packet only): pitch 0, the pitch the packet would have in a longer stream, or 7, which
    is no multiple of 16 and sends the stream to the descriptor path."""
    s = Stream(n, plen, last, bpc, 9000 + 17 * n + bpc % 1009 + plen % 97 + last % 89)
    ps = s.ps({"pitch0": 0, "pitch": None, "odd": 7}[mode])
    dev = gpu_ctx.upload(s.img)
    pk = s.descs()
    for local in (False, True):
        assert s.want_key(local) == (-1, -1)
        assert verify_one(gpu_ctx, res, dev, s.arena_len, ps, bpc, local) == (-1, -1), local
        assert gpu_ctx.verify_packets_dev(dev.ptr, s.arena_len, pk, bpc, local) == (-1, -1), local
    for p, q in s.flips():
        off = s.data_at(p, q)
        poke(gpu_ctx, dev, s, off, 0x04)
        try:
            for local in (False, True):
                want = s.want_key(local)
                # a flipped byte is seen wherever it sits, but for a short tail chunk under remote semantics
                assert want == (p, q // bpc) or (not local and q >= s.lens[p] // bpc * bpc and want == (-1, -1))
                assert verify_one(gpu_ctx, res, dev, s.arena_len, ps, bpc, local) == want, (p, q, local)
                assert gpu_ctx.verify_packets_dev(dev.ptr, s.arena_len, pk, bpc, local) == want, (p, q, local)
        finally:
            poke(gpu_ctx, dev, s, off, 0x04)
    assert verify_one(gpu_ctx, res, dev, s.arena_len, ps, bpc, True) == (-1, -1)
    assert np.array_equal(gpu_ctx.download(dev, s.img.nbytes), s.img)  # a verify writes nothing
    dev.free()
    check_compute(gpu_ctx, s, ps)


# ---- b. unit counts around the wave split -----------------------------------------------------------
# 256-thread workgroups planned at 2 rounds per wave: 1 ... 8 units are one workgroup whose 4 waves take
# 0, 1 or 2 rounds (kq = units / 4, kr = units % 4), 9 units the first grid of two, and so on
SPLIT_CASES = [(4096, n) for n in list(range(1, 21)) + [31, 32, 33]] + [(4096 * 3, n) for n in (1, 2, 3, 5, 6)]


@pytest.mark.parametrize("bpc", [512, 4096])
@pytest.mark.parametrize("plen,n", SPLIT_CASES, ids=[f"{p // 4096}r-n{n}" for p, n in SPLIT_CASES])
def test_unit_counts_around_the_wave_split(gpu_ctx, res, bpc, plen, n):
    """Each stream barriered and as the second of two chained launches, the second overlapped with the
    first (the kernel with the solo last step): a clean arena and one with a flip in its last unit, each
    launch into its own result word, in both orders. Then a compute over blanked words."""
    s = Stream(n, plen, plen, bpc, 12000 + 31 * n + bpc + plen % 101)
    ps = s.ps()
    clean = gpu_ctx.upload(s.img)
    bad = gpu_ctx.upload(s.img)
    off = s.data_at(n - 1, plen - 1 - 37)
    s.img[off] ^= 0x20
    want = s.want_key(False)
    s.img[off] ^= 0x20
    assert want == (n - 1, (plen - 1 - 37) // bpc)
    gpu_ctx.upload(s.img[off:off + 1] ^ np.uint8(0x20), bad, offset=off)
    a, b = (clean, s.arena_len, ps), (bad, s.arena_len, ps)
    assert verify_chain(gpu_ctx, res, [a + (False,)], bpc) == [(-1, -1)]
    assert verify_chain(gpu_ctx, res, [b + (False,)], bpc) == [want]
    assert verify_chain(gpu_ctx, res, [a + (False,), b + (True,)], bpc) == [(-1, -1), want]
    assert verify_chain(gpu_ctx, res, [b + (False,), a + (True,)], bpc) == [want, (-1, -1)]
    assert verify_chain(gpu_ctx, res, [a + (False,), b + (True,), a + (True,), b + (True,)], bpc) == \
        [(-1, -1), want, (-1, -1), want]
    clean.free()
    bad.free()
    check_compute(gpu_ctx, s, ps)


# ---- c. workgroup-size switch points ----------------------------------------------------------------
@pytest.mark.parametrize("bpc", [512, 4096])
@pytest.mark.parametrize("n", [256, 257, 1024, 1025])
def test_workgroup_size_switch_points(gpu_ctx, res, bpc, n):
    """64 KiB packets: 256 / 257 packets are 4096 / 4112 units and 1024 / 1025 are 16384 / 16400, either
    side of the launcher's 256-, 512- and 1024-thread workgroups. Verify barriered and overlapped with a
    flip in the first and in the last unit; at 257 and 1025 packets a compute round trip."""
    from libhdfs3_amd.engine import CrcContext

    plen = 65536
    wpp = 4 * (plen // bpc)
    crc_off, data_off = 16, 16 + wpp + (-(16 + wpp)) % 16
    pitch = data_off + plen
    host = np.random.default_rng(1000 * n + bpc).integers(0, 256, size=n * pitch, dtype=np.uint8)
    rows = host.reshape(n, pitch)
    # packets are whole chunks, so the words of all packets are the words of their data end to end
    data = np.ascontiguousarray(rows[:, data_off:])
    rows[:, crc_off:crc_off + wpp] = oracle_compute(data.reshape(-1), bpc).reshape(n, wpp)
    del data
    ps = CrcContext.packet_stream(crc_off, data_off, pitch, n, plen)
    clean = gpu_ctx.upload(host)
    bad = gpu_ctx.upload(host)
    a = (clean, host.nbytes, ps)
    b = (bad, host.nbytes, ps)
    assert verify_chain(gpu_ctx, res, [a + (False,)], bpc) == [(-1, -1)]
    for p, q in [(0, 1234), (n - 1, plen - 4096 + 2345)]:
        off = p * pitch + data_off + q
        gpu_ctx.upload(host[off:off + 1] ^ np.uint8(0x10), bad, offset=off)
        host[off] ^= 0x10
        want = oracle_key([rows[p, data_off:]], rows[p], pitch, crc_off, bpc, False)
        host[off] ^= 0x10
        assert want == (0, q // bpc)  # the oracle over the flipped packet alone: its chunk
        want = (p, want[1])
        assert verify_chain(gpu_ctx, res, [b + (False,)], bpc) == [want], (p, q)
        assert verify_chain(gpu_ctx, res, [a + (False,), b + (True,), a + (True,)], bpc) == \
            [(-1, -1), want, (-1, -1)], (p, q)
        assert verify_chain(gpu_ctx, res, [b + (False,), a + (True,)], bpc) == [want, (-1, -1)], (p, q)
        gpu_ctx.upload(host[off:off + 1], bad, offset=off)
    bad.free()
    if n in (257, 1025):
        blank = host.copy()
        blank.reshape(n, pitch)[:, crc_off:crc_off + wpp] = BLANK
        gpu_ctx.upload(blank, clean)
        del blank
        gpu_ctx.compute_packet_stream_async(clean.ptr, host.nbytes, ps, bpc)
        assert np.array_equal(gpu_ctx.download(clean, host.nbytes), host)
    clean.free()


# ---- d. argument edges at one packet ----------------------------------------------------------------
@pytest.mark.parametrize("bpc", [512, 8192])
def test_one_packet_argument_edges(gpu_ctx, res, bpc):
    from libhdfs3_amd.engine import CrcContext, Hdfs3CrcError

    s = Stream(1, 65536, 65536 - 300, bpc, 77 + bpc)
    blank, _ = s.blanked()
    dev = gpu_ctx.upload(blank)
    gpu_ctx.memset(res, 0, 8)
    before = gpu_ctx.kernel_launches
    refused = [
        # the data reaches past the arena's end (by one byte, and by far); the allocation itself holds it
        (CrcContext.packet_stream(s.crc_off, s.data_off, 0, 1, 65536, s.last), s.arena_len - 1),
        (CrcContext.packet_stream(s.crc_off, s.data_off, s.pitch, 1, 65536, 65536), s.arena_len),
        (CrcContext.packet_stream(s.crc_off, s.data_off, 0, 1, 65536, s.last), s.data_off),
        # last_len above data_len
        (CrcContext.packet_stream(s.crc_off, s.data_off, 0, 1, 4096, 8192), s.arena_len),
        (CrcContext.packet_stream(s.crc_off, s.data_off, s.pitch, 1, s.last - 1, s.last), s.arena_len),
    ]
    for ps, alen in refused:
        with pytest.raises(Hdfs3CrcError):
            gpu_ctx.verify_packet_stream_async(dev.ptr, alen, ps, bpc, res.ptr)
        with pytest.raises(Hdfs3CrcError):
            gpu_ctx.compute_packet_stream_async(dev.ptr, alen, ps, bpc)
    # no packet at all: nothing to do, whatever the other fields say
    empty = CrcContext.packet_stream(s.crc_off, s.data_off, 0, 0, 65536, 65536)
    gpu_ctx.verify_packet_stream_async(dev.ptr, s.arena_len, empty, bpc, res.ptr)
    gpu_ctx.compute_packet_stream_async(dev.ptr, s.arena_len, empty, bpc)
    gpu_ctx.synchronize()
    assert gpu_ctx.kernel_launches == before
    assert not gpu_ctx.download(res, 8).any()
    assert np.array_equal(gpu_ctx.download(dev, blank.nbytes), blank)
    dev.free()
